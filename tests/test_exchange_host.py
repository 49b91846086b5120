"""Multi-compartment exchange (epg.X) and the MT helpers on the host: tables, shapes, errors and the encoded plan
(G17 from the reference, tests/golden/make_golden_exchange.py).  No GPU needed."""
import os

import numpy as np
import pytest

from epgpy_amd import epg, exchange, magnettransfer, _lib
from epgpy_amd import functions as _functions

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "g17_exchange.npz"))


def close(a, b, rtol=1e-14):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(np.max(np.abs(b))), 1e-300)
    assert float(np.max(np.abs(a - b))) <= rtol * scale, float(np.max(np.abs(a - b))) / scale


def test_tables_match_reference():
    close(epg.X(5, 0.01, T1=[1000, 500], T2=[100, 20]).mat, GOLDEN["tab_scalar"])
    kmat3 = GOLDEN["kmat3"]
    close(epg.X(7, kmat3, T1=[800, 1000, 300], T2=[60, 80, 15], g=[0, 0.01, -0.02]).mat, GOLDEN["tab_n3"])
    x = epg.X(5, GOLDEN["khi_ax1"], axis=1, T1=[[900, 400]], T2=[[70, 25]])
    assert x.axis == int(GOLDEN["tab_ax1_axis"]) == 1
    close(x.mat, GOLDEN["tab_ax1"])
    xa = epg.X(GOLDEN["tab_arr_in"], 0.01, T1=[1000, 500], T2=[100, 20], g=[[0.0], [0.05]])
    close(xa.mat, GOLDEN["tab_arr"])
    assert xa.shape == tuple(GOLDEN["tab_arr_shape"]) == (2, 3)
    assert epg.X(4.5, 0.01, duration=True).duration == float(GOLDEN["dur_true"]) == 4.5


def test_exchange_matrix_and_expm():
    close(exchange.exchange_matrix(2e-3, densities=[0.8, 0.2]), GOLDEN["exm_dens"])
    close(exchange.exchange_matrix([1e-3, 2e-3, 5e-3], axis=1, ncomp=2), GOLDEN["exm_k"])
    close(exchange.exchange_matrix(0.02, ncomp=3), GOLDEN["exm_n3"])
    close(exchange.expm(GOLDEN["expm_in"]), GOLDEN["expm_out"])
    close(exchange.expm(GOLDEN["expm_herm_in"]), GOLDEN["expm_herm_out"])
    A = np.random.default_rng(3).uniform(-1, 1, (4, 4))
    np.testing.assert_allclose(exchange.expm(A) @ exchange.expm(-A), np.eye(4), atol=1e-13)
    assert np.array_equal(exchange.expm(np.zeros((3, 3))), np.eye(3))
    with pytest.raises(ValueError):
        exchange.exchange_matrix(-1.0)


def test_mt_helpers():
    close(magnettransfer.saturation_rate(0.5, 13.0, 15.1e-3), GOLDEN["mt_sat_hard"])
    close(magnettransfer.saturation_rate(2.0, GOLDEN["mt_sat_wave_in"], 15.1e-3), GOLDEN["mt_sat_wave"])
    for shape in ("gaussian", "lorentzian", "super-lorentzian"):
        close(magnettransfer.absorption_rate(12e-3, shape, GOLDEN["mt_offres"]), GOLDEN[f"mt_abs_{shape}"])
    with pytest.raises(ValueError):
        magnettransfer.absorption_rate(12e-3, "voigt")


def test_shapes_axes_and_errors():
    x = epg.X(5, 0.01)
    assert x.shape == (2,) and x.axis == 0 and x.ncomp == 2 and x.mat.shape == (2, 2, 3)
    x3 = epg.X(5, exchange.exchange_matrix(0.02, ncomp=3), T2=[50, 60, 70], axis=-1)
    assert x3.axis == 0 and x3.shape == (3,)
    xg = epg.X(5, 0.01, g=[np.linspace(-0.1, 0.1, 7)])
    assert xg.shape == (2, 7)
    assert epg.X(5, 0.01).duration == 0 and epg.X(5, 0.01, duration=3).duration == 3
    assert epg.X is exchange.X and "X" in repr(x)
    with pytest.raises(ValueError, match="at least 2D"):
        epg.X(5, [0.1, 0.2])
    with pytest.raises(ValueError, match="square"):
        epg.X(5, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="sum to 0"):
        epg.X(5, [[0.1, -0.1], [0.2, 0.1]])


def test_encoded_plan():
    """one OP_X record per X: ia = N, ib = compartment stride, 3 N^2 doubles per entry, one entry per group"""
    offres = np.linspace(-0.1, 0.1, 5)
    x = epg.X(5, 0.01, T1=[1000, 500], T2=[100, 20], g=[offres])            # compartments on axis 0 of a (2, 5) grid
    seq = [epg.T(10, 90), x, epg.S(1), epg.ADC]
    enc, _, _ = _functions.compile_sequence(seq)
    assert enc.grid == (2, 5)
    recs = [r for r in enc.records if r[0] == _lib.OP_X]
    assert len(recs) == 1
    opcode, space, ia, ib, off, ncoef = recs[0]
    assert (ia, ib, ncoef) == (2, 5, 12)
    assert enc.spaces[space] == (0, 1)                   # stride 0 on the compartment axis
    ops, grid, spaces, coef, _ = enc.arrays(64)
    tab = coef[off: off + 5 * 12].reshape(5, 12)
    mT = np.moveaxis(x.mat[..., 0], (0, 1), (-2, -1))     # [5, 2, 2]
    assert np.array_equal(tab[:, 0:8:2], mT.real.reshape(5, 4)) and np.array_equal(tab[:, 1:8:2], mT.imag.reshape(5, 4))
    assert np.array_equal(tab[:, 8:], np.moveaxis(x.mat[..., 2], (0, 1), (-2, -1)).real.reshape(5, 4))
    # compartments on axis 1 of a (3, 2) grid: stride 1; three compartments: 27 doubles
    x1 = epg.X(5, GOLDEN["khi_ax1"], axis=1)
    enc1, _, _ = _functions.compile_sequence([x1, epg.ADC])
    assert [r[2:4] for r in enc1.records if r[0] == _lib.OP_X] == [(2, 1)]
    enc3, _, _ = _functions.compile_sequence([epg.X(5, GOLDEN["kmat3"]), epg.ADC])
    assert [(r[2], r[5]) for r in enc3.records if r[0] == _lib.OP_X] == [(3, 27)]
    # X plans keep their states in HBM: no 16 / 32-order packing, no 2048-order resident capacity
    assert enc.packable() == 0 and enc.capacity() == 64


def test_out_of_scope_raises_naming_x():
    x2 = epg.X(5, 0.01)
    with pytest.raises(NotImplementedError, match="X"):
        _functions.compile_sequence([x2, epg.ADC, epg.X(5, exchange.exchange_matrix([0.01, 0.02], axis=1), axis=1), epg.ADC])
    with pytest.raises(NotImplementedError, match="X"):      # n-D shift vectors that differ between the compartments
        _functions.compile_sequence([epg.T(90, 90), epg.S([[1, 0], [2, 0]]), x2, epg.ADC])
    seq = [epg.T(10, 90), x2, epg.ADC]
    with pytest.raises(NotImplementedError, match="X"):
        _functions._check_exchange(seq, [epg.Jacobian("T2")], None, "host", [0])
    with pytest.raises(NotImplementedError, match="X"):
        _functions._check_exchange(seq, [], None, "device", [0])
    with pytest.raises(NotImplementedError, match="X"):
        _functions._check_exchange(seq, [], None, "host", [0, 1])
    assert _functions.has_exchange(seq) and not _functions.has_exchange([epg.T(10, 90), epg.ADC])


# ------------------------------------------------------------------------------------------------ extended-precision reference
def _golden_sim_case(name):
    from tests.test_gpu_exchange import _sim_cases     # (the G17 sequences; that module's tests stay GPU-marked)
    seq, opts, dens = _sim_cases()[name]
    flat = _functions.flatten_sequence(seq)
    nshift = sum(abs(op.k) for op in flat if isinstance(op, epg.S))
    nmax = min(nshift, opts.get("max_nstate", nshift)) + 1
    reduce = [op.reduce for op in flat if isinstance(op, epg.Probe)][0]
    return flat, _functions.getshape(flat), dens, nmax, opts.get("max_nstate"), reduce


@pytest.mark.parametrize("name", ["sim_spgr_bm", "sim_spgr_bm_sum", "sim_spgr_mt_sum", "sim_bssfp_bm", "sim_se3", "sim_axis1"])
def test_extended_recurrence_matches_golden(name):
    """the clongdouble recurrence (with truncation at max_nstate and T @ R matrices) reproduces the G17 signals to 1e-13"""
    from tests.exchange_recurrence import recurrence
    seq, grid, dens, nmax, max_nstate, reduce = _golden_sim_case(name)
    want = GOLDEN[name]
    got = recurrence(seq, grid, dens, nmax, dtype=np.clongdouble, max_nstate=max_nstate)
    assert got.dtype == np.clongdouble
    if reduce is not None:
        got = got.sum(axis=tuple(1 + int(ax) for ax in np.atleast_1d(reduce)))
    assert float(np.max(np.abs(got - want))) <= 1e-13 * max(1.0, float(np.max(np.abs(want))))


@pytest.mark.parametrize("seed", range(24))
def test_extended_against_float64_recurrence(seed):
    """the float64 recurrence (the checker of test_random_sequences) within 1e-13 of the extended-precision one: the
    float64 rounding the GPU tolerance has to absorb"""
    from tests.exchange_recurrence import recurrence, random_case
    seq, grid, dens, nmax = random_case(seed)
    r64 = recurrence(seq, grid, dens, nmax)
    rext = recurrence(seq, grid, dens, nmax, dtype=np.clongdouble)
    assert r64.dtype == np.complex128
    assert float(np.max(np.abs(r64 - rext))) <= 1e-13 * max(1.0, float(np.max(np.abs(rext))))


def test_recurrence_reset_pd_z0_truncation():
    """the operators the device tests lean on, against hand-derived states: RESET / PD restore [0, 0, rho]; PD(reset=False)
    changes only the equilibrium X and E relax to; Z0 probes; F+ / F- cut above max_nstate; a start state"""
    from tests.exchange_recurrence import recurrence
    dens = np.array([0.7, 0.3])
    x = epg.X(4.0, exchange.exchange_matrix(0.05, densities=dens), T1=[900, 300], T2=[80, 20], g=[0.01, -0.02])
    seq = [epg.T(90, 0), epg.S(1), epg.RESET, epg.ADC, epg.Adc("Z0"), epg.T(30, 0), epg.PD([0.2, 0.5]), epg.Adc("Z0")]
    r = recurrence(seq, (2,), dens, 2, dtype=np.clongdouble)
    assert np.array_equal(r[0], [0, 0]) and np.array_equal(r[1], dens) and np.array_equal(r[2], [0.2, 0.5])
    # PD without reset: X then relaxes Z0 towards the new densities (a fixed point of X)
    seq = [epg.PD([0.2, 0.5], reset=False), x, epg.Adc("Z0")]
    r = recurrence(seq, (2,), dens, 1, dtype=np.clongdouble)
    mL = np.moveaxis(x.mat[..., 2], (0, 1), (-2, -1)).real
    want = mL @ (dens - [0.2, 0.5]) + [0.2, 0.5]
    assert float(np.max(np.abs(r[0] - want))) <= 1e-15
    # truncation: a 90 pulse then S(1), S(1): F+ at order 2 is dropped with max_nstate=1, kept without
    seq = [epg.T(90, 90), epg.S(1), epg.S(1), epg.S(-1), epg.S(-1), epg.ADC]
    full = recurrence(seq, (1,), 1.0, 3, dtype=np.clongdouble)
    cut = recurrence(seq, (1,), 1.0, 3, dtype=np.clongdouble, max_nstate=1)
    assert abs(full[0, 0] - 1) <= 1e-15 and cut[0, 0] == 0
    cut_op = recurrence([epg.T(90, 90), epg.S(1, nmax=1), epg.S(1, nmax=1), epg.S(-1), epg.S(-1), epg.ADC], (1,), 1.0, 3)
    assert cut_op[0, 0] == 0
    # a start state: F+(1) = 1 comes back to k = 0 after S(-1), with the density of the start state
    init = np.zeros((3, 3), dtype=complex)
    init[2, 0] = 1.0       # F+(1)
    init[0, 1] = 1.0       # F-(-1) = conj(F+(1))
    r = recurrence([epg.S(-1), epg.ADC, epg.RESET, epg.Adc("Z0")], (1,), 0.4, 2, init=init, dtype=np.clongdouble)
    assert r[0, 0] == 1 and r[1, 0] == 0.4


def test_recurrence_float64_default_unchanged():
    """dtype=complex128 (the default) keeps the recurrence's float64 results"""
    from tests.exchange_recurrence import recurrence, random_case
    seq, grid, dens, nmax = random_case(3)
    a = recurrence(seq, grid, dens, nmax)
    b = recurrence(seq, grid, dens, nmax, dtype=np.complex128)
    assert a.dtype == np.complex128 and np.array_equal(a, b)
