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
