"""GPU: float wavenumbers on the device -- the two kernels of the shift-merge against NumPy, the reference's recorded results
through simulate() and through op(sm), the T2* known answer, and the errors."""
import ctypes

import numpy as np
import pytest

from epgpy_amd import epg, kmerge, _lib
from tests import merge_cases, merge_oracle

pytestmark = pytest.mark.gpu

NVOX = (1, 3, 70, 4099)          # 4099 voxels: more than one block of partials (256 voxels per block)
TOL = 1e-12                      # the project's standing tolerance on O(1) signals


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def random_half(nvox, K, seed):
    rng = np.random.default_rng(seed)
    half = rng.normal(size=(nvox, 3, K)) + 1j * rng.normal(size=(nvox, 3, K))
    half *= 10.0 ** rng.uniform(-6, 1, size=(1, 1, K))       # rows of very different size
    return half


def device_state(half):
    st = _lib.DeviceState(_lib.get_context(), half.shape[0], half.shape[2])
    st.upload(half, np.linspace(0.5, 1.5, half.shape[0]))
    return st


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("K", (64, 128))
@pytest.mark.parametrize("nvox", NVOX)
def test_row_stats_against_numpy(K, nvox):
    half = random_half(nvox, K, seed=K + nvox)
    st, ctx = device_state(half), _lib.get_context()
    for nrow in (K, K - 23, 1):
        sums, maxabs = _lib.state_row_stats(ctx, st, nrow)
        again = _lib.state_row_stats(ctx, st, nrow)
        want_sums, want_max = merge_oracle.row_stats(half, nrow)
        err = np.abs(sums - want_sums).max() / want_sums.max()
        print(f"row_stats K={K} nvox={nvox} nrow={nrow}: sums rel err {np.abs(sums / want_sums - 1).max():.2e}")
        assert sums.shape == (3, nrow) and np.all(np.abs(sums - want_sums) <= 1e-13 * want_sums), err
        assert np.array_equal(bits(maxabs), bits(want_max))                      # maxima exactly
        assert np.allclose(sums, np.abs(half[:, :, :nrow]).sum(axis=0), rtol=1e-13)
        assert np.allclose(maxabs, np.abs(half[:, :, :nrow]).max(axis=(0, 1)), rtol=5e-16)
        assert np.array_equal(bits(sums), bits(again[0])) and np.array_equal(bits(maxabs), bits(again[1]))   # two calls, equal bits


def hand_table(Ks, Kd, nrow):
    """empty destinations; one with three sources (one conjugated, one from the other transverse component); orders >= 64
    when the source has them; the last destination order in use"""
    C, SH = _lib.GS_CONJ, _lib.MERGE_COMP_SHIFT
    top = Ks - 1
    lists = [[[] for _ in range(nrow)] for _ in range(3)]
    lists[0][0] = [3, 5 | (1 << SH) | C, top]                              # A_0 <- A_3 + conj(B_5) + A_top
    lists[0][2] = [1 | (1 << SH)]                                          # A_2 <- B_1
    lists[0][nrow - 1] = [top | C, 0, 7 | (2 << SH)]                       # last order <- conj(A_top) + A_0 + Z_7
    lists[1][1] = [2 | C, 2 | (1 << SH), 2 | (1 << SH) | C, top | (1 << SH)]
    lists[2][0] = [0 | (2 << SH), (top // 2) | (2 << SH) | C]
    lists[2][nrow - 2] = [top | (2 << SH)]
    offsets, sources = np.zeros((3, nrow + 1), np.int32), []
    for c in range(3):
        offsets[c, 0] = len(sources)
        for j in range(nrow):
            sources += lists[c][j]
            offsets[c, j + 1] = len(sources)
    return offsets, np.asarray(sources, np.int32)


@pytest.mark.parametrize("Ks,Kd", ((64, 64), (128, 64), (64, 128)))
@pytest.mark.parametrize("nvox", NVOX)
def test_merge_against_numpy_bit_for_bit(Ks, Kd, nvox):
    ctx = _lib.get_context()
    half = random_half(nvox, Ks, seed=Ks + Kd + nvox)
    src = device_state(half)
    for nrow in (Kd, Kd - 13):
        offsets, sources = hand_table(Ks, Kd, nrow)
        dst = device_state(random_half(nvox, Kd, seed=1))             # (garbage that the merge must overwrite)
        _lib.state_merge(ctx, dst, src, nrow, offsets, sources)
        got, dens = dst.download()
        want = merge_oracle.apply_table(half, offsets, sources, Kd)
        assert np.array_equal(bits(got), bits(want))
        assert not np.any(got[:, :, nrow:]) and not np.any(got[:, 1, 2:]) and np.any(got[:, 0, 0])
        assert np.array_equal(dens, np.linspace(0.5, 1.5, nvox))      # dst takes the densities of src
    back, _ = src.download()
    assert np.array_equal(bits(back), bits(half))


def test_merge_argument_checks():
    ctx = _lib.get_context()
    src, dst = device_state(random_half(2, 64, 0)), device_state(random_half(2, 64, 1))
    offsets, sources = hand_table(64, 64, 10)
    with pytest.raises(NotImplementedError, match="kgrid"):           # more than 1024 stored orders: the entry point's own check
        _lib.state_merge(ctx, dst, src, 1025, np.zeros((3, 1026), np.int32), np.zeros(0, np.int32))
    with pytest.raises(_lib.EpgxError, match="must differ"):
        _lib.state_merge(ctx, src, src, 10, offsets, sources)
    with pytest.raises(_lib.EpgxError, match="nrow_dst"):
        _lib.state_merge(ctx, dst, src, 65, np.zeros((3, 66), np.int32), np.zeros(0, np.int32))
    bad = sources.copy()
    bad[0] = 64                                                        # an order outside the source
    with pytest.raises(_lib.EpgxError, match="order 64"):
        _lib.state_merge(ctx, dst, src, 10, offsets, bad)
    bad[0] = 3 << _lib.MERGE_COMP_SHIFT                               # a component that does not exist
    with pytest.raises(_lib.EpgxError, match="component 3"):
        _lib.state_merge(ctx, dst, src, 10, offsets, bad)
    off = offsets.copy()
    off[1, 3] = off[1, 2] - 1
    with pytest.raises(_lib.EpgxError, match="CSR"):
        _lib.state_merge(ctx, dst, src, 10, off, sources)
    with pytest.raises(_lib.EpgxError, match="nvox mismatch"):
        _lib.state_merge(ctx, device_state(random_half(3, 64, 2)), src, 10, offsets, sources)
    with pytest.raises(_lib.EpgxError, match="nrow"):
        _lib.state_row_stats(ctx, src, 65)
    got, _ = dst.download()
    assert np.array_equal(bits(got), bits(random_half(2, 64, 1)))     # nothing was launched


# ------------------------------------------------------------------------------------------------ T2* known answer
def test_t2star_one_voxel_known_answer():
    seq = [epg.T(30, 90)] + [epg.C(0.5, 1 / 5), epg.ADC] * 20
    sig = epg.simulate(seq, kgrid=0.1)
    want = 0.5 * np.exp(-0.1 * np.arange(1, 21))
    print("t2star max abs err", np.abs(np.asarray(sig).reshape(-1) - want).max())
    assert np.asarray(sig).shape == (20, 1) and np.abs(np.asarray(sig).reshape(-1) - want).max() <= TOL


def test_t2star_70_voxels_golden(golden):
    g = golden("g22_merge")
    ops, opts = merge_cases.build(epg, "t2star")
    sig = epg.simulate(ops, **opts)
    assert sig.shape == g["t2star_signal"].shape and np.abs(sig - g["t2star_signal"]).max() <= TOL
    sm = run_ops(ops, opts)
    assert sm.kdim == 4 and sm.coords.dtype == np.float64 and np.allclose(sm.t.reshape(-1)[sm.nstate:].max(), 2.0)
    assert np.abs(sm.F0 - g["t2star_signal"][-1]).max() <= TOL


# ------------------------------------------------------------------------------------------------ golden cases
def run_ops(ops, opts):
    sm = epg.StateMatrix(shape=epg.getshape(ops), **opts)
    for op in epg.flatten_sequence(ops):
        sm = op(sm, inplace=True)
    return sm


def match_final(sm, g, name):
    states, coords = g[name + "_states"], g[name + "_coords"]
    assert sm.states.shape == states.shape and sm.coords.shape == coords.shape and sm.coords.dtype == np.float64
    print(name, "states err", np.abs(sm.states - states).max(), "coords rel err", np.abs(sm.coords - coords).max() / np.abs(coords).max())
    assert np.abs(sm.states - states).max() <= TOL
    assert np.abs(sm.coords - coords).max() <= 1e-12 * np.abs(coords).max()
    assert sm.check()


@pytest.mark.parametrize("name", ("grad3d_1", "grad3d_5", "grad3d_70", "multi1d", "long1d", "mixed"))
def test_golden_cases_through_simulate_and_operators(golden, name):
    g = golden("g22_merge")
    ops, opts = merge_cases.build(epg, name)
    sig = epg.simulate(ops, **opts)
    print(name, "signal err", np.abs(sig - g[name + "_signal"]).max())
    assert sig.shape == g[name + "_signal"].shape and np.abs(sig - g[name + "_signal"]).max() <= TOL
    assert np.array_equal(epg.simulate(ops, mode="stepwise", **opts), sig)
    sm = run_ops(ops, opts)
    match_final(sm, g, name)
    if name == "long1d":
        assert sm.nstate + 1 > 64 and sm._state.K == 128
    # the state matrix hands its float coordinates over and carries on (statematrix.py:58-64)
    again = epg.StateMatrix(sm.states, coords=sm.coords, **opts)
    assert again.coords.dtype == np.float64 and np.array_equal(again.coords, sm.coords) and again.nstate == sm.nstate


def test_hyperecho_through_shift_merge():
    """the reference's hyper-echo with float wavenumbers (test/test_shift.py:302-312): everything refocuses into F0"""
    necho = 100
    alphas = np.linspace(10, 80, necho)
    grad = epg.S([1.11, -2.29, 0.41])
    seq = [epg.T(90, 90)] + sum([[grad, epg.T(a, 0)] for a in alphas], start=[])
    seq += [grad, epg.T(180, 0)] + sum([[grad, epg.T(-a, 0)] for a in alphas[::-1]], start=[]) + [grad]
    sm = epg.StateMatrix(kgrid=1)
    for op in seq:
        sm = op(sm, inplace=True)
    states = sm.states
    assert np.allclose(states[:, sm.nstate], [1, 1, 0]) and np.allclose(states[:, :sm.nstate], 0)
    assert np.allclose(sm.F0, 1) and np.allclose(sm.Z0, 0)


# ------------------------------------------------------------------------------------------------ errors
def test_float_shift_errors_on_the_device_paths():
    seq = [epg.T(30, 90), epg.S(1.5), epg.ADC]
    for kwargs in (dict(mode="resident"), dict(mode="stream"), dict(out="device")):
        with pytest.raises(ValueError, match="device-recordable"):
            epg.simulate(seq, kgrid=1, **kwargs)
    with pytest.raises(NotImplementedError, match="ngpu > 1"):
        epg.simulate(seq, kgrid=1, ngpu=2)
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.simulate(seq)
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.S(1.5)(epg.StateMatrix())
    with pytest.raises(NotImplementedError, match="option kgrid="):       # simulate(): the grid of a run is its option ...
        epg.simulate([epg.T(30, 90), epg.S(1.5, kgrid=1), epg.ADC])
    sm = epg.S(1.5, kgrid=1)(epg.T(30, 90)(epg.StateMatrix()))           # ... op(sm) honours the operator's own
    assert sm.coords.dtype == np.float64 and np.allclose(sm.coords.reshape(-1), [-1.5, 0, 1.5])
    assert np.array_equal(epg.simulate([epg.T(30, 90), epg.S(1.5, kgrid=2), epg.ADC], kgrid=1),
                          epg.simulate([epg.T(30, 90), epg.S(1.5), epg.ADC], kgrid=1))      # the option wins (shift.py:130)
    with pytest.raises(NotImplementedError, match="float shift"):
        epg.simulate([epg.T(30, 90, order1="alpha"), epg.S(1.5), epg.ADC], probe=epg.Jacobian("alpha"), kgrid=1)
    with pytest.raises(NotImplementedError, match="shift-prune"):
        epg.S([[1.5], [0.5]], kgrid=1)(epg.StateMatrix(shape=(2,)))
    with pytest.raises(NotImplementedError, match="shift-prune"):
        epg.simulate([epg.T(30, 90), epg.C(0.5, [0.1, 0.2]), epg.ADC], kgrid=0.1)
    from epgpy_amd.exchange import X
    with pytest.raises(NotImplementedError, match="X"):
        epg.simulate([epg.T(30, 90), X(5, 0.01), epg.S(1.5), epg.ADC], kgrid=1)
    with pytest.raises(NotImplementedError, match="general equilibrium"):
        epg.S(1.5, kgrid=1)(epg.StateMatrix(equilibrium=[[0, 0, 0.5], [0.1, 0.1, 1], [0, 0, 0.5]]))


def test_an_integer_shift_still_takes_its_own_path():
    """nothing changes for integer shifts: S(1) from equilibrium is the 1-D shift, S([1, 0]) the planned gather"""
    sm = epg.S(1)(epg.T(90, 90)(epg.StateMatrix()))
    assert sm.coords is None and sm.nstate == 1
    sm = epg.S([1, 0])(epg.T(90, 90)(epg.StateMatrix()))
    assert sm.coords.dtype.kind == "i" and sm.t == 0 and sm.i0 == sm.nstate
