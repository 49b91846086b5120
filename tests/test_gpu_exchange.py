"""Multi-compartment exchange (epg.X) on the device: G17 scenarios from the reference (op(sm), simulate in the three
modes), the kernel the library picks, voxel ranges, random sequences against a NumPy EPG-X recurrence, one large grid."""
import os

import numpy as np
import pytest

from epgpy_amd import epg, exchange, magnettransfer, _lib, EpgxError
from epgpy_amd import functions as _functions
from tests.exchange_recurrence import recurrence, random_case

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "g17_exchange.npz"))
ATOL = 1e-12


def maxerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ------------------------------------------------------------------------------------------------ op(sm): G17 scenarios
@pytest.mark.parametrize("name, make", [
    ("noexchange", lambda: epg.X(10, 0)),
    ("same", lambda: epg.X(10, 0.1)),
    ("mixed", lambda: epg.X(10, 1)),
    ("relax", lambda: epg.X(10, 0, T2=[np.inf, 1e-8])),
    ("fastrelax", lambda: epg.X(10, 10, T2=[np.inf, 1e-8])),
    ("mean", lambda: epg.X(10, 1e10, T2=[30, 40])),
    ("recovery", lambda: epg.X(10, 0, T1=1e-10, T2=1e-10)),
    ("densities", lambda: epg.X(10, [[3e10, -1e10], [-3e10, 1e10]])),
    ("unequal", lambda: epg.X(5, exchange.exchange_matrix(0.05, densities=[0.8, 0.2]), T1=[900, 300], T2=[80, 20],
                              g=[0, 0.02])),
    ("axis1", lambda: epg.X(5, GOLDEN["khi_ax1"], axis=1, T1=[[900, 400]], T2=[[70, 25]])),
    ("taus", lambda: epg.X(GOLDEN["tab_arr_in"], 0.01, T1=[1000, 500], T2=[100, 20], g=[[0.0], [0.05]])),
])
def test_op_scenarios(name, make):
    states, dens, want = GOLDEN[f"op_{name}_in"], GOLDEN[f"op_{name}_dens"], GOLDEN[f"op_{name}_out"]
    sm = epg.StateMatrix(states, density=dens)
    got = make()(sm)
    assert got.shape == want.shape[:-2]
    assert maxerr(got.states, want) <= ATOL * max(1.0, float(np.max(np.abs(want))))
    assert np.array_equal(sm.states, states)          # not in place


def test_op_conservation_error():
    sm = epg.StateMatrix([1, 1, 0], density=GOLDEN["op_bad_dens"])
    with pytest.raises(RuntimeError, match="conserve"):
        epg.X(5, GOLDEN["op_bad_khi"])(sm)


def test_op_broadcast_from_one_compartment():
    sm = epg.StateMatrix([1, 1, 0])
    assert sm.shape == (1,)
    out = epg.X(10, 1, T2=[30, 40])(sm)
    assert out.shape == (2,)
    assert maxerr(epg.X(10, 1e10, T2=[30, 40])(sm).states, GOLDEN["op_mean_out"]) <= ATOL


# ------------------------------------------------------------------------------------------------ simulate: G17 signals
def _sim_cases():
    FA, TR, NRF, b1, G, trf, W = GOLDEN["sim_params"]
    NRF = int(NRF)
    PH = GOLDEN["sim_ph"]
    k_bm, k_mt = GOLDEN["sim_k_bm"], GOLDEN["sim_k_mt"]
    f_bm, f_mt = [0.8, 0.2], [1 - 0.117, 0.117]
    exg = epg.X(TR, k_bm, T1=[1000, 500], T2=[100, 20])
    mt = epg.X(TR, k_mt, T1=[779, 779], T2=[45, 12e-3])
    sat = epg.R(rL=[0, trf * W])
    adc_sum = epg.Adc(reduce=0)
    rfs = [epg.T(FA, [i * (i + 1) / 2 * PH]) for i in range(NRF)]
    shift = epg.S(1)
    offres = 1 / TR * np.linspace(-0.5, 0.5, 101)
    exg_g = epg.X(TR, k_bm, T1=[1000, 500], T2=[100, 20], g=[offres])
    rf1, rf2 = epg.T(FA, 0), epg.T(FA, 180)
    x3 = epg.X(5.0, GOLDEN["kmat3"], T1=[800, 1000, 300], T2=[60, 80, 15], g=[0, 0.01, -0.02])
    x_a1 = epg.X(TR, GOLDEN["khi_ax1"], axis=1, T1=[[900, 400]], T2=[[70, 25]])
    return {
        "sim_spgr_bm": ([[rf, epg.ADC, exg, shift] for rf in rfs], dict(max_nstate=100), f_bm),
        "sim_spgr_bm_sum": ([[rf, adc_sum, exg, shift] for rf in rfs], dict(max_nstate=100), f_bm),
        "sim_spgr_mt_sum": ([[epg.T([FA, 0], rf.phi) @ sat, adc_sum, mt, shift] for rf in rfs], dict(max_nstate=100), f_mt),
        "sim_bssfp_bm": ([[rf1, exg_g], [rf2, exg_g]] * 250 + [[rf1, adc_sum]], {}, f_bm),
        "sim_se3": ([epg.T(90, 90)] + [[shift, x3, epg.T(150, 0), shift, x3, epg.ADC]] * 12, {}, [1.0, 1.0, 1.0]),
        "sim_axis1": ([epg.T([[20.0], [40.0], [60.0]], 90)] + [[shift, x_a1, epg.T(120, 0), shift, x_a1, epg.ADC]] * 10, {},
                      [[0.5, 0.5]] * 3),
    }


@pytest.mark.parametrize("mode", ["resident", "stream", "stepwise"])
@pytest.mark.parametrize("name", ["sim_spgr_bm", "sim_spgr_bm_sum", "sim_spgr_mt_sum", "sim_bssfp_bm", "sim_se3", "sim_axis1"])
def test_simulate_golden(name, mode):
    seq, opts, dens = _sim_cases()[name]
    got = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode=mode, **opts)
    assert maxerr(got, GOLDEN[name]) <= ATOL


# ------------------------------------------------------------------------------------------------ kernel choice
def test_kernel_for_names_fused_and_split():
    """the 2-pool SPGR at K = 128 runs on xrun_kernel<2, 2, ..>; at K = 512 (beyond the fused kernel) as pieces"""
    FA, TR = 10.0, 5.0
    exg = epg.X(TR, GOLDEN["sim_k_bm"], T1=[1000, 500], T2=[100, 20])
    seq = [[epg.T(FA, [i * 11.0]), epg.ADC, exg, epg.S(1)] for i in range(100)]
    enc, _, _ = _functions.compile_sequence(seq, shape=(2, 64))
    ctx = _lib.get_context(0)
    assert enc.capacity() == 128
    plan = enc.device_plan(ctx, 128)
    assert _lib.kernel_for(ctx, plan, 128) == "xrun_kernel<2, 2, false>"
    st = _lib.DeviceState(ctx, enc.nvox, 128)
    assert _lib.kernel_for(ctx, plan, 128, state_in=st, state_out=st) == "xrun_kernel<2, 2, true>"
    plan512 = enc.device_plan(ctx, 512)
    assert _lib.kernel_for(ctx, plan512, 512) == "split<exchange_kernel>"
    # three compartments at K = 64, four at K = 128
    enc3, _, _ = _functions.compile_sequence([epg.T(90, 90), epg.X(5, GOLDEN["kmat3"]), epg.S(1), epg.ADC])
    assert _lib.kernel_for(ctx, enc3.device_plan(ctx, 64), 64) == "xrun_kernel<3, 1, false>"
    assert _lib.kernel_for(ctx, enc3.device_plan(ctx, 256), 256) == "split<exchange_kernel>"


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_exchange as t
from epgpy_amd import _lib, epg
out = {{}}
for name in ["sim_spgr_bm", "sim_spgr_mt_sum", "sim_bssfp_bm", "sim_se3", "sim_axis1"]:
    seq, opts, dens = t._sim_cases()[name]
    out[name] = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode="resident", **opts)
enc, _, _ = t._functions.compile_sequence(t._sim_cases()["sim_spgr_bm"][0], options=dict(max_nstate=100))
out["kernel"] = np.array(_lib.kernel_for(_lib.get_context(0), enc.device_plan(_lib.get_context(0), 128), 128))
np.savez({path!r}, **out)
"""


def test_fused_against_split_path(tmp_path):
    """xrun_kernel against the split path (EPGX_XRUN=0, read once per process: a child process of its own) within 1e-13;
    resident and stream launches of xrun_kernel bit-identical"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "split.npz")
    env = dict(os.environ, EPGX_XRUN="0")
    proc = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, path=path)], env=env, cwd=root,
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    split = np.load(path)
    assert str(split["kernel"]) == "split<exchange_kernel>"
    for name in ["sim_spgr_bm", "sim_spgr_mt_sum", "sim_bssfp_bm", "sim_se3", "sim_axis1"]:
        seq, opts, dens = _sim_cases()[name]
        fused = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode="resident", **opts)
        stream = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode="stream", **opts)
        assert maxerr(fused, split[name]) <= 1e-13, name
        assert np.array_equal(fused, stream), name


# ------------------------------------------------------------------------------------------------ voxel ranges
def test_voxel_ranges_whole_groups():
    rng = np.random.default_rng(5)
    M = 96
    exg = epg.X(5.0, GOLDEN["sim_k_bm"], T1=[1000, 500], T2=[100, 20], g=[rng.uniform(-0.1, 0.1, M)])
    seq = [[epg.T([rng.uniform(5, 60, M)], 90), epg.ADC, exg, epg.S(1)] for _ in range(20)]
    enc, _, _ = _functions.compile_sequence(seq)
    assert enc.grid == (2, M)
    ctx = _lib.get_context(0)
    K = 64
    plan = enc.device_plan(ctx, K)
    nvox = enc.nvox

    def run(vox0, count):
        sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
        _lib.run(ctx, plan, 0, plan.n_ops, vox0, count, None, None, K, sig.ptr.value, nvox, vox0)
        return sig.download(np.complex128, (enc.n_adc, nvox))

    # axis 0 holds the compartments: a group spans the whole grid (2 * 96 voxels), no shorter range is whole groups
    with pytest.raises(EpgxError):
        run(0, M)
    # compartments on the LAST axis: groups are pairs of voxels
    khi = exchange.exchange_matrix(np.full(M, 0.01), axis=1)
    x1 = epg.X(5.0, khi, axis=1, T1=[[1000, 500]], T2=[[100, 20]])
    seq1 = [[epg.T([[a] for a in rng.uniform(5, 60, M)], 90), epg.ADC, x1, epg.S(1)] for _ in range(20)]
    enc1, _, _ = _functions.compile_sequence(seq1)
    assert enc1.grid == (M, 2)
    plan1 = enc1.device_plan(ctx, K)
    sig = _lib.DeviceBuffer(ctx, 16 * enc1.n_adc * enc1.nvox)
    _lib.run(ctx, plan1, 0, plan1.n_ops, 0, enc1.nvox, None, None, K, sig.ptr.value, enc1.nvox, 0)
    ref = sig.download(np.complex128, (enc1.n_adc, enc1.nvox))
    parts = _lib.DeviceBuffer(ctx, 16 * enc1.n_adc * enc1.nvox)
    for v0 in range(0, enc1.nvox, 64):
        _lib.run(ctx, plan1, 0, plan1.n_ops, v0, 64, None, None, K, parts.ptr.value, enc1.nvox, v0)
    assert np.array_equal(parts.download(np.complex128, (enc1.n_adc, enc1.nvox)), ref)
    with pytest.raises(EpgxError):
        _lib.run(ctx, plan1, 0, plan1.n_ops, 1, 64, None, None, K, parts.ptr.value, enc1.nvox, 1)
    with pytest.raises(EpgxError):
        _lib.run(ctx, plan1, 0, plan1.n_ops, 0, 63, None, None, K, parts.ptr.value, enc1.nvox, 0)


# ------------------------------------------------------------------------------------------------ random sequences
@pytest.mark.parametrize("seed", range(24))
def test_random_sequences(seed):
    seq, grid, dens, nmax = random_case(seed)
    want = recurrence(seq, grid, dens, nmax)
    for mode in ("resident", "stream"):
        got = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode=mode)
        assert maxerr(got, want) <= ATOL, (mode, seed)


# ------------------------------------------------------------------------------------------------ one large grid
def test_large_grid_spgr():
    rng = np.random.default_rng(7)
    M = 262144
    dens = [0.8, 0.2]
    khi = GOLDEN["sim_k_bm"]
    T2b = rng.uniform(10, 30, M)
    x = epg.X(5.0, khi, T1=[[1000] * 1, [500]], T2=[np.full(M, 100.0), T2b])
    fa = rng.uniform(5, 30, M)
    seq = [[epg.T([fa], 50.0 * i * (i + 1) / 2), epg.ADC, x, epg.S(1)] for i in range(40)]
    got = epg.simulate(seq, init=epg.StateMatrix(density=dens), max_nstate=60)
    assert got.shape == (40, 2, M)
    idx = rng.choice(M, 4096, replace=False)
    xs = epg.X(5.0, khi, T1=[[1000], [500]], T2=[np.full(4096, 100.0), T2b[idx]])
    seq_s = [[epg.T([fa[idx]], 50.0 * i * (i + 1) / 2), epg.ADC, xs, epg.S(1)] for i in range(40)]
    want = recurrence([op for step in seq_s for op in step], (2, 4096), dens, 41)
    assert maxerr(got[:, :, idx], want) <= ATOL
