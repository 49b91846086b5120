"""Every device path of epg.X against the extended-precision recurrence (tests/exchange_recurrence.py, np.clongdouble):
the 14 xrun_kernel<NC, M, HAS_IN> instantiations and exchange_kernel<2 .. 8> of the split path, compartments on every kind
of grid axis with tables that differ per group and per voxel, voxel ranges, the pipelined host download, a state carried
in, numeric edges and the limits.  Bound: max|gpu - ref| <= 1e-13 max(1, max|ref|)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg, exchange, _lib, EpgxError
from epgpy_amd import functions as _functions
from tests.exchange_recurrence import recurrence, conserving_khi

pytestmark = pytest.mark.gpu

REL = 1e-13
MEASURED = {}          # group (a) .. (g) -> largest max|gpu - ref| / max(1, max|ref|) seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmax|gpu - extended reference| / max(1, max|ref|) per group:",
          {k: float(f"{v:.3g}") for k, v in sorted(MEASURED.items())})


def check(group, got, want, rel=REL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.max(np.abs(got.astype(np.clongdouble) - want))) / max(1.0, float(np.max(np.abs(want))))
    MEASURED[group] = max(MEASURED.get(group, 0.0), err)
    assert err <= rel, (group, err)


def ctx():
    return _lib.get_context(0)


# ------------------------------------------------------------------------------------------------ cases
def comp_shape(grid, ax):
    """[1, .., N, .., 1]: a parameter that varies along the compartment axis only"""
    return tuple(n if i == ax else 1 for i, n in enumerate(grid))


def group_shape(grid, ax):
    """the grid with 1 on the compartment axis: one value per group"""
    return tuple(1 if i == ax else n for i, n in enumerate(grid))


def make_case(seed, grid, ax, K, kmax, nsteps=28, init=False):
    """(sequence, densities [*grid], options) mixing every operator xrun_kernel walks; shifts reach past kmax so that
    truncation acts; X tables differ per group (tau, g), T / E / PD tables per voxel.  `init`: densities per voxel for a
    start state (the equilibrium of a run from nothing has density 1)"""
    rng = np.random.default_rng(seed)
    n = grid[ax]
    dens = rng.uniform(0.3, 1.0, grid) if init else np.ones(grid)
    khi = conserving_khi(rng, rng.uniform(0.3, 1.0, n), rng.uniform(5e-3, 5e-2)).reshape((1,) * ax + (n, n))
    x = epg.X(rng.uniform(1, 8, group_shape(grid, ax)), khi, axis=ax, T1=rng.uniform(300, 1500, comp_shape(grid, ax)),
              T2=rng.uniform(10, 150, comp_shape(grid, ax)), g=rng.uniform(-0.05, 0.05, grid))
    big = max(3, min(K - 1, int(kmax * 0.6)))
    seq = [epg.T(rng.uniform(30, 120, grid), 90), x]
    kinds = ["T", "E", "S", "S", "X", "X", "ADC", "Z0", "SPOIL", "RESET", "PD", "PDX", "EG"]
    for i in range(nsteps):
        kind = kinds[i % len(kinds)] if i < len(kinds) else str(rng.choice(kinds))
        if kind == "T":
            seq.append(epg.T(rng.uniform(5, 150, grid), rng.uniform(0, 360, grid)))
        elif kind == "E":            # real: fuse=True folds it into the T before it (an E . T . E record, T0)
            seq.append(epg.E(rng.uniform(1, 10), rng.uniform(300, 2000, grid), rng.uniform(20, 200, grid)))
        elif kind == "EG":
            seq.append(epg.E(rng.uniform(1, 10), rng.uniform(300, 2000, grid), rng.uniform(20, 200, grid),
                             g=rng.uniform(-0.03, 0.03, grid)))
        elif kind == "S":
            seq.append(epg.S(int(rng.choice([1, -1, 2, -2, big, -big]))))
        elif kind == "X":
            seq.append(x)
        elif kind == "ADC":
            seq.append(epg.ADC)
        elif kind == "Z0":
            seq.append(epg.Adc("Z0"))
        elif kind == "SPOIL":
            seq.append(epg.SPOILER)
        elif kind == "RESET":
            seq += [epg.RESET, epg.T(rng.uniform(30, 120, grid), 90)]
        elif kind == "PD":
            seq += [epg.PD(rng.uniform(0.2, 1.0, grid)), epg.T(rng.uniform(30, 120, grid), 45)]
        else:     # a density change that X and E see without a reset
            seq += [epg.PD(rng.uniform(0.2, 1.0, grid), reset=False), x, epg.Adc("Z0")]
    # two long shifts one way: 1.2 kmax, past the truncation order (or past K - 1)
    seq += [epg.S(big), x, epg.T(rng.uniform(30, 120, grid), 60), epg.S(big), x, epg.T(rng.uniform(30, 120, grid), 0),
            epg.ADC, epg.Adc("Z0")]
    return seq, dens, dict(max_nstate=kmax)


def random_half_state(seed, grid, nstate, K):
    """a valid start state (F-(k) = conj F+(-k), Z(-k) = conj Z(k)) up to order `nstate`: (half [nvox, 3, K] for
    DeviceState.upload, full [*grid, 2 nstate + 1, 3] rows k = -nstate .. nstate for the recurrence)"""
    rng = np.random.default_rng(seed)
    nvox = int(np.prod(grid))
    fp = (rng.uniform(-1, 1, (nvox, 2 * nstate + 1)) + 1j * rng.uniform(-1, 1, (nvox, 2 * nstate + 1))) * 0.3
    z = (rng.uniform(-1, 1, (nvox, nstate + 1)) + 1j * rng.uniform(-1, 1, (nvox, nstate + 1))) * 0.3
    z[:, 0] = z[:, 0].real
    full = np.zeros((nvox, 2 * nstate + 1, 3), dtype=np.complex128)
    full[:, :, 0] = fp
    full[:, :, 1] = fp[:, ::-1].conj()
    full[:, nstate:, 2] = z
    full[:, :nstate, 2] = z[:, :0:-1].conj()
    half = np.zeros((nvox, 3, K), dtype=np.complex128)
    half[:, 0, : nstate + 1] = full[:, nstate:, 0]
    half[:, 1, : nstate + 1] = full[:, nstate:, 1]
    half[:, 2, : nstate + 1] = full[:, nstate:, 2]
    return half, full.reshape(tuple(grid) + full.shape[1:])


def launch(seq, grid, K, options, *, fuse=True, start=None, ranges=None):
    """one plan at capacity K through _lib.run: (kernel name, records [n_adc, *grid]); `start` = (half, dens) uploaded
    into a DeviceState (HAS_IN); `ranges`: [(vox0, count)] launches of whole groups instead of one"""
    enc, _, _ = _functions.compile_sequence(seq, shape=grid, options=options, fuse=fuse)
    assert enc.grid == tuple(grid)
    c = ctx()
    plan = enc.device_plan(c, K)
    nvox = enc.nvox
    state = None
    if start is not None:
        state = _lib.DeviceState(c, nvox, K)
        state.upload(start[0], np.asarray(start[1], dtype=np.float64).reshape(-1))
    name = _lib.kernel_for(c, plan, K, state_in=state, state_out=state)
    sig = _lib.DeviceBuffer(c, 16 * enc.n_adc * nvox)
    for v0, cnt in ranges or [(0, nvox)]:
        _lib.run(c, plan, 0, plan.n_ops, v0, cnt, state, state, K, sig.ptr.value, nvox, v0)
    return name, sig.download(np.complex128, (enc.n_adc, nvox)).reshape((enc.n_adc,) + tuple(grid))


def reference(seq, grid, dens, options, init=None):
    return recurrence(_functions.flatten_sequence(seq), grid, dens, options["max_nstate"], dtype=np.clongdouble,
                      max_nstate=options["max_nstate"], init=init)


# (a) every (NC, K) xrun_kernel covers: NC * K / 64 <= 8
FUSED = [(2, 64), (2, 128), (2, 256), (3, 64), (3, 128), (4, 64), (4, 128)]
SPLIT = [(n, K) for n in range(2, 9) for K in (64, 256, 1024)]
GROUPS = 5


def instantiation_case(n, K, has_in):
    grid = (n, GROUPS)
    kmax = K - 1 if has_in else K // 2 + 5
    seq, dens, opts = make_case(100 * n + K + has_in, grid, 0, K, kmax, init=has_in)
    start = random_half_state(7 * n + K, grid, 9, K) if has_in else None
    return seq, grid, dens, opts, start


def run_instantiation(n, K, has_in, fuse):
    seq, grid, dens, opts, start = instantiation_case(n, K, has_in)
    return launch(seq, grid, K, opts, fuse=fuse, start=None if start is None else (start[0], dens))


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("has_in", [False, True])
@pytest.mark.parametrize("n, K", FUSED)
def test_xrun_instantiations(n, K, has_in, fuse):
    name, got = run_instantiation(n, K, has_in, fuse)
    assert name == f"xrun_kernel<{n}, {K // 64}, {'true' if has_in else 'false'}>"
    seq, grid, dens, opts, start = instantiation_case(n, K, has_in)
    check("a", got, reference(seq, grid, dens, opts, init=None if start is None else start[1]))


def split_case(n, K):
    grid = (n, 3)
    kmax = min(K - 1, 200) if K > 64 else K - 1
    seq, dens, opts = make_case(1000 + 10 * n + K, grid, 0, K, kmax, nsteps=20)
    return seq, grid, dens, opts


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("n, K", SPLIT)
def test_split_exchange_kernels(n, K, fuse):
    seq, grid, dens, opts = split_case(n, K)
    name, got = launch(seq, grid, K, opts, fuse=fuse)
    fused = n <= 4 and K <= 256 and n * K // 64 <= 8
    assert name == (f"xrun_kernel<{n}, {K // 64}, false>" if fused else "split<exchange_kernel>")
    check("a", got, reference(seq, grid, dens, opts))


# (b) compartments on axis 0, on the last axis, on a middle axis, on axis 2 of four; no two axes of one extent
LAYOUTS = {
    "first": ((2, 5), 0),
    "last": ((5, 3), 1),
    "middle": ((3, 4, 5), 1),
    "axis2": ((2, 5, 3, 7), 2),
}


def layout_Ks(n):
    """(fused K, split K) for n compartments"""
    return 64, (512 if n == 2 else 256)


def layout_case(layout, K):
    grid, ax = LAYOUTS[layout]
    seq, dens, opts = make_case(5000 + len(grid) * 10 + ax + K, grid, ax, K, min(K - 1, 100))
    return seq, grid, ax, dens, opts


@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(layout, path):
    grid, ax = LAYOUTS[layout]
    n = grid[ax]
    K = layout_Ks(n)[path == "split"]
    seq, grid, ax, dens, opts = layout_case(layout, K)
    name, got = launch(seq, grid, K, opts)
    assert name == (f"xrun_kernel<{n}, 1, false>" if path == "fused" else "split<exchange_kernel>")
    check("b", got, reference(seq, grid, dens, opts))


# (c) voxel ranges of whole groups, vox0 != 0
@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("layout", ["last", "middle", "axis2"])
def test_voxel_ranges(layout, path):
    grid, ax = LAYOUTS[layout]
    n = grid[ax]
    span = n * int(np.prod(grid[ax + 1:]))
    nvox = int(np.prod(grid))
    assert span < nvox
    K = layout_Ks(n)[path == "split"]
    seq, grid, ax, dens, opts = layout_case(layout, K)
    _, whole = launch(seq, grid, K, opts)
    # uneven ranges of whole groups: 1, 2, 1, 2 .. blocks of `span` voxels
    bounds, v0, step = [], 0, 1
    while v0 < nvox:
        cnt = min(step * span, nvox - v0)
        bounds.append((v0, cnt))
        v0, step = v0 + cnt, 3 - step
    assert len(bounds) >= 2 and any(b[0] for b in bounds)
    name, parts = launch(seq, grid, K, opts, ranges=bounds)
    assert np.array_equal(parts, whole)
    check("c", parts, reference(seq, grid, dens, opts))
    # ranges that cut a group are refused, on either path
    for v0, cnt in [(1, span), (span, span - 1), (span // n, span)]:
        with pytest.raises(EpgxError):
            launch(seq, grid, K, opts, ranges=[(v0, cnt)])


# (d) fused against split (EPGX_XRUN=0 is read once per process: a child process of its own)
_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_exchange_paths as t
out = {{}}
for n, K in t.FUSED:
    for has_in in (False, True):
        name, out[f"a_{{n}}_{{K}}_{{int(has_in)}}"] = t.run_instantiation(n, K, has_in, True)
        assert name == "split<exchange_kernel>", name
for layout in t.LAYOUTS:
    grid, ax = t.LAYOUTS[layout]
    K = t.layout_Ks(grid[ax])[0]
    seq, grid, ax, dens, opts = t.layout_case(layout, K)
    name, out["b_" + layout] = t.launch(seq, grid, K, opts)
    assert name == "split<exchange_kernel>", name
np.savez({path!r}, **out)
"""


def test_fused_against_split(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "split.npz")
    env = dict(os.environ, EPGX_XRUN="0")
    proc = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, path=path)], env=env, cwd=root,
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    split = np.load(path)
    worst = 0.0
    for n, K in FUSED:
        for has_in in (False, True):
            name, fused = run_instantiation(n, K, has_in, True)
            assert name.startswith("xrun_kernel<")
            worst = max(worst, float(np.max(np.abs(fused - split[f"a_{n}_{K}_{int(has_in)}"]))))
    for layout in LAYOUTS:
        grid, ax = LAYOUTS[layout]
        K = layout_Ks(grid[ax])[0]
        seq, grid, ax, dens, opts = layout_case(layout, K)
        name, fused = launch(seq, grid, K, opts)
        assert name.startswith("xrun_kernel<")
        worst = max(worst, float(np.max(np.abs(fused - split["b_" + layout]))))
    MEASURED["d (fused - split)"] = worst
    assert worst <= REL


# (e) pipelined download: several slabs of whole 3-voxel groups
PIPE_ROWS = 87382      # 3 x 87382 voxels x 8 records x 16 B = 33.6 MB: four slabs of 65538 voxels (65536 rounded up to 3)


def test_pipelined_download():
    rng = np.random.default_rng(11)
    grid = (PIPE_ROWS, 3)
    fa = rng.uniform(5, 60, grid)
    t2 = rng.uniform(10, 120, grid)
    x = epg.X(np.linspace(3, 6, PIPE_ROWS)[:, None], exchange.exchange_matrix(0.02, ncomp=3)[None], axis=1,
              T1=[[900, 1200, 400]], T2=t2)
    seq = [[epg.T(fa, 40.0 * i * (i + 1) / 2), epg.ADC, x, epg.S(1)] for i in range(8)]
    nvox = 3 * PIPE_ROWS
    assert 16 * 8 * nvox >= _functions.PIPELINE_MIN_BYTES
    got = epg.simulate(seq, mode="resident")
    assert got.shape == (8,) + grid
    # one launch of the same plan
    enc, _, _ = _functions.compile_sequence(seq)
    K = enc.capacity()
    c = ctx()
    plan = enc.device_plan(c, K)
    assert _lib.kernel_for(c, plan, K) == "xrun_kernel<3, 1, false>"
    sig = _lib.DeviceBuffer(c, 16 * enc.n_adc * nvox)
    _lib.run(c, plan, 0, plan.n_ops, 0, nvox, None, None, K, sig.ptr.value, nvox, 0)
    assert np.array_equal(got, sig.download(np.complex128, (enc.n_adc, nvox)).reshape(got.shape))
    # the reference on the groups at both sides of every slab seam (the library's default slab: 65536 rounded up to 3)
    slab = 65538
    rows = sorted({r for j in range(slab, nvox, slab) for r in (j // 3 - 1, j // 3, j // 3 + 1)} | {0, PIPE_ROWS - 1})
    assert all(j % 3 == 0 for j in range(slab, nvox, slab))
    rows = np.array(rows)
    xs = epg.X(np.linspace(3, 6, PIPE_ROWS)[rows][:, None], exchange.exchange_matrix(0.02, ncomp=3)[None], axis=1,
               T1=[[900, 1200, 400]], T2=t2[rows])
    seq_s = [[epg.T(fa[rows], 40.0 * i * (i + 1) / 2), epg.ADC, xs, epg.S(1)] for i in range(8)]
    want = recurrence(_functions.flatten_sequence(seq_s), (len(rows), 3), 1.0, 9, dtype=np.clongdouble)
    check("e", got[:, rows], want)
    got64 = epg.simulate(seq, mode="resident", dtype=np.complex64)
    assert got64.dtype == np.complex64
    assert np.array_equal(got64, got.astype(np.complex64))


# (f) a state carried in
@pytest.mark.parametrize("mode", ["resident", "stream", "stepwise"])
def test_state_carried_in(mode):
    rng = np.random.default_rng(21)
    grid = (4, 3)                         # compartments on the last axis, densities per voxel
    dens = rng.uniform(0.2, 1.0, grid)
    khi = np.stack([conserving_khi(rng, d, 0.02) for d in dens])          # [4, 3, 3]: conserves each group's densities
    x = epg.X(4.0, khi, axis=1, T1=[[900, 1200, 400]], T2=[[80, 40, 15]], g=rng.uniform(-0.03, 0.03, grid))
    prefix = [epg.T(rng.uniform(30, 90, grid), 90), epg.S(1), x, epg.T(rng.uniform(30, 150, grid), 20), epg.S(2), x,
              epg.E(3.0, rng.uniform(300, 1500, grid), rng.uniform(20, 100, grid)), epg.S(-1)]
    sm = epg.StateMatrix(density=dens)
    for op in prefix:
        sm = op(sm)
    rest = [[epg.T(rng.uniform(10, 60, grid), 30.0 * i), epg.ADC, x, epg.S(1), epg.Adc("Z0")] for i in range(10)]
    got = epg.simulate(rest, init=sm, mode=mode)
    flat = prefix + _functions.flatten_sequence(rest)
    want = recurrence(flat, grid, dens, 20, dtype=np.clongdouble)
    check("f", got, want)


# (g) numeric edges inside simulate()
def test_khi_zero_is_plain_relaxation():
    T1, T2, g = [[900], [300]], [[80], [20]], [[0.01], [-0.02]]
    x = epg.X(5.0, 0, T1=T1, T2=T2, g=g)
    e = epg.E(5.0, T1, T2, g=g)
    fa = [[20, 35, 50]]
    mk = lambda op: [[epg.T(fa, 17.0 * i), epg.ADC, op, epg.S(1)] for i in range(30)]
    dens = [0.7, 0.3]
    gx = epg.simulate(mk(x), init=epg.StateMatrix(density=dens))
    ge = epg.simulate(mk(e), init=epg.StateMatrix(density=dens))
    assert float(np.max(np.abs(gx - ge))) <= 1e-14
    check("g", gx, recurrence(_functions.flatten_sequence(mk(x)), (2, 3), dens, 31, dtype=np.clongdouble))


@pytest.mark.parametrize("edge", ["fast", "t2tiny", "unequal"])
def test_numeric_edges(edge):
    dens = [0.8, 0.2] if edge == "unequal" else [0.5, 0.5]
    x = {"fast": lambda: epg.X(10, 1e10, T2=[30, 40]),
         "t2tiny": lambda: epg.X(10, 0.05, T1=[1000, 500], T2=[np.inf, 1e-8]),
         "unequal": lambda: epg.X(5, exchange.exchange_matrix(0.05, densities=dens), T1=[900, 300], T2=[80, 20],
                                  g=[0, 0.02])}[edge]()
    fa = [[15, 40, 70, 110]]
    seq = [[epg.T(fa, 23.0 * i * i), epg.ADC, x, epg.S(1), epg.Adc("Z0"), epg.S(-2)] for i in range(24)]
    flat = _functions.flatten_sequence(seq)
    want = recurrence(flat, (2, 4), dens, 80, dtype=np.clongdouble)
    for mode in ("resident", "stream"):
        got = epg.simulate(seq, init=epg.StateMatrix(density=dens), mode=mode)
        check("g", got, want)


# (h) limits
def test_nine_compartments_refused():
    x9 = epg.X(5, exchange.exchange_matrix(0.01, ncomp=9))
    with pytest.raises(EpgxError, match="2 .. 8 compartments"):
        epg.simulate([epg.T(90, 90), x9, epg.ADC])
    enc, _, _ = _functions.compile_sequence([epg.T(90, 90), x9, epg.ADC])
    with pytest.raises(EpgxError, match="2 .. 8 compartments"):
        enc.device_plan(ctx(), 64)


def test_more_than_1024_orders_refused():
    x = epg.X(5, 0.01)
    seq = [epg.T(90, 90)] + [[x, epg.S(40)] for _ in range(30)] + [epg.ADC]
    with pytest.raises(NotImplementedError):
        epg.simulate(seq)
    with pytest.raises(NotImplementedError):
        epg.simulate(seq, mode="resident")
