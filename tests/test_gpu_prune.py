"""The per-voxel float shift ('shift-prune', csrc/epgx_prune.hip) on the device, against the host oracle
(tests/prune_oracle.py) at every edge of the launch geometry.  States are compared bit for bit on the stored (non-negative) half -- the other half is its mirror
image by construction --, coordinates within 4 (m + 4) 2^-53 max|k_source| for a cell of m sources: the only freedom is the
association order of the weighted mean."""
import numpy as np
import pytest

from epgpy_amd import epg, _lib
from tests import prune_oracle

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
K = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.uint64)


def make_voxels(nvox, n_in, kdim, seed, lattice=False, empty_from=None):
    """half states [nvox, 3, 64], coordinates [nvox, kdim, 64], live counts, shifts [nvox, kdim]: symmetric voxels whose
    quantised candidates stay 0.02 of a cell away from every boundary (grid 1)"""
    rng = np.random.default_rng(seed)
    half = np.zeros((nvox, 3, K), dtype=np.complex128)
    half[:, :, :n_in] = rng.normal(size=(nvox, 3, n_in)) + 1j * rng.normal(size=(nvox, 3, n_in))
    half[:, 2, 0] = half[:, 2, 0].real
    half[:, 1, 0] = half[:, 0, 0].conj()
    if empty_from is not None:
        half[:, :2, empty_from:] = 0
    k = np.zeros((nvox, kdim, K))
    k[:, 0, :n_in] = np.arange(n_in)
    if not lattice:
        k[:, :, 1:n_in] += rng.uniform(-0.2, 0.2, size=(nvox, kdim, n_in - 1))
        if kdim == 4:
            k[:, 3, 1:n_in] += rng.integers(-2, 3, size=(nvox, n_in - 1))
    shifts = rng.integers(-2, 3, size=(nvox, kdim)) + rng.uniform(0.05, 0.25, size=(nvox, kdim))
    if nvox > 1:
        shifts[1] = 0.0       # a voxel that does not move next to others that do
    return half, k, np.full(nvox, n_in, np.int32), shifts


def full_voxel(half_v, k_v, n):
    """[2n-1, 3] states and [2n-1, kdim] coordinates of one voxel with n live stored rows"""
    pos = half_v[:, :n].T
    st = np.concatenate([pos[:0:-1][:, [1, 0, 2]].conj(), pos])
    kp = k_v[:, :n].T
    return st, np.concatenate([0.0 - kp[:0:-1], kp])


def run_device(half, k, nlive, table, shape, sstride, nmax=None, prune=True, tol=1e-8):
    ctx = _lib.get_context()
    nvox, kdim = half.shape[0], k.shape[1]
    src, dst = _lib.DeviceState(ctx, nvox, K), _lib.DeviceState(ctx, nvox, K)
    src.upload(half, np.ones(nvox))
    csrc, cdst = _lib.DeviceCoords(ctx, nvox, kdim), _lib.DeviceCoords(ctx, nvox, kdim)
    csrc.upload(k, nlive)
    live = _lib.state_prune_shift(ctx, dst, cdst, src, csrc, table, shape, sstride, np.ones(kdim), np.ones(kdim), nmax, prune, tol)
    got, _ = dst.download()
    kk, nl = cdst.download()
    return got, kk, nl, live, src


def check_against_oracle(half, k, nlive, shifts, got, kk, nl, live, nmax=None, prune=True, tol=1e-8):
    worst = 0.0
    for v in range(half.shape[0]):
        st, co = full_voxel(half[v], k[v], nlive[v])
        details = {}
        rows = prune_oracle.shift_voxel(st, co, shifts[v], 1.0, nmax, prune, tol, details)
        assert min(details["margin"]) > 1e-3
        cells = [c for c in sorted(rows) if c >= (0,) * k.shape[1]]
        assert nl[v] == len(cells), (v, nl[v], len(cells))
        want = np.array([rows[c][:3] for c in cells]).T
        assert np.array_equal(bits(got[v, :, :len(cells)]), bits(want)), f"voxel {v}: states differ"
        assert not np.any(got[v, :, len(cells):]) and not np.any(kk[v, :, len(cells):])
        kmax = np.abs(co).max() + np.abs(shifts[v]).max()
        for j, c in enumerate(cells):
            err = np.abs(kk[v, :, j] - rows[c][3]).max()
            bound = 4 * (details["sources"][c] + 4) * EPS * kmax
            worst = max(worst, err / bound) if bound > 0 else worst
            assert err <= bound, (v, c, err, bound)
    assert live == nl.max()
    print("coords: worst error / bound", worst)


@pytest.mark.parametrize("nvox,kdim", ((1, 1), (3, 3), (67, 4), (257, 1)))
def test_voxel_counts_against_the_oracle(nvox, kdim):
    half, k, nlive, shifts = make_voxels(nvox, 5, kdim, seed=nvox)
    got, kk, nl, live, _ = run_device(half, k, nlive, shifts, [nvox], [1])
    check_against_oracle(half, k, nlive, shifts, got, kk, nl, live)


@pytest.mark.parametrize("n_in", (1, 15, 16, 17, 22))
def test_stored_orders_against_the_oracle(n_in):
    # (two columns while 3 n_in - 1 candidate cells fit into 64 rows; one column, where most candidates share cells, above)
    half, k, nlive, shifts = make_voxels(3, n_in, 2 if 3 * n_in - 1 <= 64 else 1, seed=n_in)
    got, kk, nl, live, _ = run_device(half, k, nlive, shifts, [3], [1])
    check_against_oracle(half, k, nlive, shifts, got, kk, nl, live)


def test_64_stored_orders_in_and_out():
    """an integer lattice and a shift that stays inside the cells: every destination has three sources, 64 rows stay 64"""
    half, k, nlive, _ = make_voxels(3, 64, 1, seed=64, lattice=True)
    shifts = np.array([[0.2], [0.0], [-0.3]])
    got, kk, nl, live, _ = run_device(half, k, nlive, shifts, [3], [1])
    check_against_oracle(half, k, nlive, shifts, got, kk, nl, live)
    assert live == 64 and np.all(nl == 64)


def test_trim_against_the_oracle():
    half, k, nlive, shifts = make_voxels(5, 22, 1, seed=7)
    got, kk, nl, live, _ = run_device(half, k, nlive, shifts, [5], [1], nmax=9)
    check_against_oracle(half, k, nlive, shifts, got, kk, nl, live, nmax=9)
    assert live == 10


def test_rows_cross_64_before_the_prune_and_fit_after_it():
    half, k, nlive, _ = make_voxels(3, 40, 1, seed=40, lattice=True, empty_from=10)
    shifts = np.full((3, 1), 30.3)
    got, kk, nl, live, _ = run_device(half, k, nlive, shifts, [3], [1])
    check_against_oracle(half, k, nlive, shifts, got, kk, nl, live)
    assert live == 40


def test_a_voxel_that_does_not_fit_raises_and_leaves_the_source():
    half, k, nlive, _ = make_voxels(3, 40, 1, seed=41, lattice=True)
    half[0, :2, 10:] = 0                       # (voxel 0 fits, the others keep 70 rows)
    shifts = np.full((3, 1), 30.3)
    ctx = _lib.get_context()
    src, dst = _lib.DeviceState(ctx, 3, K), _lib.DeviceState(ctx, 3, K)
    src.upload(half, np.ones(3))
    csrc, cdst = _lib.DeviceCoords(ctx, 3, 1), _lib.DeviceCoords(ctx, 3, 1)
    csrc.upload(k, nlive)
    with pytest.raises(NotImplementedError, match="kgrid.*max_nstate.*prune"):
        _lib.state_prune_shift(ctx, dst, cdst, src, csrc, shifts, [3], [1], [1.0], [1.0], None, True, 1e-8)
    back, _ = src.download()
    kback, nback = csrc.download()
    assert np.array_equal(bits(back), bits(half)) and np.array_equal(kback, k) and np.array_equal(nback, nlive)


def test_two_launches_give_equal_bits_and_a_voxel_does_not_depend_on_its_neighbours():
    half, k, nlive, shifts = make_voxels(9, 17, 3, seed=3)
    a = run_device(half, k, nlive, shifts, [9], [1])
    b = run_device(half, k, nlive, shifts, [9], [1])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    one = run_device(half[5:6], k[5:6], nlive[5:6], shifts[5:6], [1], [1])
    assert np.array_equal(bits(one[0][0]), bits(a[0][5])) and np.array_equal(one[1][0].view(np.uint64), a[1][5].view(np.uint64))
    assert one[2][0] == a[2][5]


def test_shift_table_along_one_axis():
    """a shift that varies along the first of two grid axes: the table has one entry per point of that axis"""
    half, k, nlive, _ = make_voxels(6, 5, 1, seed=11)
    table = np.array([[1.2], [0.0], [-0.7]])
    got, kk, nl, live, _ = run_device(half, k, nlive, table, [3, 2], [1, 0])
    check_against_oracle(half, k, nlive, np.repeat(table, 2, axis=0), got, kk, nl, live)


def test_argument_checks():
    ctx = _lib.get_context()
    src, dst = _lib.DeviceState(ctx, 2, K), _lib.DeviceState(ctx, 2, K)
    c1, c2, c3 = _lib.DeviceCoords(ctx, 2, 1), _lib.DeviceCoords(ctx, 2, 1), _lib.DeviceCoords(ctx, 2, 2)
    c1.upload(np.zeros((1, 1, K)), [1])
    args = (np.ones((1, 1)), [2], [0], [1.0], [1.0], None, True, 1e-8)
    with pytest.raises(_lib.EpgxError, match="must differ"):
        _lib.state_prune_shift(ctx, src, c2, src, c1, *args)
    with pytest.raises(_lib.EpgxError, match="kdim"):
        _lib.state_prune_shift(ctx, dst, c3, src, c1, *args)
    with pytest.raises(_lib.EpgxError, match="grid of 3 voxels"):
        _lib.state_prune_shift(ctx, dst, c2, src, c1, np.ones((1, 1)), [3], [0], [1.0], [1.0], None, True, 1e-8)
    with pytest.raises(_lib.EpgxError, match="table"):
        _lib.state_prune_shift(ctx, dst, c2, src, c1, np.ones((1, 1)), [2], [1], [1.0], [1.0], None, True, 1e-8)
    with pytest.raises(_lib.EpgxError, match="positive"):
        _lib.state_prune_shift(ctx, dst, c2, src, c1, np.ones((1, 1)), [2], [0], [1.0], [0.0], None, True, 1e-8)
    with pytest.raises(NotImplementedError, match="64"):
        _lib.state_prune_shift(ctx, _lib.DeviceState(ctx, 2, 128), c2, src, c1, *args)
    with pytest.raises(_lib.EpgxError, match="kdim"):
        _lib.DeviceCoords(ctx, 2, 5)
    with pytest.raises(_lib.EpgxError, match="nlive"):
        c1.upload(np.zeros((1, 1, K)), [65])


def test_f0_readout_with_a_time_coordinate_and_round_trip():
    T2, R2 = np.array([40.0, 80.0, 120.0, 200.0]), np.array([0.02, 0.05, 0.11])
    seq = [epg.T(20, 90)] + [epg.C(2.0, R2[:, None]), epg.E(2.0, 1000.0, T2[None, :]), epg.T(20, 0)] * 3
    sm = epg.StateMatrix(shape=(3, 4), kgrid=0.03, voxel_coords=True)
    for op in seq:
        sm = op(sm, inplace=True)
    assert sm.kdim == 4 and sm.coords.shape == (3, 4, 2 * sm.nstate + 1, 4)
    want = (sm.F * sm.i0 * np.exp(-np.abs(sm.t))).sum(axis=-1)
    got = sm.F0
    print("F0 err", np.abs(got - want).max())
    assert got.shape == (3, 4) and np.abs(got - want).max() <= 8 * (2 * sm.nstate + 1) * EPS * np.abs(sm.F).sum(axis=-1).max()
    assert np.abs(got).max() > 1e-2 and np.ptp(np.abs(got)) > 1e-3          # (not a broadcast result)
    assert sm.Z0.shape == sm.Z.shape
    again = epg.StateMatrix(sm.states, coords=sm.coords, kgrid=0.03, voxel_coords=True)
    assert np.array_equal(again.coords, sm.coords) and np.array_equal(bits(again.states), bits(sm.states))
    assert np.array_equal(again._kspace.live(), sm._kspace.live())
    assert sm.copy().options["voxel_coords"] is True
