"""The per-voxel float shift ('shift-prune') without a device: the oracle's own invariants, the routing of the option
`voxel_coords`, and the errors that stay as they were without it."""
import numpy as np
import pytest

from epgpy_amd import epg, kmerge
from tests import prune_oracle


def voxel(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(n, 3)) + 1j * rng.normal(size=(n, 3))
    pos[0, 2] = pos[0, 2].real
    pos[0, 1] = pos[0, 0].conj()
    k = (np.arange(n) + np.r_[0, rng.uniform(-0.2, 0.2, n - 1)]).reshape(-1, 1)
    return np.concatenate([pos[:0:-1][:, [1, 0, 2]].conj(), pos]), np.concatenate([-k[:0:-1], k])


def test_oracle_keeps_the_symmetry_and_the_centre_row():
    st, k = voxel(6, 0)
    rows = prune_oracle.shift_voxel(st, k, [1.3], 1.0)
    cells = sorted(rows)
    assert len(cells) % 2 == 1 and (0,) in rows and all(tuple(-c for c in cell) in rows for cell in cells)
    for cell in cells:
        F, col1, Z, kk = rows[cell]
        mF, mcol1, mZ, mk = rows[tuple(-c for c in cell)]
        assert col1 == np.conj(mF) and np.allclose(Z, np.conj(mZ)) and np.allclose(kk, -mk)
    # a zero shift of rows that sit alone in their cells changes nothing
    same = prune_oracle.shift_voxel(st, k, [0.0], 1.0)
    assert len(same) == len(st) and all(np.allclose(same[(i - 5,)][:3], st[i]) for i in range(len(st)))


def test_oracle_trims_and_prunes():
    st, k = voxel(8, 1)
    rows = prune_oracle.shift_voxel(st, k, [0.2], 1.0, nmax=3)
    assert len(rows) == 7
    st[:3] = st[-3:] = 0
    assert len(prune_oracle.shift_voxel(st, k, [0.2], 1.0)) == 9 and len(prune_oracle.shift_voxel(st, k, [0.2], 1.0, prune=False)) == 15
    states, coords = prune_oracle.layout([rows, {(0,): rows[(0,)]}], (2,), np.ones(1))
    assert states.shape == (2, 7, 3) and not np.any(states[1, :3]) and not np.any(coords[1])


def test_rounding_is_half_away_from_zero():
    assert np.array_equal(prune_oracle.rnd(np.array([0.5, -0.5, 1.49, -1.51, 0.0, 2.5])), [1, -1, 1, -2, 0, 3])


def test_routing_of_the_option():
    vec, one = epg.S([[1.5], [0.5]], kgrid=1.0), epg.S(1.5, kgrid=1.0)
    assert kmerge.per_voxel(vec, None) and not kmerge.per_voxel(one, None)
    assert kmerge.per_voxel(epg.C(1.0, [0.1, 0.2]), None) and kmerge.per_voxel(epg.G(1.0, [[1, 0, 0], [0, 1, 0]]), None)
    assert not kmerge.per_voxel(epg.S(np.array([[1], [2]])), None)              # an integer vector: the planned gather
    assert kmerge.per_voxel(epg.S(np.array([[1], [2]])), kmerge.FloatKSpace.equilibrium(1))
    ks = kmerge.VoxelKSpace.__new__(kmerge.VoxelKSpace)
    assert kmerge.per_voxel(one, ks) and kmerge.per_voxel(epg.S(2), ks) and kmerge.is_float(ks)
    with pytest.raises(NotImplementedError, match="per-voxel coordinates"):
        ks.points
    with pytest.raises(NotImplementedError, match="D \\(diffusion\\)"):
        ks.bmatrices(1.0)
    assert isinstance(kmerge.VoxelKSpace.equilibrium(4), kmerge.FloatKSpace) and kmerge.VoxelKSpace.equilibrium(4).kdim == 4


def test_errors_of_the_option_before_any_launch():
    seq = [epg.T(30, 90), epg.S([[1.5], [0.5]]), epg.ADC]
    for kwargs, match in ((dict(mode="resident"), "mode='resident'"), (dict(mode="stream"), "mode='stream'"),
                          (dict(out="device"), 'out="device"'), (dict(ngpu=2), "ngpu > 1")):
        with pytest.raises(NotImplementedError, match=match):
            epg.simulate(seq, kgrid=1.0, voxel_coords=True, **kwargs)
    with pytest.raises(NotImplementedError, match="D \\(diffusion\\)"):
        epg.simulate(seq[:2] + [epg.D(1.0, 1e-3), epg.ADC], kgrid=1.0, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="shift-prune"):                # a compiled plan never takes it
        epg.compile_sequence(seq, options=dict(kgrid=1.0, voxel_coords=True))


def test_pinned_errors_without_the_option():
    for op in (epg.S([[1.5, 0.2], [0.5, 0.1]], kgrid=0.1), epg.C(1.0, [0.1, 0.2], kgrid=0.1)):
        with pytest.raises(NotImplementedError, match="shift-prune.*voxel_coords"):
            epg.compile_sequence([op, epg.ADC])
    with pytest.raises(NotImplementedError, match="shift-prune.*voxel_coords"):
        kmerge.FloatKSpace(np.zeros((1, 1)), lead=(2,))
    with pytest.raises(NotImplementedError, match="shift-prune"):
        kmerge.FloatKSpace.from_coords(np.zeros((2, 1, 1)))


def test_further_errors_of_the_option_before_any_launch():
    seq = [epg.T(30, 90), epg.S([[1.5], [0.5]]), epg.ADC]
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.simulate(seq, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="kgrid per voxel"):
        epg.simulate(seq, kgrid=np.ones((2, 1)), voxel_coords=True)
    for probe, name in ((epg.DFT([[0.0, 0.0, 0.0]]), "DFT"), (epg.Imaging([[0.0, 0.0, 0.0]]), "Imaging")):
        with pytest.raises(NotImplementedError, match=name + " on per-voxel coordinates"):
            epg.simulate(seq[:2] + [probe], kgrid=1.0, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="System on per-voxel coordinates"):
        epg.simulate([epg.System(kvalue=2.0)] + seq, kgrid=1.0, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="derivative states"):
        epg.simulate(seq[:2] + [epg.Jacobian("alpha")], kgrid=1.0, voxel_coords=True)
    from epgpy_amd import distributed
    with pytest.raises(NotImplementedError, match="simulate_sharded with per-voxel float shifts"):
        distributed.simulate_sharded(seq, kgrid=1.0, voxel_coords=True)
    ks = kmerge.VoxelKSpace.__new__(kmerge.VoxelKSpace)
    ks.grid = (3, 1)
    with pytest.raises(NotImplementedError, match="widening the grid"):
        ks.with_lead((3, 4))


def test_exchange_and_the_tiled_path_with_the_option():
    seq = [epg.T(30, 90), epg.S([[[1.5]], [[0.5]]]), epg.X(5, 0.01, T1=[1000, 500], T2=[100, 20]), epg.ADC]
    with pytest.raises(NotImplementedError, match="X \\(exchange\\)"):
        epg.simulate(seq, kgrid=1.0, voxel_coords=True)
    # the tiled path is entered through mode="resident" written out only: a sequence long enough for it raises there as well
    long = [epg.T(30, 90)] + [epg.S([[1.5], [0.5]]), epg.T(10, 0)] * 1100 + [epg.ADC]
    with pytest.raises(NotImplementedError, match="mode='resident' with per-voxel float shifts"):
        epg.simulate(long, kgrid=1.0, voxel_coords=True, mode="resident")
