"""Spatial read-out, host side (no GPU): utils.imaging / utils.dft against the reference's records (G20), shapes and errors,
System / sm.system bookkeeping, the folded half-representation formula the kernel evaluates, and the per-class tables."""
import os
import types

import numpy as np
import pytest

from epgpy_amd import epg, utils, functions, statematrix, kspace, probe, operator
from tests import imaging_cases as ic


class Rec:
    """stands for an operator of a case: what it is and what it was given"""

    def __init__(self, kind, args=(), kw=None):
        self.kind, self.args, self.kw = kind, args, kw or {}


def recording_ns():
    def mk(kind):
        return lambda *args, **kw: Rec(kind, args, kw)
    return types.SimpleNamespace(T=mk("T"), E=mk("E"), S=mk("S"), ADC=Rec("ADC"), DFT=mk("DFT"), Imaging=mk("Imaging"),
                                 System=mk("System"))


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


def element_bound(F, k, weights, reduce, npshape, voxel_shape="box", voxel_size=1):
    """the bar of tests/imaging_cases.bound for a record: per element 1e-12 max(1, M), M = sum_r |w_r F_r|; times |weights|,
    summed over what `reduce` sums"""
    w = 1.0 if voxel_shape == "point" else np.sinc(k * voxel_size / 2 / np.pi).prod(-1)
    M = (np.abs(F) * np.abs(w)).sum(-1)                               # [*grid]
    bar = np.broadcast_to(ic.bound(M).reshape(M.shape + (1,) * len(npshape)), M.shape + tuple(npshape)).copy()
    if weights is not None:
        bar *= np.abs(weights)
    if reduce is True:
        return bar.sum()
    return bar if reduce is False else bar.sum(axis=reduce)


def test_dft_matches_reference_1d(golden):
    seq, kw = ic.cases(recording_ns())["dft_1d"]
    pos = seq[-1].args[0]
    F, k = golden["dft_1d_F"], golden["dft_1d_k"]
    got = utils.dft(pos, F, k)
    want = golden["dft_1d_0"][0]
    assert got.shape == want.shape == (3, 31) and got.dtype == np.complex128
    assert np.all(np.abs(got - want) <= element_bound(F, k, None, False, (31,), "point"))
    assert functions.dft is utils.dft and functions.imaging is utils.imaging and epg.imaging is utils.imaging and epg.dft is utils.dft


def test_imaging_matches_reference_classes(golden):
    seq, kw = ic.cases(recording_ns())["classes_3d"]
    F, k = golden["classes_3d_F"], golden["classes_3d_k"]
    assert F.shape == (4, 3, 13) and k.shape == (4, 1, 13, 3)
    for i, pb in enumerate(kw["probe"]):
        want = golden[f"classes_3d_{i}"][0]
        pos = np.asarray(pb.args[0])
        npshape = pos.shape[:-1] if pos.ndim > 1 else pos.shape
        if pb.kind == "DFT":
            got = utils.dft(pos, F, k)
            bar = element_bound(F, k, None, False, npshape, "point")
        else:
            got = utils.imaging(pos, F, k, **{key: (np.array(v) if key == "weights" else v) for key, v in pb.kw.items()})
            bar = element_bound(F, k, pb.kw.get("weights"), pb.kw.get("reduce", True), npshape,
                                pb.kw.get("voxel_shape", "box"), pb.kw.get("voxel_size", 1))
        assert got.shape == want.shape, (i, got.shape, want.shape)
        assert np.all(np.abs(got - want) <= bar), (i, np.abs(got - want).max())


def test_imaging_shapes_and_rules():
    rng = np.random.default_rng(3)
    F = rng.standard_normal((2, 3, 5)) + 1j * rng.standard_normal((2, 3, 5))
    k = 10.0 * np.arange(-2, 3).reshape(1, 1, 5, 1) * np.array([1.0, 0.5])
    pos1 = np.linspace(-0.1, 0.1, 7)
    # 1-D positions mean [P, 1]; the result carries the position axes behind the grid
    assert utils.imaging(pos1, F, k, reduce=False).shape == (2, 3, 7)
    assert np.array_equal(utils.imaging(pos1, F, k, reduce=False), utils.imaging(pos1[:, None], F, k, reduce=False))
    pos2 = rng.uniform(-0.1, 0.1, (4, 6, 2))
    full = utils.imaging(pos2, F, k, reduce=False)
    assert full.shape == (2, 3, 4, 6) and full.dtype == np.complex128
    # reduce: True sums everything, an int or a tuple those axes
    assert np.allclose(utils.imaging(pos2, F, k), full.sum())
    assert np.allclose(utils.imaging(pos2, F, k, reduce=1), full.sum(axis=1))
    assert np.allclose(utils.imaging(pos2, F, k, reduce=(0, 3)), full.sum(axis=(0, 3)))
    # only the first d wavenumber columns enter the phase; the box factor runs over all of them
    point1 = utils.imaging(pos1, F, k, voxel_shape="point", reduce=False)
    theta = k[..., 0][..., None, :] * pos1[:, None]
    assert np.allclose(point1, (F[..., None, :] * np.exp(1j * theta)).sum(-1))
    box = np.sinc(k * 0.05 / 2 / np.pi).prod(-1)
    assert np.allclose(utils.imaging(pos1, F, k, voxel_size=0.05, reduce=False),
                       ((box * F)[..., None, :] * np.exp(1j * theta)).sum(-1))
    # phase in degrees; weights by NumPy broadcasting
    assert np.allclose(utils.imaging(pos2, F, k, phase=90.0, reduce=False), 1j * full)
    wts = rng.standard_normal((6,))
    assert np.allclose(utils.imaging(pos2, F, k, weights=wts, reduce=False), full * wts)
    # without `expand` positions broadcast against the leading axes
    assert utils.imaging(rng.uniform(-1, 1, (3, 2)), F, k, expand=False, reduce=False).shape == (2, 3)
    with pytest.raises(ValueError, match="Unknown voxel shape"):
        utils.imaging(pos1, F, k, voxel_shape="ball")
    with pytest.raises(ValueError):
        utils.imaging(pos2, F, k, weights=np.ones((5,)), reduce=False)
    # dft: point voxels, nothing summed
    assert np.array_equal(utils.dft(pos1, F, k), point1)
    assert np.allclose(utils.dft(pos1, F, k, reduce=True), point1.sum())


def test_kmask_drops_states_below_tol_everywhere():
    """states whose voxel factor is <= tol in EVERY voxel leave the sum; one voxel above tol keeps the state for all"""
    size = 0.5
    kz = 2 * np.pi / size                       # sinc(k size / 2 pi) = sinc(1) = 0 (to rounding)
    k = np.array([[[-kz], [0.0], [kz]], [[-kz / 2], [0.0], [kz / 2]]])        # [2 voxels, 3 rows, 1]
    F = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], dtype=complex)
    pos = np.array([0.0])
    # voxel 1 keeps rows 0 and 2 above tol: they stay, and voxel 0 adds its (rounding-level) factor times F
    both = utils.imaging(pos, F, k, voxel_size=size, reduce=False)
    assert np.allclose(both[:, 0], [2.0, 2.0 + 4 * np.sinc(0.5)])
    # voxel 0 alone: rows 0 and 2 are dropped outright, even with a huge F
    alone = utils.imaging(pos, np.array([[1e30, 2.0, 1e30]], dtype=complex), k[:1], voxel_size=size, reduce=False)
    assert alone[0, 0] == 2.0
    # a larger tol drops what a smaller one keeps
    assert utils.imaging(pos, F[1:], k[1:], voxel_size=size, tol=0.9, reduce=False)[0, 0] == 2.0


def test_modulation_formula():
    """with a time coordinate: exp(-|t| Re m) exp(2 pi i t Im m) per state, states decayed below tol left out"""
    F = np.array([[1.0, 2.0, 3.0]], dtype=complex)
    k = np.array([[[-1.0], [0.0], [1.0]]])
    t = np.array([[-2.0, 0.0, 2.0]])
    pos = np.array([0.3])
    m = 0.5 + 0.25j
    want = (F * np.exp(-np.abs(t) * 0.5) * np.exp(2j * np.pi * t * 0.25) * np.exp(1j * k[..., 0] * 0.3)).sum(-1)
    assert np.allclose(utils.imaging(pos, F, k, t, modulation=m, voxel_shape="point", reduce=False)[:, 0], want)
    assert np.allclose(utils.imaging(pos, F, k, t, modulation=100.0, voxel_shape="point", reduce=False)[:, 0], 2.0)
    # no time coordinate: modulation has no effect
    assert np.array_equal(utils.imaging(pos, F, k, modulation=m, voxel_shape="point", reduce=False),
                          utils.imaging(pos, F, k, voxel_shape="point", reduce=False))


def test_system_bookkeeping():
    arrays = statematrix.SystemArrays()
    assert arrays.get("weights") is None and arrays.get("weights", 3) == 3 and "weights" not in arrays and len(arrays) == 0
    with pytest.raises(KeyError):
        arrays["coords"]
    given = [1.0, 2.0]
    arrays.set("weights", given)
    assert np.array_equal(arrays["weights"], [1.0, 2.0]) and np.array_equal(arrays.get("weights", broadcast=False), [1.0, 2.0])
    twin = arrays.copy()
    twin.set("weights", [5.0])
    twin.set("coords", [[0.0]])
    assert np.array_equal(arrays["weights"], [1.0, 2.0]) and "coords" not in arrays and list(twin) == ["weights", "coords"]

    op = epg.System(kvalue=[2.0, 3.0], tvalue=4.0, weights=[[1, 2, 3]], coords=np.zeros((5, 2)))
    assert op.shape == (1,) and op.nshift == 0 and op.duration == 0 and op.name == "System"
    assert op._on_host() and not op.PASSIVE and op._parts() == [op]
    sm = types.SimpleNamespace(kvalue=1.0, tvalue=1.0, system=statematrix.SystemArrays())
    assert op._apply(sm) is sm
    assert sm.kvalue == [2.0, 3.0] and sm.tvalue == 4.0
    assert sm.system["weights"].shape == (1, 3) and sm.system["coords"].shape == (5, 2) and "kvalue" not in sm.system
    assert isinstance(epg.System(name="scanner"), operator.Operator) and epg.System(name="scanner").name == "scanner"


def test_probe_objects():
    dft, img = epg.DFT([0.0, 0.1]), epg.Imaging(np.zeros((4, 2)), voxel_size=0.1, reduce=(0,), name="im")
    for pb in (dft, img, epg.DFT(), epg.Imaging()):
        assert isinstance(pb, epg.Probe) and pb._device_kind() is None and pb.PASSIVE and pb._parts() == []
    assert dft.coords.shape == (2,) and img.coords.shape == (4, 2) and img.opts == {"voxel_size": 0.1, "reduce": (0,)}
    assert repr(dft) == "DFT" and repr(img) == "im" and epg.DFT().coords is None
    assert "EVERY acquisition" in epg.Imaging.__doc__


@pytest.mark.parametrize("nrow,npos,d,box,nvox", [c for c in ic.RANDOM if c[0] <= 200])
def test_folded_formula(nrow, npos, d, box, nvox):
    """the sum over the STORED orders the kernel evaluates, restated in NumPy on fold()ed states, against utils.imaging on
    the full rows"""
    half, K, k, w, pos = ic.random_problem(1000 * nrow + npos, nvox, nrow, npos, d, box)
    full = statematrix.unfold(half, (nvox,), nrow - 1)[..., 0]                          # F, rows -n .. n
    assert np.array_equal(statematrix.fold(statematrix.unfold(half, (nvox,), nrow - 1), K)[:, :2], half[:, :2])
    kfull, wfull = np.concatenate([-k[:0:-1], k]), np.concatenate([w[:0:-1], w])
    want = utils.imaging(pos, full * wfull, kfull[None], voxel_shape="point", reduce=False)

    a, b = half[:, 0, :nrow], half[:, 1, :nrow].copy()
    b[:, 0] = 0
    P, Q, R, S = w * (a.real + b.real), w * (a.imag + b.imag), w * (a.real - b.real), w * (a.imag - b.imag)
    theta = k @ pos.T
    c, s = np.cos(theta), np.sin(theta)
    got = (P @ c - Q @ s) + 1j * (R @ s + S @ c)
    assert got.shape == want.shape == (nvox, npos)
    M = ic.magnitude(full, wfull)
    assert np.all(np.abs(got - want) <= ic.bound(M)[:, None])
    # and the extended-precision restatement the device tests use
    ref = ic.longdouble_image(*ic.fold_terms(half, k, w), pos)
    assert np.all(np.abs(ref - want) <= ic.bound(M)[:, None])


def planned_kspace():
    """the planner's coordinates after four vectorised 3-D shifts (one direction per voxel class)"""
    ks = kspace.KSpace.equilibrium(3)
    for _ in range(4):
        ks, _tab = ks.after_mixing().shifted(ic.K3)
    return ks


def test_readout_tables_per_class():
    ks = planned_kspace()
    assert ks.lead == (4,) and ks.kdim == 3
    kvalue = [60.0, 50.0, 40.0]
    coords = ks.coords * np.asarray(kvalue)                                  # [4, R, 3], as StateMatrix.k
    for ncol in (1, 2, 3):
        k, w, lead = probe.readout_tables(ks, ks.nstate, kvalue, ncol, "box", [0.02, 0.03, 0.05])
        assert lead == (4,) and k.shape == (4, ks.nstate + 1, ncol) and w.shape == (4, ks.nstate + 1)
        assert np.array_equal(k, coords[:, ks.centre:, :ncol])
        assert np.allclose(w, np.sinc(coords[:, ks.centre:] * [0.02, 0.03, 0.05] / 2 / np.pi).prod(-1), rtol=0, atol=1e-16)
    k, w, _ = probe.readout_tables(ks, ks.nstate, kvalue, 2, "point")
    assert np.array_equal(w, np.ones((4, ks.nstate + 1)))
    # the drop rule: kept if the factor exceeds tol in ANY class -- the same states utils.imaging keeps
    size = [2 * np.pi / 120.0, 2 * np.pi / 100.0, 0]       # the factor vanishes where a coordinate is even and not zero: orders 2 and 4, in every class
    k, w, _ = probe.readout_tables(ks, ks.nstate, kvalue, 3, "box", size, tol=1e-8)
    factor = np.sinc(coords[:, ks.centre:] * size / 2 / np.pi).prod(-1)
    kept = np.any(np.abs(factor) > 1e-8, axis=0)
    assert kept.tolist() == [True, True, False, True, False]
    assert np.array_equal(w != 0, np.broadcast_to(kept, w.shape) & (factor != 0)) and np.array_equal(w[:, kept], factor[:, kept])
    rng = np.random.default_rng(0)
    F = rng.standard_normal((4, 3, ks.nrow)) + 1j * rng.standard_normal((4, 3, ks.nrow))
    pos = rng.uniform(-0.3, 0.3, (5, 3))
    want = utils.imaging(pos, F, coords[:, None], voxel_size=size, reduce=False)
    wfull = np.concatenate([w[:, :0:-1], w], axis=1)[:, None, :]
    got = utils.imaging(pos, F * wfull, coords[:, None], voxel_shape="point", reduce=False)
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    # 1-D orders without a planner: k_j = j kvalue
    k, w, lead = probe.readout_tables(None, 5, 300.0, 1, "point")
    assert lead == () and np.array_equal(k[0, :, 0], 300.0 * np.arange(6)) and w.shape == (1, 6)
    with pytest.raises(ValueError):
        probe.readout_tables(None, 5, 300.0, 2, "point")
    with pytest.raises(ValueError, match="Unknown voxel shape"):
        probe.readout_tables(None, 5, 300.0, 1, "ball")


def test_class_ranges():
    assert probe.class_ranges((4, 3), (4,)) == [(0, 3, 0), (3, 6, 1), (6, 9, 2), (9, 12, 3)]
    assert probe.class_ranges((4, 3), ()) == [(0, 12, 0)]
    assert probe.class_ranges((2, 2, 5), (2, 2)) == [(0, 5, 0), (5, 10, 1), (10, 15, 2), (15, 20, 3)]
    assert probe.class_ranges((2, 3, 2), (1, 3)) == [(0, 2, 0), (2, 4, 1), (4, 6, 2), (6, 8, 0), (8, 10, 1), (10, 12, 2)]
    assert probe.class_ranges((3, 2), (1,)) == [(0, 6, 0)]


def test_image_reduction_plan():
    shape = (4, 3, 5, 4)
    assert probe._image_reduction(False, None, shape) is None
    assert probe._image_reduction(True, None, shape) == ([1, 1, 1, 1], None)
    assert probe._image_reduction(None, None, shape)[0] == [1, 1, 1, 1]
    assert probe._image_reduction((0,), None, shape)[0] == [1, 0, 0, 0]
    assert probe._image_reduction(-1, None, shape)[0] == [0, 0, 0, 1]
    assert probe._image_reduction((2, 3), np.ones((5, 4)), shape)[1].shape == (1, 1, 5, 4)
    assert probe._image_reduction((0, 0), None, shape) is None and probe._image_reduction((4,), None, shape) is None
    assert probe._image_reduction((), None, shape) is None
    assert probe._image_reduction(True, None, (2,) * 9) is None
    assert probe._weights_fit(np.ones((5, 4)), shape) and probe._weights_fit(np.ones((4, 1, 1, 1)), shape)
    assert not probe._weights_fit(np.ones((4, 3)), shape) and not probe._weights_fit(np.ones((1,) * 5), shape)
    assert not probe._weights_fit(np.array(["a"]), shape)


def test_golden_file_holds_every_record_and_is_small(golden):
    """(that the generator reproduces the file bit for bit -- fixed member dates in `save_npz` -- can only be checked where the
    reference is present)"""
    assert os.path.getsize(ic.GOLDEN) < 512 * 1024
    names = [key for name, (seq, kw) in ic.cases(recording_ns()).items() for key in ic.record_names(name, kw)]
    assert set(names) | {"dft_1d_F", "dft_1d_k", "classes_3d_F", "classes_3d_k"} == set(golden.files)
    assert golden["img_2d_none_0"].shape == (64, 3, 256) and golden["img_2d_all_0"].shape == (64,)
    assert golden["classes_3d_0"].shape == (1, 4, 3, 5, 4) and golden["classes_3d_6"].shape == (1, 3, 5, 4)
    assert golden["classes_3d_7"].shape == (1, 4, 3) and golden["classes_3d_9"].shape == (1, 4, 3, 7)
