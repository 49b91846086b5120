"""CPU: the C boundary of epgx_signal_gram / epgx_signal_project, the argument checks of match.compress that need no GPU, the
host half of the compression (Gram matrix -> basis) on exact input, and the conditions on the inputs of
tests/test_gpu_compress.py: the yardstick of tests/compress_cases.py accepts plain float64 and rejects an error of 1e-12, and
at least 90 % of the voxels of the cases matched in the compressed space are decisive under the reference alone."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import match, functions, _lib, _build
from tests import match_cases as mc
from tests import compress_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_agrees():
    """include/epgx.h, _lib.py, INTEGRATION.md and the built library: both entry points, still ABI 11"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "#define EPGX_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11
    for name, nargs in (("epgx_signal_gram", 8), ("epgx_signal_project", 9)):
        proto = re.search(rf"int {name}\(([^)]*)\)", header).group(1)
        assert len(proto.split(",")) == len(_lib.SYMBOLS[name][1]) == nargs, name
    lib = _lib.load()
    assert lib.epgx_abi_version() == 11 and hasattr(lib, "epgx_signal_gram") and hasattr(lib, "epgx_signal_project")
    assert any(src == "epgx_compress.hip" for _, src, _ in _build.UNITS)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "epgx_signal_gram" in doc and "epgx_signal_project" in doc
    assert callable(_lib.signal_gram) and callable(_lib.signal_project)
    import inspect
    assert inspect.signature(_lib.signal_gram).parameters["nsplit"].default == 0
    assert callable(match.compress)


def test_raw_entries_validate_before_any_device_work():
    """NULL arguments are refused without a context: EPGX_ERR_INVALID and a message"""
    lib = _lib.load()
    assert lib.epgx_signal_gram(None, None, 0, None, 1, 1, 0, None) == -1
    assert b"epgx_signal_gram" in lib.epgx_last_error()
    assert lib.epgx_signal_project(None, None, 1, None, 0, 1, 0, None, 0) == -1
    assert b"epgx_signal_project" in lib.epgx_last_error()


def test_nsplit_rule():
    """the documented choice for nsplit = 0 is a function of (nrec, natoms): about 2048 workgroups, 1024 atoms per split at least"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    assert "min(ceil(2048 / npair), max(natoms / 1024, 1))" in header
    for (nrec, natoms), want in {(1, 1): 1, (5, 17): 1, (4, 2047): 1, (5, 2048): 2, (64, 10 ** 6): 976, (65, 10 ** 6): 683,
                                 (1000, 10 ** 6): 16, (1000, 4096): 4, (5000, 10 ** 6): 1}.items():
        assert _lib.gram_nsplit(nrec, natoms) == want, (nrec, natoms)
        assert 1 <= _lib.gram_nsplit(nrec, natoms) <= natoms


class _Ptr:
    value = 1 << 20


class _Buf:
    """stands in for a DeviceBuffer: the checks under test raise before anything touches it"""
    class ctx:
        device = 0
    ptr = _Ptr()


def test_argument_errors_before_the_device():
    whole = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1)
    part = functions.DeviceSignal(_Buf(), 6, (5, 7), 0, 1, vox0=0, count=20)
    sharded = functions.ShardedDeviceSignal([part], (5, 7))
    for kw in (dict(), dict(rank=3, energy=0.99)):                      # neither, both
        with pytest.raises(ValueError, match="exactly one"):
            match.compress(whole, **kw)
    for rank in (0, 65, 7):                                             # 7: above the 6 records
        with pytest.raises(ValueError, match="rank"):
            match.compress(whole, rank=rank)
        with pytest.raises(ValueError, match="rank"):
            match.compress(np.zeros((6, 4, 4)), rank=rank)
    for energy in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="energy"):
            match.compress(whole, energy=energy)
    for bad in (sharded, part):
        with pytest.raises(NotImplementedError, match="dictionary"):
            match.compress(bad, rank=2)
    # a compressed dictionary of 6 records at rank 2, without a device: only the record counts 6 and 2 are taken
    Uh, lam = match.gram_basis(np.diag(np.arange(6.0, 0.0, -1.0)))
    basis = match.Basis(Uh, lam, 2)
    cdic = match.Dictionary.__new__(match.Dictionary)
    cdic.basis, cdic.nrec, cdic.natoms, cdic.grid = basis, 2, 35, (5, 7)
    basis.dictionary = cdic
    for nrec in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="records"):
            match.match(cdic, np.zeros((nrec, 3)))
    with pytest.raises(ValueError, match="records"):
        basis.project(np.zeros((5, 3)))
    with pytest.raises(NotImplementedError, match="signals"):
        basis.project(part)


@pytest.fixture(scope="module")
def decay():
    D, S, rank = cc.compressed_cases()["decay_257_67_37"]
    return D, S, rank


def test_host_half_on_exact_input(decay):
    """gauge, reproducibility, orthonormality and captured energy of the host half on the extended-precision Gram matrix"""
    D = decay[0]
    G = cc.gram64(D)
    U, lam = match.gram_basis(G)
    nrec = D.shape[0]
    assert U.shape == (nrec, nrec) and U.dtype == np.complex128 and lam.shape == (nrec,) and (np.diff(lam) <= 0).all()
    # the gauge: the component of largest modulus of every column (the first among equals) is real and positive
    k = np.argmax(np.abs(U), axis=0)
    pivot = U[k, np.arange(nrec)]
    assert (pivot.imag == 0).all() and (pivot.real > 0).all()
    for _ in range(2):
        again, lam2 = match.gram_basis(G.copy())
        assert again.tobytes() == U.tobytes() and lam2.tobytes() == lam.tobytes()
    # a phase on the input columns of eigh must not come through: the gauge of a scaled eigenvector is the same vector
    ortho = float(np.abs(U.conj().T @ U - np.eye(nrec)).max())
    print("max |U^H U - I| =", ortho)
    assert ortho <= cc.ORTHO_BOUND
    sv = np.linalg.svd(D, compute_uv=False)
    for rank in cc.HOST_RANKS:
        kept = float((np.abs(U[:, :rank].conj().T @ D) ** 2).sum())
        err = abs(kept - float((sv[:rank] ** 2).sum())) / float(sv[0] ** 2)
        print("rank", rank, "captured energy off by", err, "of sigma_0^2")
        assert err <= cc.ENERGY_BOUND
    basis = match.Basis(U, lam, 6)
    assert basis.U.shape == (nrec, 6) and basis.s.shape == (nrec,) and basis.rank == 6 and basis.nrec == nrec
    assert np.allclose(basis.s[:6], sv[:6], rtol=1e-9) and (basis.s >= 0).all() and 0.999 < basis.energy <= 1.0


def test_gauge_removes_the_phase():
    rng = np.random.default_rng(5)
    A = mc._cgauss(rng, (9, 30))
    G = A @ A.conj().T
    U, _ = match.gram_basis(G)
    V = U * np.exp(2j * np.pi * rng.random(9))[None, :]                 # any other phase convention of the same eigenvectors
    k = np.argmax(np.abs(V), axis=0)
    p = V[k, np.arange(9)]
    assert np.abs(V * (np.conj(p) / np.abs(p))[None, :] - U).max() <= 4 * cc.U


def test_unresolved_rank_and_energy_selection():
    D = cc.rank3_dictionary()
    U, lam = match.gram_basis(cc.gram64(D))
    assert match.resolved_rank(lam) == 3
    with pytest.raises(ValueError, match="largest resolvable rank is 3"):
        match.select_rank(lam, rank=5)
    assert match.select_rank(lam, rank=3) == 3
    # energy=: the smallest sufficient rank
    lam = np.array([8.0, 1.0, 0.5, 0.25, 0.125, 0.125])
    share = np.cumsum(lam) / lam.sum()
    for energy, want in ((0.5, 1), (0.8, 1), (0.81, 2), (0.9, 2), (0.95, 3), (0.975, 4), (0.98, 5), (1.0, 6)):
        got = match.select_rank(lam, energy=energy)
        assert got == want and share[got - 1] >= energy and (got == 1 or share[got - 2] < energy), (energy, got)
    flat = np.ones(200)
    with pytest.raises(ValueError, match="64"):
        match.select_rank(flat, energy=0.9)
    with pytest.raises(ValueError, match="64"):
        match.select_rank(flat, rank=65)
    with pytest.raises(ValueError, match="no valid atom"):
        match.select_rank(np.zeros(5), rank=1)
    with pytest.raises(ValueError, match="exactly one"):
        match.select_rank(lam)


def test_yardstick_accepts_float64_and_rejects_1e_12():
    """the plain float64 formulas pass both bounds; one entry off by 1e-12 relative does not"""
    cases = cc.cases()
    for name in ("gauss_33_37", "gauss_257_65", "decay_257_37", "invalid"):
        D, S = cases[name]
        Dv = D[:, cc.valid_atoms(D)]
        G = Dv @ Dv.conj().T
        cc.check_gram(G, D, name)
        s = min(2, D.shape[0] - 1)                   # (a diagonal entry: there sum |D||D| is the entry itself)
        bad = G.copy()
        bad[s, s] *= 1 + 1e-12
        with pytest.raises(AssertionError):
            cc.check_gram(bad, D, name)
        B = cc.host_basis(D)[:, :4]
        out = B.conj().T @ S
        cc.check_project(out, B, S, name)
        bad = out.copy()
        bad[1, 3] *= 1 + 1e-12
        with pytest.raises(AssertionError):
            cc.check_project(bad, B, S, name)


def test_invalid_case_is_what_it_says():
    D, _ = cc.invalid_case()
    assert list(np.flatnonzero(~cc.valid_atoms(D))) == [3, 8, 16]
    ref, bound = cc.gram_ref(D)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()


def test_compressed_cases_are_decisive():
    """>= 90 % of the voxels are decisive under the extended-precision yardstick on (U^H D, U^H S) alone"""
    for name, (D, S, rank) in cc.compressed_cases().items():
        U, lam = match.gram_basis(cc.gram64(D))
        assert match.select_rank(lam, rank=rank) == rank
        Ur = U[:, :rank]
        y = mc.Yardstick(Ur.conj().T @ D, Ur.conj().T @ S)
        share = y.decisive.mean()
        assert share >= 0.9, (name, float(share))
