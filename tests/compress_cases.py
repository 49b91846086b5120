"""Yardstick and seeded cases of the dictionary-compression tests (tests/test_compress_host.py on the CPU,
tests/test_gpu_compress.py).

References are computed in np.clongdouble and a float64 result is held to bounds DERIVED from the inner-product error bound
(Higham, Accuracy and Stability, 3.1: |fl(x.y) - x.y| <= gamma_n sum |x_i||y_i|, which holds for ANY order of summation), with
u = 2^-53 and a complex product counted as four real ones -- not to anything measured:

    Gram:     |G_dev[s,t] - G_ref[s,t]|  <=  4 (nvalid + 4) u  sum over valid a of |D[s,a]| |D[t,a]|
    project:  |out[r,c] - ref[r,c]|      <=  4 (nrec + 4) u    sum_t |U[t,r]| |X[t,c]|

An atom is valid when its norm sum_t |D[t,a]|^2 is a finite number > 0 (the rule of match).

The two constants at the end bound what numpy.linalg.eigh leaves of the host half; LAPACK's constants are not derivable, so
these -- and only these -- are measured values with a margin of 8.
"""
import numpy as np

from tests import match_cases as mc

U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble


def valid_atoms(D):
    with np.errstate(all="ignore"):
        n = (np.abs(D.astype(CLD)) ** 2).sum(axis=0)
        return np.isfinite(n) & (n > 0)


def gram_ref(D):
    """(G_ref clongdouble [nrec, nrec], bound longdouble [nrec, nrec]) over the valid columns of D [nrec, natoms]"""
    D = np.asarray(D, dtype=np.complex128)
    Dv = D[:, valid_atoms(D)].astype(CLD)
    A = np.abs(Dv)
    return Dv @ np.conj(Dv).T, LD(4 * (Dv.shape[1] + 4) * U) * (A @ A.T)


def project_ref(B, X):
    """(ref clongdouble [rank, ncol], bound longdouble [rank, ncol]) of B^H X for B [nrec, rank], X [nrec, ncol] (finite)"""
    B, X = np.asarray(B, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    return np.conj(B.astype(CLD)).T @ X.astype(CLD), LD(4 * (B.shape[0] + 4) * U) * (np.abs(B).astype(LD).T @ np.abs(X).astype(LD))


def check(got, ref, bound, what=""):
    """asserts |got - ref| <= bound entry by entry; returns the largest used fraction of the bound (for printing)"""
    got = np.asarray(got)
    assert got.dtype == np.complex128 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(CLD) - ref)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, bad[:4].tolist(), [float(err[tuple(i)]) for i in bad[:4]], [float(bound[tuple(i)]) for i in bad[:4]])
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0), initial=0.0))


def check_gram(G, D, what=""):
    ref, bound = gram_ref(D)
    return check(G, ref, bound, what)


def check_project(out, B, X, what=""):
    ref, bound = project_ref(B, X)
    return check(out, ref, bound, what)


def gram64(D):
    """the extended-precision Gram matrix rounded to float64: exact input for the host half"""
    return gram_ref(D)[0].astype(np.complex128)


# ---------------------------------------------------------------------------------------------------------- seeded cases
# (natoms, nrec).  Around the 16 x 16 x 4 tile and a 64-wide block: the issue's list; then both sides of the constants of
# csrc/epgx_compress.h -- the 64-record block of gram_kernel (63, 64; 65 and 130 are in the list), its 16-atom LDS chunk (15, 16,
# 17 atoms are in the list), the 16 records of project_kernel's unrolled group (15, 16; 17 is in the list), the 64 / 32 / 16
# columns of a wavefront and 256 / 128 / 64 of a workgroup (255 atoms; 257 is in the list; rank 16 | 17 and 32 | 33 switch the
# variant), and GRAM_MIN_ATOMS = 1024, where the library's own nsplit goes from 1 to 2 (2047, 2048 atoms).
SHAPES = [(1, 1), (15, 3), (16, 4), (17, 5), (33, 37), (257, 5), (257, 65), (1025, 17), (33, 130),
          (33, 63), (33, 64), (33, 15), (255, 16), (2047, 4), (2048, 5)]
LONG = (33, 1000)
RANKS = (1, 4, 15, 16, 17, 33, 64)
NMEAS = 19


def invalid_case():
    """match_cases.invalid_case: 17 atoms, 5 records; atom 3 is all zero, atom 16 holds a NaN, atom 8 an Inf"""
    return mc.invalid_case()[:2]


def cases():
    """name -> (D [nrec, natoms], S [nrec, NMEAS])"""
    out = {}
    for natoms, nrec in SHAPES + [LONG]:
        out[f"gauss_{natoms}_{nrec}"] = mc.gaussian_case(3, natoms, NMEAS, nrec)[:2]
    out["decay_257_37"] = mc.decaying_case(2, 257, 67, 37)[:2]
    out["invalid"] = invalid_case()
    return out


def ranks_for(nrec):
    return [r for r in RANKS if r <= nrec]


def host_basis(D):
    """U [nrec, nrec] of the host half on the exact Gram matrix of D"""
    from epgpy_amd import match
    return match.gram_basis(gram64(D))[0]


# the cases matched in the compressed space: name -> (D, S, rank).  Rank and noise are chosen so that the extended-precision
# yardstick of match_cases on (U^H D, U^H S) alone finds >= 90 % of the voxels decisive (tests/test_compress_host.py).
def compressed_cases():
    return {"decay_257_67_37": mc.decaying_case(2, 257, 67, 37)[:2] + (6,),
            "gauss_257_67_37": mc.gaussian_case(1, 257, 67, 37)[:2] + (16,)}


def rank3_dictionary():
    """40 atoms, 12 records, every atom a combination of 3 fixed columns: G has 3 eigenvalues above rounding"""
    rng = np.random.default_rng(31)
    return mc._cgauss(rng, (12, 3)) @ mc._cgauss(rng, (3, 40))


# numpy.linalg.eigh on the exact Gram matrix of the decay_257_67_37 dictionary (37 records), measured on the CPU by
# tests/test_compress_host.py::test_host_half_on_exact_input (printed there), times 8:
ORTHO_BOUND = 8 * 2.3e-15        # max |U^H U - I| over all 37 columns; measured 2.22e-15
ENERGY_BOUND = 8 * 1.1e-15       # | ||U_r^H D||_F^2 - sum_{r<rank} sigma_r^2 | / sigma_0^2 at ranks 1, 4, 6; measured 1.04e-15
HOST_RANKS = (1, 4, 6)           # (the Gram route resolves 10 eigenvalues of this dictionary)
