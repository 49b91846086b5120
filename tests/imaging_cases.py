"""Spatial read-out cases for the tests: the G20 sequences (tests/golden/make_golden_imaging.py builds the same ones from the
reference's operators), random read-out problems, and an extended-precision restatement of the sum over phase states.

Everything keeps |k . x| <= 1000 rad, which the tolerance of the tests is derived for (`bound`)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g20_imaging.npz")

FOV, NPIX = 0.2, 16            # m, pixels per side of the 2-D cases
T2_IMG = [50.0, 70.0, 90.0]


def lattice(npix=NPIX, fov=FOV):
    """pixel centres of an npix x npix lattice over the field of view: [npix * npix, 2] (m)"""
    ax = (np.arange(npix) - npix // 2) * (fov / npix)
    return np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)


def phantom(npix=NPIX, fov=FOV):
    """proton density of three tissues on the lattice, [3, npix * npix]: a disc, the ring around it and a small square;
    zero elsewhere (most of every map)"""
    x, y = lattice(npix, fov).T / fov
    r = np.hypot(x, y)
    disc = np.where(r < 0.17, 1.0, 0.0)
    ring = np.where((r >= 0.17) & (r < 0.30), 0.6 + 0.4 * x, 0.0)
    square = np.where((np.abs(x - 0.33) < 0.07) & (np.abs(y + 0.30) < 0.1), 0.8, 0.0)
    return np.stack([disc, ring, square])


def gre_lines(ns, nline, imaging, npix=NPIX, spoil=False, T2=T2_IMG):
    """`nline` phase-encode lines of a gradient-echo read-out: excitation, prephasing, npix samples of `imaging(line)` one
    read-out step apart, then a shift that does NOT rewind (the lines mix)"""
    seq = []
    for j in range(nline):
        phi = 117.0 * j * (j + 1) / 2 if spoil else 0.0
        seq += [ns.T(30, phi), ns.S([-(npix // 2), j - nline // 2])]
        seq += [imaging(j, phi), ns.E(0.1, 1000, T2), ns.S([1, 0])] * npix
        seq += [ns.S([npix // 4, nline // 2 - j])]
    return seq


K3 = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -1, 1]])[:, None, :]     # one shift vector per point of grid axis 0
POS_542 = np.stack(np.meshgrid(np.linspace(-0.4, 0.4, 5), np.linspace(-0.3, 0.5, 4), indexing="ij"), axis=-1)
POS_543 = np.concatenate([POS_542, (0.1 * np.arange(20).reshape(5, 4, 1) - 0.45)], axis=-1)
POS_7 = np.linspace(-0.5, 0.45, 7)
W_4354 = (1 + np.arange(240).reshape(4, 3, 5, 4) % 7) * np.exp(0.3j * np.arange(240).reshape(4, 3, 5, 4))
W_54 = 0.5 + np.arange(20.0).reshape(5, 4) / 10


def cases(ns):
    """{name: (sequence, simulate keywords)}; `ns` provides T, E, S, ADC, DFT, Imaging, System.  Probes handed over with
    `probe=` are acquired at the sequence's ADC; every Imaging with weights of its own is acquired once"""
    out = {}
    # --- 1-D
    pos31 = 1e-2 * np.linspace(-0.5, 0.5, 31)
    out["dft_1d"] = ([ns.T(10, 0), ns.E(1, 1000, [30, 60, 90]), ns.S(1)] * 20 + [ns.S(-10), ns.DFT(pos31)], {"kvalue": 300})
    pos301 = 1e-2 * np.linspace(-0.5, 0.5, 301)
    train = []
    for i in range(200):
        train += [ns.T(12, 7 * i), ns.E(1, 1000, [35.0, 70.0, 140.0], 0.01), ns.S(1)]
    out["dft_1d_long"] = (train + [ns.ADC], {"kvalue": 500, "probe": [
        ns.DFT(pos301), ns.Imaging(pos301, voxel_size=1e-2 / 301, reduce=False)]})
    # --- 2-D gradient echo, weights from the system
    pix, pd, size = lattice(), phantom(), FOV / NPIX
    system = ns.System(weights=pd, kvalue=2 * np.pi / FOV)
    for label, reduce in (("all", True), ("none", False), ("ax0", (0,)), ("ax1", (1,))):
        out[f"img_2d_{label}"] = ([system] + gre_lines(ns, 4, lambda j, phi, r=reduce: ns.Imaging(pix, voxel_size=size, reduce=r)), {})
    out["img_2d_noweights"] = ([ns.System(kvalue=2 * np.pi / FOV)] + gre_lines(
        ns, 4, lambda j, phi: ns.Imaging(pix, voxel_size=size, reduce=(1,))), {})
    out["img_2d_spoiled"] = ([system] + gre_lines(
        ns, 4, lambda j, phi: ns.Imaging(pix, voxel_size=size, phase=-phi), spoil=True), {})
    # --- 3-D coordinates that differ between voxel classes
    seq3 = [ns.System(kvalue=[60, 50, 40])]
    for i in range(6):
        seq3 += [ns.T(25, 30 * i), ns.E(2, 900, [[40.0, 80.0, 120.0]]), ns.S(K3)]
    seq3 += [ns.S(-2 * K3), ns.ADC]
    out["classes_3d"] = (seq3, {"probe": [
        ns.DFT(POS_542),
        ns.DFT(POS_543),
        ns.DFT(POS_7),
        ns.Imaging(POS_542, voxel_size=0.02, reduce=False),
        ns.Imaging(POS_543, voxel_size=[0.02, 0.03, 0.05], reduce=False),
        ns.Imaging(POS_543, voxel_size=0.03, weights=W_4354, reduce=False),
        ns.Imaging(POS_543, voxel_size=0.03, weights=W_4354, reduce=(0,)),
        ns.Imaging(POS_542, voxel_size=[0.02, 0.03, 0.05], weights=W_54, reduce=(2, 3)),
        ns.Imaging(POS_542, voxel_shape="point", weights=W_54, reduce=(0,)),
        ns.Imaging(POS_7, voxel_size=0.04, reduce=False),
    ]})
    return out


def record_names(name, kw):
    """keys of the stored records of one case"""
    n = len(kw.get("probe", [None]))
    return [f"{name}_{i}" for i in range(n)]


# ---------------------------------------------------------------------------------------------- extended precision
def fold_terms(half, k, w):
    """the rows of a folded state [nvox, 3, K] as (F [nvox, 2 nrow - 1], k [2 nrow - 1, d], w [2 nrow - 1]): stored orders
    first, then their mirror images (row -k: conj(B_j), wavenumber -k_j, the same factor)"""
    nrow = len(k)
    A, B = half[:, 0, :nrow], half[:, 1, :nrow]
    return (np.concatenate([A, np.conj(B[:, 1:])], axis=1), np.concatenate([k, -k[1:]], axis=0),
            np.concatenate([w, w[1:]], axis=0))


def longdouble_image(F, k, w, pos, phasor=1.0):
    """im[v, p] = phasor * sum_r w_r F[v, r] exp(i k_r . x_p) in np.longdouble: theta, sin / cos and the sum (the inputs are
    the doubles the device receives)"""
    ld = np.longdouble
    theta = np.asarray(k, ld) @ np.asarray(pos, ld).T                    # [R, P]
    c, s = np.cos(theta), np.sin(theta)
    fr = np.asarray(F.real, ld) * np.asarray(w, ld)
    fi = np.asarray(F.imag, ld) * np.asarray(w, ld)
    re, im = fr @ c - fi @ s, fr @ s + fi @ c
    pr, pi = ld(np.real(phasor)), ld(np.imag(phasor))
    return (re * pr - im * pi).astype(np.float64) + 1j * (re * pi + im * pr).astype(np.float64)


def magnitude(F, w):
    """M = sum_r |w_r F_r| per voxel: the scale of the rounding bound"""
    return (np.abs(F) * np.abs(w)).sum(axis=-1)


def bound(M):
    """per-element bar of a read-out record whose terms add up to M in magnitude.  A term w F exp(i theta) carries the error
    of theta: the device may form theta in another operation order than the reference, at most 3 roundings, i.e.
    3 eps |theta|; with |theta| <= 1000 that is 6.7e-13 M, and the reference's own distance to the extended-precision sum is
    1.2e-15 M at |theta| <= 500.  Hence 1e-12 max(1, M) -- the project's 1e-12 bar on O(1) signals"""
    return 1e-12 * np.maximum(1.0, M)


def random_problem(seed, nvox, nrow, npos, d, box):
    """(half [nvox, 3, K], K, k [nrow, d], w [nrow], pos [npos, d]) with |k . x| <= 1000"""
    rng = np.random.default_rng(seed)
    K = next(c for c in (64, 128, 256, 512, 1024) if c >= nrow)
    half = np.zeros((nvox, 3, K), np.complex128)
    decay = np.exp(-np.arange(nrow) / max(nrow / 3, 1.0))
    half[:, :, :nrow] = (rng.standard_normal((nvox, 3, nrow)) + 1j * rng.standard_normal((nvox, 3, nrow))) * decay
    half[:, 1, 0] = np.conj(half[:, 0, 0])
    half[:, 2, 0] = half[:, 2, 0].real
    kmax, xmax = 2000.0, 0.5 / d
    k = rng.uniform(-kmax, kmax, (nrow, d))
    k[0] = 0
    pos = rng.uniform(-xmax, xmax, (npos, d))
    w = np.sinc(k * 2e-3 / 2 / np.pi).prod(-1) if box else np.ones(nrow)
    if box and nrow > 2:
        w[nrow // 2] = 0.0          # a dropped order
    return half, K, k, w, pos


RANDOM = [(nrow, npos, 1 + (i + j) % 3, (i + j) % 2 == 1, nvox)
          for i, nrow in enumerate((1, 2, 63, 64, 65, 200, 1024))
          for j, (npos, nvox) in enumerate(((1, 3), (7, 17), (64, 256), (301, 277)))]
