"""Float-wavenumber (shift-merge) cases shared by the golden generator (tests/golden/make_golden_merge.py, which drives the
reference) and the tests (which drive this package): `build(epg, name)` returns (operators, options) from whichever `epg`
namespace it is given.  Parameters come from seeded generators, so both sides see the same numbers."""
import numpy as np


def _uniform(seed, lo, hi, n):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def grad3d(epg, nvox, cycles=6):
    """the 3-D two-gradient train: two gradient lobes on different axes per cycle, relaxation, one refocusing pulse per voxel"""
    rng = np.random.default_rng(3)
    T2, alpha = rng.uniform(30, 200, nvox), rng.uniform(100, 170, nvox)
    g1, g2 = epg.G(1.0, [3.7, 0, 0]), epg.G(0.6, [0, 2.9, 0])
    relax, refoc = epg.E(5, 1000, T2), epg.T(alpha, 0)
    return [epg.T(90, 90)] + [g1, relax, refoc, g2, relax, epg.ADC] * cycles, {"kgrid": 500}


def multi1d(epg, nvox=3):
    """1-D, two float shifts whose sums fall into shared grid cells: destinations with more than one source per component,
    and a refocused pair of rows that the pruning removes"""
    alpha = _uniform(5, 40, 120, nvox)
    s1, s2 = epg.S(1.0), epg.S(0.55)
    relax = epg.E(3, 800, 90)
    seq = [epg.T(90, 90), s1, epg.T(180, 0), s1, epg.ADC]                       # the echo: rows +-1 end up empty
    seq += [s1, relax, epg.T(alpha, 30), s2, relax, epg.T(alpha, 0), epg.ADC] * 4
    return seq, {"kgrid": 0.37}


def long1d(epg, nvox=2, cycles=70):
    """a train whose state matrix crosses 64 stored orders (a second capacity class).  The highest order of such a train decays
    geometrically and passes every fixed tolerance at some echo: the pruning tolerance sits below the whole train"""
    alpha = _uniform(7, 90, 120, nvox)
    shift, relax, refoc = epg.S(1.3717, prune=1e-25), epg.E(2, 1000, 300), epg.T(alpha, 0)
    return [epg.T(90, 90)] + [shift, relax, refoc, shift, epg.ADC] * (cycles // 2), {"kgrid": 1.0}


def mixed(epg, nvox=4):
    """an integer shift once float coordinates exist, and diffusion on float coordinates"""
    alpha = _uniform(11, 20, 80, nvox)
    seq = [epg.T(alpha, 90), epg.S(1.2), epg.E(4, 900, 70), epg.T(50, 20), epg.S(1), epg.D(10, 0.4), epg.ADC,
           epg.S([0.7]), epg.T(alpha, 0), epg.D(5, 0.4), epg.S(2), epg.ADC]
    return seq, {"kgrid": 0.25, "kvalue": 30.0}


def t2star(epg, nvox=70):
    """T2* decay: the time accumulation C after one excitation per voxel; F0 = sin(alpha) / 1 * exp(-0.1 n) * ..."""
    alpha = _uniform(13, 20, 90, nvox)
    return [epg.T(alpha, 90)] + [epg.C(0.5, 1 / 5), epg.ADC] * 20, {"kgrid": 0.1}


CASES = {
    "grad3d_1": lambda epg: grad3d(epg, 1),
    "grad3d_5": lambda epg: grad3d(epg, 5),
    "grad3d_70": lambda epg: grad3d(epg, 70),
    "multi1d": multi1d,
    "long1d": long1d,
    "mixed": mixed,
    "t2star": t2star,
}
PER_SHIFT = ("grad3d_5", "multi1d", "long1d", "mixed")       # cases whose states / coords around every shift are recorded



def recorded(name, index):
    """whether shift `index` of a PER_SHIFT case is recorded: every one, except in the long train -- there every eighth and
    those around and past 64 stored orders"""
    return name != "long1d" or index % 8 == 0 or index >= 60


# constructor calls of G / C whose attributes are recorded from the reference: (class name, args, kwargs)
ATTRIBUTES = [
    ("G", (1.0, [3.7, 0, 0]), {}),
    ("G", (0.6, 2.5), {"duration": True}),
    ("G", ([1.0, 2.0], [[1.0, 0.5], [0.2, 0.1]]), {}),
    ("G", (2.0, [0.1, 0.2]), {"duration": 7}),
    ("C", (0.5, 1 / 5), {}),
    ("C", (2.0,), {"duration": True}),
    ("C", (1.5, [0.1, 0.2, 0.4]), {}),
]


def build(epg, name):
    return CASES[name](epg)


def is_merge_shift(epg, op, coords):
    """True if `op` is a shift that takes the shift-merge on coordinates `coords` (None, int or float array)"""
    if not isinstance(op, epg.S):
        return False
    floating = coords is not None and np.asarray(coords).dtype.kind == "f"
    return floating or (not isinstance(op.k, int) and np.asarray(op.k).dtype.kind == "f")
