"""The derivative cases of the tiled path (Jacobians beyond 1024 orders: csrc/epgx_tiled.hip tiled_deriv_kernel,
include/epgx.h epgx_run_tiled_deriv) that tests/test_gpu_tiled_jacobian.py runs on the device and
tests/test_tiled_jacobian_host.py measures on the CPU -- oracle tuples (tests/sequences.py), the variables, the options of
simulate() -- and the per-column check of tests/jacobian_cases.py:

    err_v = max|got[..., v] - ref[..., v]| / max|ref[..., v]|   <=   16 x the case's float64 floor   (never above 1e-11)

against tests/jacobian_recurrence.py (np.clongdouble).  Shapes: five voxels (not a multiple of the four wavefronts of a
workgroup), spin-echo trains of about 530 echoes = 1061 orders = three tiles of 448.  A long T2 against a short echo spacing
and refocusing angles near 130 degrees keep the late echoes fed by what went through the upper tiles; the host test asserts
that in every column the echoes after number 450 reach 1e-3 of the column's maximum."""
import numpy as np

from tests.jacobian_cases import RL

LATE = 450             # echoes behind this one carry what went through the tiles above the first
TAU, ALPHA = 0.4, 130.0

# float64 floors: max over columns of max|oracle - recurrence| / max|column|, measured on the CPU by
# tests/test_tiled_jacobian_host.py and rounded up by half.  16 x a floor may not exceed 1e-11.
FLOORS = {
    "t_one": 6.1e-14, "t_one_nofuse": 6.1e-14, "t_passes": 7.6e-14, "t_shifts": 5.7e-14, "t_plain": 1.6e-13, "t_plain_exact": 1.6e-13,
    "t_init": 2.7e-13, "t_probes": 1.4e-13,
}


def tissue(seed=2300, n=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(800, 2000, n), rng.uniform(250, 450, n), rng.uniform(0.85, 1.15, n)


def stages(seed=2300):
    """(excitation, refocusing pulse, relaxation) of the trains, with their partials"""
    T1, T2, B1 = tissue(seed)
    exc = ("T", 90 * B1, 90, {"order1": {"B1": {"alpha": 90}}})
    rfc = ("T", ALPHA * B1, 0, {"order1": {"B1": {"alpha": ALPHA}, "fa": {"alpha": 1.0}}})
    rlx = ("E", TAU, T1, T2, 0, {"order1": RL})
    return exc, rfc, rlx


def echoes(n, seed=2300):
    _, rfc, rlx = stages(seed)
    return [("S", 1), rlx, rfc, ("S", 1), rlx, ("ADC",)] * n


def mixed_shifts():
    """S(+1) and S(-1); a shift by 5 (the schedule expands it) and by -3; shifts by 40 and -300 / +300 (more than the halo of 32:
    the copy kernel, every window); with max_nstate = 1100 the truncation cuts inside tile 2 (orders 896 .. 1343)"""
    exc, rfc, rlx = stages(2304)
    seq = [exc] + echoes(225, 2304)                                   # 450 orders
    seq += [("S", -1), rlx, rfc, ("S", 1), ("ADC",)]
    seq += [("S", 5), rlx, rfc, ("ADC",), ("S", -3), rlx, ("S", 3), ("ADC",)]        # 455
    seq += [("S", 40), rlx, rfc, ("ADC",)]                            # 495
    seq += echoes(100, 2304)                                          # 695
    seq += [("S", -300), rfc, ("S", 300), ("ADC",)]                   # what sat in the upper tiles comes down and goes back
    return seq + echoes(215, 2304)                                    # 1125 > 1100: truncated


def plain_operators():
    """SPOILER, PD with reset and RESET, each once, after more than 448 orders are populated"""
    exc, rfc, rlx = stages(2305)
    seq = [exc] + echoes(520, 2305)                                   # 1040 orders
    seq += [("SPOILER",), rfc, ("ADC",)] + echoes(5, 2305)            # 1050
    seq += [("PD", 0.8, True), exc] + echoes(230, 2305)               # from equilibrium again: 460 orders
    seq += [("RESET",), exc] + echoes(30, 2305)
    return seq


def init_head(K=1200):
    """operators that prepare a start state of K / 2 + 4 orders (no partials): a few populated orders far up"""
    return [("T", 35.0, 10.0), ("S", 1), ("E", 3.0, 800.0, 90.0, 0), ("T", 50.0, 0.0), ("S", K // 2), ("T", 70.0, 40.0), ("S", 3),
            ("E", 2.0, 800.0, 90.0, 0)]


CASES = {}


def case(name, tuples, variables, *, cap=None, exact=False, fuse=True, head=None, probes=("F0",), columns=None):
    """columns: the probe's variable list where it differs from ["magnitude"] + variables (an unknown variable)"""
    assert name not in CASES and name in FLOORS, name
    CASES[name] = dict(tuples=tuples, variables=list(variables), cap=cap, exact=exact, fuse=fuse, head=head, probes=tuple(probes),
                       columns=columns)


def _define():
    case("t_one", [stages()[0]] + echoes(530), ["T2"])
    case("t_one_nofuse", [stages()[0]] + echoes(530), ["T2"], fuse=False)
    # one more variable than a launch carries (TILED_DERIV_V = 2): passes of two and one; "zzz" is declared by no operator
    case("t_passes", [stages(2303)[0]] + echoes(530, 2303), ["T1", "T2", "B1"], columns=["magnitude", "T1", "T2", "zzz", "B1"])
    case("t_shifts", mixed_shifts(), ["T2", "B1"], cap=1100)
    case("t_plain", plain_operators(), ["T2"])
    case("t_plain_exact", plain_operators(), ["T2"], exact=True)
    case("t_init", echoes(480, 2306), ["T2", "fa"], head=init_head())
    case("t_probes", [stages(2307)[0]] + echoes(530, 2307), ["T2", "B1"], probes=("F0", "Z0"))


_define()


def full_tuples(c):
    return (c["head"] or []) + c["tuples"]


def plain(tuples):
    return [t[:-1] if isinstance(t[-1], dict) else t for t in tuples]
