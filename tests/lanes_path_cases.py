"""The cases that hold the three one-voxel-per-lane kernels of the growing launch -- rows_grow_lanes_kernel<NSP, true> (`train`),
rows_grow_lanes_kernel<NSP, false> (`any list`) and rows_grow_lanes_kernel_odd<NSP, 12> (`lanes-odd`), NSP 0 / 1 / 2 / 4 each
(epgx_grow_lanes.hip, epgx_grow_lanes_odd.hip; selection: epgx_launch_grow.h) -- to the extended-precision recurrence
(tests/signal_recurrence.py) PER RECORD, with the check, MARGIN and CAP of tests/signal_cases.py:

    for every record r   max_vox|gpu[r] - ref[r]|  <=  16 floor max_vox|ref[r]|,   a record of zeros exactly zero

`floor`: the largest per-record error of the float64 NumPy oracle on the case (FLOORS, measured on the CPU and held between one
and two times the measurement by tests/test_lanes_paths_host.py).

Grids: a wave holds 64 consecutive voxels and a workgroup one wave, so the smallest grids with a third workgroup and a ragged
last one: 131 voxels (64 + 64 + 3), 128 (no ragged wave), 1; on two axes 11 x 13 = 143 with (T1, T2) dense over both axes
(one index space, the headline's form) and with (T1, T2) on one axis and B1 in the excitation on the other (two); 7 x 19 = 133
with three index spaces (the kernels' NSP = 4), built as tests/signal_cases.py::tissue(3, ..) builds its third space: B1 along
the first axis, a further relaxation along the second; 131 voxels that share every table (scalar parameters over shape=:
no index space, NSP = 0).  T2 within a factor of three inside a case.

Every case records what EPGX_TRACE must print for it on each side (trace_of): the family line `rows_grow_kernel<NSP>`, the
variant line with the kernel and L.  L = 1 + max min(top, rem) = 1 + (shifts up to the last probe) // 2 (lanes_plan).

Run as a script -- `lanes_path_cases.py OUT.npz` -- it runs every case through simulate() and writes the signals; with
EPGX_PATHS_SUBRANGE=1 it also launches the voxel sub-ranges SUBRANGES of the cases SUB_CASES through _lib.run into a buffer
that covers the whole grid and is filled with 7 + 7i; with EPGX_PATHS_THRESHOLD=1 the four launches THRESHOLD at and just
below LANES_MIN_VOXELS = 2^19 voxels, each written to OUT.npz.<name>.npy.  `[case] name` goes to stderr before each launch, so
that the library's trace lines can be attributed.  tests/test_gpu_lanes_paths.py starts it once per side."""
import os
import sys

import numpy as np

if __name__ == "__main__":     # (as a script: the repository root is not on the path yet)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.signal_cases import MARGIN, CAP, check_records     # noqa: E402, F401  (the check and its constants: one definition)

TRAIN, ANY, ODD = "train", "any list", "lanes-odd"
KERNELS = (TRAIN, ANY, ODD)
NSPS = (0, 1, 2, 4)
DECK = {TRAIN: 16, ANY: 14}
TAIL = 14                      # unprobed echoes behind the probed ones of a tail_<n> case: the launch grows, L = n + 1
LANES_MIN_VOXELS = 1 << 19     # epgx_planner.h

# every side is one child process; `default` sets none of the knobs: launches below 2^19 voxels take the rows variant
SIDES = {
    "lanes": {"EPGX_LANES": "2"},
    "train_off": {"EPGX_LANES": "2", "EPGX_LANES_TRAIN": "0"},
    "body_off": {"EPGX_LANES": "2", "EPGX_LANES_BODY": "0"},
    "odd": {"EPGX_LANES": "2", "EPGX_LANES_ODD": "2"},
    "default": {},
}
KNOBS = ("EPGX_LANES", "EPGX_LANES_BODY", "EPGX_LANES_TRAIN", "EPGX_LANES_ODD", "EPGX_TRACE", "EPGX_PATHS_SUBRANGE", "EPGX_PATHS_THRESHOLD")

# float64 floors: the largest per-record error of the oracle against the recurrence, measured on the CPU by
# tests/test_lanes_paths_host.py and rounded up to two digits.  A floor is never raised to make a device case pass; a case whose
# ORACLE needs 16 x floor > 2e-12 gets other inputs.
FLOORS = {
    "train_16_131": 2.0e-15, "train_17_131": 2.1e-15, "train_20_131": 2.3e-15, "train_23_131": 2.5e-15, "tail_3_131": 5.9e-16,
    "tail_4_131": 7.8e-16, "tail_7_131": 1.0e-15, "tail_8_131": 1.0e-15, "tail_14_131": 1.7e-15, "tail_15_131": 1.8e-15,
    "odd_lead_20_131": 0.0, "two_heads_17_131": 7.0e-15, "unprobed_middle_20_131": 2.3e-15, "unfused_17_131": 2.1e-15,
    "b1_voxel_17_131": 2.8e-15, "train_20_128": 2.4e-15, "train_17_1": 9.2e-16, "train_20_11x13": 2.8e-15,
    "odd_lead_20_11x13": 0.0, "unfused_20_11x13": 2.8e-15, "train_17_11+13": 2.5e-15, "train_23_11+13": 3.2e-15,
    "tail_7_11+13": 1.3e-15, "unfused_17_11+13": 2.5e-15, "b1_refocus_17_11+13": 3.3e-15, "mrf_40_11+13": 9.5e-15, "train_17_7x19": 1.7e-15,
    "train_20_7x19": 2.0e-15, "tail_8_7x19": 1.3e-15, "unfused_17_7x19": 1.7e-15, "train_17_shared": 1.5e-15,
    "train_20_shared": 1.6e-15, "unfused_17_shared": 1.5e-15,
}
# (odd_lead_*: every probe behind a lone S(+1) reads the parity nothing reaches -- the reference and the oracle are identically
# zero, the floor is zero, and the device must return exact zeros)

CASES = {}


def case(name, tuples, kernel, nsp, *, shape=None, fuse=True):
    """kernel: what the launch traces under EPGX_LANES=2 alone (TRAIN or ANY); nsp: the NSP of its family name"""
    assert name not in CASES and kernel in (TRAIN, ANY) and nsp in NSPS, name
    last = max(i for i, t in enumerate(tuples) if t[0] == "ADC")
    shifts = sum(1 for t in tuples[:last] if t[0] == "S")
    # LanesPlan::odd: a train whose shifts up to the last probe are even (a lone S(+1) behind the excitation makes them odd)
    CASES[name] = dict(tuples=tuples, kernel=kernel, nsp=nsp, shape=shape, fuse=fuse, L=1 + shifts // 2,
                       odd=kernel == TRAIN and shifts % 2 == 0)


def grid_of_case(c):
    from tests.signal_recurrence import signal_grid
    return tuple(c["shape"]) if c["shape"] is not None else tuple(signal_grid(c["tuples"]))


def grids():
    rng = np.random.default_rng(52)
    t1 = lambda *s: rng.uniform(600, 2000, s)
    t2 = lambda *s: rng.uniform(25.0, 70.0, s)            # within a factor of three
    return {
        "131": (t1(131), t2(131)), "128": (t1(128), t2(128)), "1": (t1(1), t2(1)),
        "11x13": (t1(11, 1), t2(1, 13)),                                                   # dense over both axes
        "11+13": (t1(11, 1), t2(11, 1), rng.uniform(0.85, 1.15, (1, 13))),                 # (T1, T2) | B1
        "7x19": (t1(7, 1), t2(1, 19), rng.uniform(0.85, 1.15, (7, 1))),                    # (T1, T2) dense, B1 | ., a relaxation . | T2
    }


def _define():
    from tests import reach_cases, sequences as sq
    from oracle import workloads as ow

    echo = reach_cases.echo
    g = grids()

    def train(T1, T2, necho, head=None, tail=0):
        return (head or [("T", 90, 90)]) + echo(T1, T2) * necho + echo(T1, T2, adc=None) * tail

    # one index space, 131 voxels: both sides of the deck of 16, the benchmark's train, the cap L = 24; the windows below the deck
    T1, T2 = g["131"]
    for n in (16, 17, 20, 23):
        case(f"train_{n}_131", ow.mse_tuples(T1, T2, necho=n), TRAIN, 1)
    for n in (3, 4, 7, 8, 14, 15):
        case(f"tail_{n}_131", train(T1, T2, n, tail=TAIL), TRAIN, 1)
    # a lone S(+1) behind the excitation: even windows on the way up, every probe reads the other parity -- zeros
    case("odd_lead_20_131", [("T", 90, 90), ("S", 1)] + echo(T1, T2) * 20, TRAIN, 1)
    # two records before the first shift: a relaxation with precession between two rotations keeps them apart
    case("two_heads_17_131", train(T1, T2, 17, head=[("T", 90, 90), ("E", 3.0, T1, T2, 0.1), ("T", 15, 40)]), TRAIN, 1)
    case("unprobed_middle_20_131", [("T", 90, 90)] + echo(T1, T2) * 5 + echo(T1, T2, adc=None) * 5 + echo(T1, T2) * 10, TRAIN, 1)
    case("unfused_17_131", ow.mse_tuples(T1, T2, necho=17), ANY, 1, fuse=False)                     # pair records
    # B1 per voxel, on the axis of (T1, T2): E . T . E still fuses on the host, into per-voxel tables -- a train
    case("b1_voxel_17_131", ow.mse_tuples(T1, T2, B1=np.random.default_rng(53).uniform(0.85, 1.15, 131), necho=17), TRAIN, 1)
    T1, T2 = g["128"]
    case("train_20_128", ow.mse_tuples(T1, T2, necho=20), TRAIN, 1)
    T1, T2 = g["1"]
    case("train_17_1", ow.mse_tuples(T1, T2, necho=17), TRAIN, 0)        # (a table of one entry varies along no axis: no index space)
    # 11 x 13, dense: the three lists of the threshold launches
    T1, T2 = g["11x13"]
    case("train_20_11x13", ow.mse_tuples(T1, T2, necho=20), TRAIN, 1)
    case("odd_lead_20_11x13", [("T", 90, 90), ("S", 1)] + echo(T1, T2) * 20, TRAIN, 1)
    case("unfused_20_11x13", ow.mse_tuples(T1, T2, necho=20), ANY, 1, fuse=False)
    # 11 x 13, two index spaces: only the excitation depends on B1
    T1, T2, B1 = g["11+13"]
    for n in (17, 23):
        case(f"train_{n}_11+13", train(T1, T2, n, head=[("T", 90 * B1, 90)]), TRAIN, 2)
    case("tail_7_11+13", train(T1, T2, 7, head=[("T", 90 * B1, 90)], tail=TAIL), TRAIN, 2)
    case("unfused_17_11+13", train(T1, T2, 17, head=[("T", 90 * B1, 90)]), ANY, 2, fuse=False)
    # B1 in the refocusing pulse as well, on an axis of its own: the relaxations fold at run time and the first shift closes the
    # excitation's record, so the first echo is a record of its own shape, which has no body -- no train
    case("b1_refocus_17_11+13", ow.mse_tuples(T1, T2, B1=B1, necho=17), ANY, 2)
    alpha, TR = sq.mrf_trains(70)
    case("mrf_40_11+13", ow.mrf_tuples(T1, T2, B1, alpha[:40], TR[:40]), ANY, 2)                    # folded run
    # 7 x 19, three index spaces: B1 in the excitation along the first axis, a relaxation along the second behind it
    T1, T2, B1 = g["7x19"]
    head3 = [("T", 90 * B1, 90), ("E", 0.1, 1200.0, T2, 0.1), ("T", 15, 40)]
    for n in (17, 20):
        case(f"train_{n}_7x19", train(T1, T2, n, head=head3), TRAIN, 4)
    case("tail_8_7x19", train(T1, T2, 8, head=head3, tail=TAIL), TRAIN, 4)
    case("unfused_17_7x19", train(T1, T2, 17, head=head3), ANY, 4, fuse=False)
    # no index space: every voxel shares every table
    for n in (17, 20):
        case(f"train_{n}_shared", ow.mse_tuples(1100.0, 60.0, necho=n), TRAIN, 0, shape=(131,))
    case("unfused_17_shared", ow.mse_tuples(1100.0, 60.0, necho=17), ANY, 0, shape=(131,), fuse=False)


_define()

# every (kernel, NSP) pair that epgx_launch_rows_grow can reach: three kernels, four translation units each.  A pair that no
# case names is listed here with the reason why no Python entry reaches it (none: a plan whose voxels share every table has
# n_spaces == 0 -- Encoder._space_of gives a table without a varying axis the space -1 -- and choose_kernel makes it a growing
# launch like any other)
UNREACHABLE = {}
SUB_CASES = ("train_20_131", "train_20_11x13", "train_17_11+13", "unfused_17_131")
SUBRANGES = ((37, 70), (64, 64))        # from mid-wave into a ragged second block; one whole block that is not block 0
PREFILL = 7.0 + 7.0j
# name -> (the small case it tiles, the big grid, the variant line it must trace with no knob set)
THRESHOLD = {
    "thr_train": ("train_20_11x13", (1024, 512), ODD),
    "thr_odd_lead": ("odd_lead_20_11x13", (1024, 512), TRAIN),
    "thr_unfused": ("unfused_20_11x13", (1024, 512), ANY),
    "thr_below": ("train_20_131", (LANES_MIN_VOXELS - 1,), "rows"),
}


def kernel_on(c, side):
    """the kernel a case's launch runs on a side: TRAIN / ANY / ODD, or "rows" """
    if side == "default":
        return "rows"
    if side in ("train_off", "body_off"):
        return ANY
    if side == "odd" and c["odd"]:
        return ODD
    return c["kernel"]


def variant_line(kernel, L):
    """the start of the launcher's variant line (epgx_launch_grow.h)"""
    if kernel == ODD:
        return f"[epgx] run: variant lanes-odd (one voxel per lane, odd orders only): L = {L}, kernel rows_grow_lanes_kernel_odd (12 cells of 2 orders),"
    if kernel == "rows":
        return "[epgx] run: variant rows (four voxels per wave): fewer voxels than the one-voxel-per-lane variant is taken for"
    return f"[epgx] run: variant lanes (one voxel per lane): L = {L}, kernel {kernel} (deck {DECK[kernel]}),"


def family_line(nsp):
    return f"[epgx] run: rows_grow_kernel<{nsp}> -- "


def check_trace(trace, kernel, L, nsp):
    """exactly one launch, of the family, on the variant and kernel expected"""
    lines = trace.splitlines()
    fam = [ln for ln in lines if ln.startswith("[epgx] run: ") and " -- " in ln]
    var = [ln for ln in lines if ln.startswith("[epgx] run: variant ")]
    assert len(fam) == 1 and fam[0].startswith(family_line(nsp)), (fam, family_line(nsp))
    assert len(var) == 1 and var[0].startswith(variant_line(kernel, L)), (var, variant_line(kernel, L))


RATIO = {}           # kernel -> largest per-record error over the case's floor that check_case has seen


def check_case(kernel, name, got, want):
    """the per-record check of a case's signals on one kernel; a case whose reference is identically zero (floor 0): exact zeros"""
    from tests.signal_recurrence import record_errors
    floor = FLOORS[name]
    got, want = np.asarray(got), np.asarray(want)
    if floor == 0.0:
        assert not want.any(), name
        assert got.shape == want.shape and not got.any(), (name, "a record of zeros in the reference is not exactly zero")
        return
    worst = max(record_errors(got, want))
    print(kernel, name, "largest per-record error", float(f"{worst:.3g}"), "=", float(f"{worst / floor:.3g}"), "floors")
    RATIO[kernel] = max(RATIO.get(kernel, 0.0), worst / floor)
    check_records(kernel, got, want, floor)


def check_tiling(big, small):
    """voxels do not interact and no lanes kernel does cross-lane arithmetic: column (i, j, ..) of a launch over a grid whose
    parameter axes are those of `small` tiled must be the bits of column (i mod a, j mod b, ..) of `small`"""
    big, small = np.asarray(big), np.asarray(small)
    assert big.ndim == small.ndim and big.shape[0] == small.shape[0], (big.shape, small.shape)
    want = small
    for ax in range(1, small.ndim):
        want = np.take(want, np.arange(big.shape[ax]) % small.shape[ax], axis=ax)
    assert want.shape == big.shape
    assert np.array_equal(big, want), ("columns differ from the tiled small launch", int(np.sum(big != want)))


def check_subrange(buf, full, vox0, nvox):
    """buf [record, nvox_total]: the columns of the range are the bits of the full launch, every other element is PREFILL"""
    buf, full = np.asarray(buf), np.asarray(full).reshape(np.shape(full)[0], -1)
    assert buf.shape == full.shape, (buf.shape, full.shape)
    assert np.array_equal(buf[:, vox0:vox0 + nvox], full[:, vox0:vox0 + nvox]), "columns of the range differ from the full launch"
    outside = np.ones(buf.shape[1], dtype=bool)
    outside[vox0:vox0 + nvox] = False
    assert np.all(buf[:, outside] == PREFILL), "an element outside the range was written"


def reference(name, oracle=False):
    """records [record, *grid] of a case in extended precision (oracle: the float64 oracle's)"""
    from tests.signal_recurrence import signal_recurrence, oracle_signal
    c = CASES[name]
    return (oracle_signal if oracle else signal_recurrence)(c["tuples"], shape=grid_of_case(c), max_nstate=63)


def tiled_tuples(name, big):
    """the tuples of a small case with every parameter array tiled along its own axes up to the grid `big`"""
    c = CASES[name]
    small = grid_of_case(c)
    made = {}

    def grow(x):
        if not isinstance(x, np.ndarray):
            return x
        for ax, n in enumerate(x.shape):
            if n > 1:
                assert n == small[ax]
                x = np.take(x, np.arange(big[ax]) % n, axis=ax)
        return x

    out = []
    for t in c["tuples"]:
        if id(t) not in made:
            made[id(t)] = tuple(grow(x) for x in t)
        out.append(made[id(t)])
    return out


# ------------------------------------------------------------------------------------------------ the child process
def _plan(tuples, grid, fuse):
    from epgpy_amd import _lib, functions as _functions
    from tests.signal_cases import ops_of
    enc, _, _ = _functions.compile_sequence(ops_of(tuples), shape=grid, options={"max_nstate": 63}, fuse=fuse)
    assert enc.grid == tuple(grid) and 32 < enc.peak + 1 <= 64, (enc.grid, enc.peak)
    ctx = _lib.get_context(0)
    return ctx, enc, enc.device_plan(ctx, 64)


def run_subrange(name, vox0, nvox):
    """[record, nvox_total]: the buffer after ONE launch of the voxels [vox0, vox0 + nvox), prefilled with PREFILL"""
    from epgpy_amd import _lib
    c = CASES[name]
    ctx, enc, plan = _plan(c["tuples"], grid_of_case(c), c["fuse"])
    total = enc.nvox
    assert 0 <= vox0 and vox0 + nvox <= total
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * total)
    sig.upload(np.full((enc.n_adc, total), PREFILL, dtype=np.complex128))
    _lib.run(ctx, plan, 0, plan.n_ops, vox0, nvox, None, None, 64, sig.ptr.value, total, vox0)
    out = sig.download(np.complex128, (enc.n_adc, total))
    sig.free()
    return out


def run_threshold(name):
    """[record, *big grid]: ONE launch of the whole big grid"""
    from epgpy_amd import _lib
    small, big, _ = THRESHOLD[name]
    ctx, enc, plan = _plan(tiled_tuples(small, big), big, CASES[small]["fuse"])
    nbytes = 16 * enc.n_adc * enc.nvox
    assert nbytes <= 170e6, nbytes
    sig = _lib.DeviceBuffer(ctx, nbytes)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, enc.nvox, None, None, 64, sig.ptr.value, enc.nvox, 0)
    out = sig.download(np.complex128, (enc.n_adc,) + tuple(big))
    sig.free()
    del plan
    ctx.release_cache()
    return out


def run_all(out_path):
    from epgpy_amd import epg
    from tests.signal_cases import ops_of

    def mark(name):
        print(f"[case] {name}", file=sys.stderr, flush=True)       # (with EPGX_TRACE: the library's lines of this launch follow)

    res = {}
    for name, c in CASES.items():
        mark(name)
        kw = {"shape": c["shape"]} if c["shape"] is not None else {}
        res[name] = np.asarray(epg.simulate(ops_of(c["tuples"]), max_nstate=63, fuse=c["fuse"], **kw))
    if os.environ.get("EPGX_PATHS_SUBRANGE") == "1":
        for name in SUB_CASES:
            for vox0, nvox in SUBRANGES:
                mark(f"sub_{vox0}_{nvox}:{name}")
                res[f"sub_{vox0}_{nvox}:{name}"] = run_subrange(name, vox0, nvox)
    np.savez(out_path, **res)
    if os.environ.get("EPGX_PATHS_THRESHOLD") == "1":
        for name in THRESHOLD:
            mark(name)
            np.save(f"{out_path}.{name}.npy", run_threshold(name))


if __name__ == "__main__":
    from tests import lanes_path_cases as me            # (the module under its package name: one CASES table)

    me.run_all(sys.argv[1])
