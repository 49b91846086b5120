"""The derivative cases that tests/test_gpu_jacobian_paths.py runs on the device and tests/test_jacobian_recurrence_host.py
measures on the CPU -- oracle tuples, the variables of the plan, the capacity and the kernel name each case must get from
choose_kernel (csrc/epgx_planner.cpp) -- and the per-column check both use:

    err_v = max|got[..., v] - ref[..., v]| / max|ref[..., v]|   <=   16 x the case's float64 floor   (never above 1e-11)

The columns of a Jacobian differ by five orders of magnitude; a bound scaled by the whole array hides an error in a small one.
Groups: (a) deriv_kernel<M, NSP, V, CONTIG> from equilibrium, (b) deriv_kernel from a state input, (c) packed_deriv_kernel,
(d) rows_deriv_kernel, (e) drun_kernel, (f) packed_dfold_kernel, (g) passes of simulate() and probes."""
import numpy as np

from epgpy_amd import epg
from tests.jacobian_recurrence import column_errors

MARGIN = 16            # four bits over the float64 floor: re-association of fused E . T . E tables, run-time fold, sum / difference cell
CAP = 1e-11            # no case may need more per column
DRUN_FOLD, DRUN_LOGD = 128, 256
MEASURED = {}          # group -> largest per-column error seen

# float64 floors: max over columns of max|oracle - recurrence| / max|column| of every case, measured on the CPU by
# tests/test_jacobian_recurrence_host.py and rounded
# up by half (the oracle's libm may differ in the last bit from one machine to the next).  16 x a floor may not exceed 1e-11: a case
# that needs more is ill-conditioned for that column, and its inputs change -- not the cap.
FLOORS = {
    "jac_mse": 2.4e-15, "jac_long": 5.4e-15, "jac_spgr": 1.1e-14, "jac_params": 4.1e-16, "jac_plain_ops": 3.4e-16,
    "jac_plain_ops_exact": 3.4e-16, "a_128_1_1": 7.4e-15, "a_128_1_1_top": 7.4e-15, "a_128_2_2": 1.2e-14,
    "a_128_2_2_top": 1.2e-14, "a_128_3_3": 1.4e-14, "a_128_3_3_top": 1.4e-14, "a_256_1_3": 1.3e-14, "a_256_1_3_top": 1.3e-14,
    "a_256_2_1": 8.9e-15, "a_256_2_1_top": 8.9e-15, "a_256_3_2": 1.4e-14, "a_256_3_2_top": 1.4e-14, "a_512_1_2": 2.5e-15,
    "a_512_1_2_top": 2.5e-15, "a_512_2_3": 6.3e-15, "a_512_2_3_top": 6.3e-15, "a_512_3_1": 1.1e-14, "a_512_3_1_top": 1.1e-14,
    "a_1024_1_1": 2.7e-15, "a_1024_1_1_top": 2.7e-15, "a_256_3_seam191": 1.2e-14, "a_256_3_seam193": 1.2e-14,
    "a_256_2_seam199": 7.5e-15, "a_256_2_seam200": 7.5e-15, "a_128_lds": 4.5e-15, "a_512_lds": 9.2e-15, "b_64_1_1": 2.5e-15,
    "b_64_2_2": 1.6e-15, "b_64_3_3": 2.0e-15, "b_128_2_1": 1.4e-15, "b_128_3_2": 3.2e-15, "b_256_1_2": 1.2e-15,
    "b_256_3_1": 1.6e-15, "b_1024_1_1": 1.4e-15, "c_10_1_1": 1.2e-15, "c_15_2_2": 1.3e-15, "c_10_3_3": 2.4e-15,
    "c_20_1_2": 1.2e-15, "c_31_2_3": 2.3e-15, "c_20_3_1": 2.8e-15, "c_15_3_1": 2.2e-15, "c_31_1_1": 1.2e-15, "d_x": 3.4e-15,
    "d_y": 1.4e-15, "d_axis": 1.7e-15, "d_x70": 2.4e-15, "d_axis_b1": 2.7e-15, "e_echo_5": 1.5e-15, "e_echo_12": 3.7e-15,
    "e_echo_20": 5.7e-15, "e_echo_40": 4.3e-15, "e_echo_25": 3.0e-15, "e_echo_logd": 6.0e-15, "e_fold_1": 3.2e-15,
    "e_fold_2": 3.2e-15, "e_fold_3": 3.2e-15, "f_10_1": 1.6e-15, "f_10_2": 1.6e-15, "f_10_3": 2.9e-15, "f_20_1": 1.9e-15,
    "f_20_2": 1.9e-15, "f_20_3": 2.7e-15, "f_spoiled_1": 6.3e-16, "f_spoiled_3": 7.2e-16, "g_passes_4": 8.4e-15,
    "g_passes_5": 1.1e-14, "g_passes_1024": 2.2e-15, "g_probes": 9.7e-16,
    "a_512_3_seam319": 1.2e-14, "a_512_3_seam321": 1.2e-14, "a_128_2_seam99": 1.2e-14, "a_128_2_seam100": 1.2e-14,
    "a_512_2_seam399": 7.5e-15, "a_512_2_seam400": 7.5e-15, "a_128_diffusion": 4.5e-15, "d_v2_x": 2.7e-15, "d_v2_y": 1.5e-15,
    "d_v2_axis": 1.9e-15, "d_v2_x70": 3.5e-15, "d_spoiled_1": 6.7e-16, "d_spoiled_2": 1.2e-15,
    "a_1024_1_seam799": 7.5e-15, "a_1024_1_seam800": 7.5e-15,
}


def floor_of(name):
    return FLOORS[name]


def check(group, got, want, floor=None):
    """per column: err_v = max|got[..., v] - want[..., v]| / max|want[..., v]| (column 0, the signal: / max(1, max|want|));
    a column whose reference is identically zero must be exactly zero.  `floor`: the case's float64 floor (bound 16 x);
    None asks for the cap of every case, 1e-11"""
    errs = column_errors(got, want)
    MEASURED[group] = max(MEASURED.get(group, 0.0), max(errs))
    bound = CAP if floor is None else MARGIN * floor
    assert bound <= CAP, (group, bound)
    print(group, "per-column errors", [float(f"{e:.3g}") for e in errs], "bound", bound)
    assert max(errs) <= bound, (group, errs, bound)
    return errs


# ------------------------------------------------------------------------------------------------ sequences (oracle tuples)
def tissue(nsp, seed, n=13):
    """(T1, T2, B1, extra records per echo): 1 index space -- per-voxel tables on one axis; 2 -- (T1, T2) on one axis, B1 on
    another; 3 (kernels' NSP = 4) -- three axes and a relaxation over the middle one alone"""
    rng = np.random.default_rng(seed)
    if nsp == 1:
        return rng.uniform(300, 2000, n), rng.uniform(60, 200, n), rng.uniform(0.8, 1.2, n), []
    if nsp == 2:
        return rng.uniform(300, 2000, (3, 1)), rng.uniform(60, 200, (3, 1)), rng.uniform(0.8, 1.2, (1, 3)), []
    if n <= 9:        # long trains: two axes, (T1, T2) dense, B1 along the first, the extra relaxation along the second -- 9 voxels
        T2 = rng.uniform(60, 200, (1, 3))
        extra = [("E", 0.3, 1200.0, T2, 0, {"order1": {"T2": {"T2": 1}}})]
        return rng.uniform(300, 2000, (3, 1)), T2, rng.uniform(0.8, 1.2, (3, 1)), extra
    a, b, c = 3, 3, 2
    T2 = rng.uniform(60, 200, (1, b, 1))
    extra = [("E", 0.3, 1200.0, T2[:, :, 0], 0, {"order1": {"T2": {"T2": 1}}})]
    return rng.uniform(300, 2000, (a, 1, 1)), T2, rng.uniform(0.8, 1.2, (1, 1, c)), extra


RL = {"T1": {"T1": 1}, "T2": {"T2": 1}, "tau": {"tau": 1}}
TRAIN_VARS = ["T1", "T2", "B1", "fa", "tau"]


def echo_train(T1, T2, B1, extra, necho, step=1, big=0, tau=2.5, alpha=150.0):
    """the g16 train: 90 degree excitation, then [S E T S E ADC] x necho with partials w.r.t. T1 / T2 / tau (relaxation), B1 and
    the refocusing angle; `step`: the shift per half echo; `big`: one S(-big) T S(+big) detour half way"""
    exc = ("T", 90 * B1, 90, {"order1": {"B1": {"alpha": 90}}})
    rfc = ("T", alpha * B1, 0, {"order1": {"B1": {"alpha": alpha}, "fa": {"alpha": 1.0}}})
    rlx = ("E", tau, T1, T2, 0, {"order1": RL})
    sh, adc = ("S", step), ("ADC",)
    echo = [sh, rlx, rfc, sh, rlx] + extra + [adc]
    seq = [exc] + echo * (necho // 2)
    if big:
        seq += [("S", -big), rfc, ("S", big)]
    return seq + echo * (necho - necho // 2)


def gre_train(T2, g, B1, extra, nrep, phi_step=58.5, phi0=None, plain=()):
    """RF-spoiled gradient echo with off-resonance (complex partials g, phi; nothing to fuse or fold): [T E ADC E S] x nrep,
    an S(-1) and the records of `plain` (SPOILER / RESET / PD ..) half way"""
    rl = ("E", 5.0, 1000.0, T2, g, {"order1": {"g": {"g": 1}, "T2": {"T2": 1}}})
    seq = []
    for i in range(nrep):
        ph = phi0 if phi0 is not None else float(phi_step * i * i % 360)
        seq += [("T", 14.8 * B1, ph, {"order1": {"phi0": {"phi": 1}, "fa": {"alpha": 1}, "B1": {"alpha": 14.8}}}), rl, ("ADC",), rl] + extra + [("S", 1)]
        if i == nrep // 2:
            seq += [("S", -1)] + list(plain)
    return seq + [("ADC",), ("ADC", "Z0")]


def gre_tissue(nsp, seed, n=9):
    rng = np.random.default_rng(seed)
    if nsp == 1:
        return rng.uniform(30, 120, n), rng.uniform(-0.03, 0.03, n), rng.uniform(0.8, 1.2, n), []
    if nsp == 2:
        return rng.uniform(30, 120, (3, 1)), rng.uniform(-0.03, 0.03, (3, 1)), rng.uniform(0.8, 1.2, (1, 3)), []
    g = rng.uniform(-0.03, 0.03, (1, 3, 1))
    return rng.uniform(30, 120, (3, 1, 1)), g, rng.uniform(0.8, 1.2, (1, 1, 2)), [("P", 0.5, g[:, :, 0])]


def mrf_train(T1, T2, B1, ntr, seed, spoiled=False, phi=90.0):
    """repetitions [T(a_n B1) E(TE) ADC E(TR_n - TE) S] over a (T1, T2) x B1 grid: a rotation over one index space between
    relaxations over another, folded by the library at run time; `spoiled`: a perfect spoiler instead of the shift"""
    rng = np.random.default_rng(seed)
    rl = {"T1": {"T1": 1}, "T2": {"T2": 1}}
    seq = [("T", 180 * B1, 90, {"order1": {"B1": {"alpha": 180.0}}}), ("E", 20.0, T1, T2, 0, {"order1": rl})]
    e_te = ("E", 3.0, T1, T2, 0, {"order1": rl})
    for a, tr in zip(rng.uniform(10, 60, ntr), rng.uniform(11, 16, ntr)):
        seq += [("T", float(a) * B1, phi, {"order1": {"B1": {"alpha": float(a)}}}), e_te, ("ADC",),
                ("E", float(tr) - 3.0, T1, T2, 0, {"order1": rl}), ("SPOILER",) if spoiled else ("S", 1)]
    return seq


def ops_of(tuples):
    """oracle tuples -> product operators; one operator object per tuple object (echo trains repeat theirs)"""
    made, ops = {}, []
    for t in tuples:
        if id(t) not in made:
            kind, o1 = t[0], (t[-1]["order1"] if isinstance(t[-1], dict) else False)
            args = t[1:-1] if isinstance(t[-1], dict) else t[1:]
            if kind == "T":
                op = epg.T(args[0], args[1], order1=o1)
            elif kind == "E":
                op = epg.E(*args, order1=o1)
            elif kind == "P":
                op = epg.P(*args, order1=o1)
            elif kind == "R":
                op = epg.R(args[0], args[1], r0=args[2], order1=o1)
            elif kind == "S":
                op = epg.S(args[0])
            elif kind == "D":
                op = epg.D(args[0], args[1])
            elif kind == "ADC":
                op = epg.ADC if len(args) == 0 or args[0] == "F0" else epg.Adc(args[0])
            elif kind == "PD":
                op = epg.PD(args[0], reset=(len(args) < 2 or args[1]))
            else:
                op = {"SPOILER": epg.SPOILER, "RESET": epg.RESET}[kind]
            made[id(t)] = op
        ops.append(made[id(t)])
    return ops


PREFIX_T2 = 90.0


def prefix(K):
    """operators that prepare a start state with orders in the upper half of capacity K (no partials)"""
    return [("T", 35.0, 10.0), ("S", 1), ("E", 3.0, 800.0, PREFIX_T2, 0), ("T", 50.0, 0.0), ("S", K // 2), ("T", 70.0, 40.0), ("S", 3),
            ("E", 2.0, 800.0, PREFIX_T2, 0)]


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def case(name, group, tuples, variables, kernel, K, *, cap=None, exact=False, probe="F0", head=None, packed=True, kvalue=None):
    assert name not in CASES, name
    CASES[name] = dict(group=group, tuples=tuples, variables=list(variables), kernel=kernel, K=K, cap=cap, exact=exact,
                       probe=probe, head=head, packed=packed, kvalue=kvalue)


def deriv_name(K, nsp, V, contig):
    return f"deriv_kernel<{K // 64}, {4 if nsp > 2 else nsp}, {V}{', true' if contig else ''}>"


def _define():
    # (a) deriv_kernel from equilibrium: (K, V, index spaces, contiguous layout); unbounded trains of K / 2 - 2 echoes fill the
    # orders up to K - 4, trains of K / 2 + 3 echoes truncated at K - 2 act in the top register
    for K, V, nsp, contig in [(128, 1, 1, True), (128, 2, 2, True), (128, 3, 3, True), (256, 1, 3, True), (256, 2, 1, True),
                              (256, 3, 2, False), (512, 1, 2, True), (512, 2, 3, True), (512, 3, 1, False), (1024, 1, 1, True)]:
        T1, T2, B1, extra = tissue(nsp, K + V, n=5 if K == 1024 else (9 if K >= 256 else 13))
        var = TRAIN_VARS[(K // 128 + V) % 3:][:V]
        case(f"a_{K}_{V}_{nsp}", "a", echo_train(T1, T2, B1, extra, K // 2 - 2), var, deriv_name(K, nsp, V, contig), K)
        case(f"a_{K}_{V}_{nsp}_top", "a", echo_train(T1, T2, B1, extra, K // 2 + 3), var, deriv_name(K, nsp, V, contig), K, cap=K - 2)
    # truncation on either side of a seam: strided, register m holds orders 64 m .. 64 m + 63; contiguous, lane l orders 4 l .. 4 l + 3
    T1, T2, B1, extra = tissue(1, 77, n=9)
    for cap in (191, 193):
        case(f"a_256_3_seam{cap}", "a", echo_train(T1, T2, B1, extra, 104), ["T1", "T2", "B1"], deriv_name(256, 1, 3, False), 256, cap=cap)
    for cap in (199, 200):
        case(f"a_256_2_seam{cap}", "a", echo_train(T1, T2, B1, extra, 104), ["T2", "fa"], deriv_name(256, 1, 2, True), 256, cap=cap)
    for cap in (319, 321):       # strided, M = 8
        case(f"a_512_3_seam{cap}", "a", echo_train(T1, T2, B1, extra, 170), ["T1", "T2", "B1"], deriv_name(512, 1, 3, False), 512, cap=cap)
    for cap in (99, 100):        # contiguous, M = 2: lane l holds orders 2 l, 2 l + 1
        case(f"a_128_2_seam{cap}", "a", echo_train(T1, T2, B1, extra, 56), ["T1", "B1"], deriv_name(128, 1, 2, True), 128, cap=cap)
    for cap in (399, 400):       # contiguous, M = 8: lane l holds orders 8 l .. 8 l + 7
        case(f"a_512_2_seam{cap}", "a", echo_train(T1, T2, B1, extra, 206), ["T2", "fa"], deriv_name(512, 1, 2, True), 512, cap=cap)
    for cap in (799, 800):       # contiguous, M = 16: lane l holds orders 16 l .. 16 l + 15 (one derivative state, five voxels)
        case(f"a_1024_1_seam{cap}", "a", echo_train(T1[:5], T2[:5], B1[:5], extra, 406), ["T2"], deriv_name(1024, 1, 1, True), 1024, cap=cap)
    # 1-D diffusion between the pulses, acting on the derivative states too (exact_partials): the strided layout
    case("a_128_diffusion", "a", echo_train(T1, T2, B1, [("D", 0.5, 1e-3)], 60), ["T2", "B1"], deriv_name(128, 1, 2, False), 128, exact=True,
         kvalue=3e3)
    # shifts by two and long shifts: the strided layout, staged through LDS
    case("a_128_lds", "a", echo_train(T1, T2, B1, extra, 20, step=2, big=17), ["T1", "B1"], deriv_name(128, 1, 2, False), 128)
    T1, T2, B1, extra = tissue(2, 78)
    case("a_512_lds", "a", echo_train(T1, T2, B1, extra, 100, step=2, big=50), ["T2", "B1", "fa"], deriv_name(512, 2, 3, False), 512)
    # (b) from a state input: K = 64 goes to deriv_kernel<1, ..> with every number of index spaces
    for K, V, nsp, contig in [(64, 1, 1, False), (64, 2, 2, False), (64, 3, 3, False), (128, 2, 1, True), (128, 3, 2, True),
                              (256, 1, 2, True), (256, 3, 1, False), (1024, 1, 1, True)]:
        T1, T2, B1, extra = tissue(nsp, 900 + K + V, n=5 if K == 1024 else 13)
        var = TRAIN_VARS[(K // 64 + V) % 3:][:V]
        case(f"b_{K}_{V}_{nsp}", "b", echo_train(T1, T2, B1, extra, 6), var, deriv_name(K, nsp, V, contig), K, head=prefix(K))
    # (c) packed_deriv_kernel: 16 / 32 orders, S(-1), spoilers and resets through the generic record; 9 and 70 voxels
    gvars = ["g", "T2", "phi0"]
    for cap, V, nsp, n in [(10, 1, 1, 9), (15, 2, 2, 9), (10, 3, 3, 9), (20, 1, 2, 9), (31, 2, 3, 9), (20, 3, 1, 70), (15, 3, 1, 70),
                           (31, 1, 1, 9)]:
        T2, g, B1, extra = gre_tissue(nsp, 300 + cap + V, n)
        KP = 16 if cap <= 15 else 32
        case(f"c_{cap}_{V}_{nsp}", "c", gre_train(T2, g, B1, extra, 36, plain=[("SPOILER",), ("ADC",), ("RESET",)]), gvars[3 - V:] if V < 3 else gvars,
             f"packed_deriv_kernel<{4 if nsp > 2 else nsp}, {V}, {KP}>", KP, cap=cap)
    # (d) rows_deriv_kernel: 64 orders (47 before the reset, truncated at 50), one derivative state; rotations about x, y and a general axis; both semantics of plain operators
    stops = [("SPOILER",), ("ADC",), ("PD", 0.7, False), ("T", 20.0, 30.0, {"order1": {"fa": {"alpha": 1}}}), ("ADC",), ("RESET",)]
    for tag, nsp, n, phi0, var, exact in [("x", 1, 9, 0.0, "g", False), ("y", 2, 9, 90.0, "T2", True), ("axis", 3, 9, None, "phi0", False),
                                          ("x70", 1, 70, 0.0, "fa", True), ("axis_b1", 3, 9, 37.0, "B1", True)]:
        T2, g, B1, extra = gre_tissue(nsp, 400 + n + nsp, n)
        case(f"d_{tag}", "d", gre_train(T2, g, B1, extra, 90, phi0=phi0, plain=stops), [var], f"rows_deriv_kernel<{4 if nsp > 2 else nsp}, 4, 1>", 64,
             cap=50, exact=exact)
    for tag, nsp, n, phi0, var, exact in [("v2_x", 1, 9, 0.0, ["g", "T2"], False), ("v2_y", 2, 9, 90.0, ["phi0", "fa"], True),
                                          ("v2_axis", 3, 9, None, ["g", "phi0"], False), ("v2_x70", 1, 70, 0.0, ["T2", "B1"], True)]:
        T2, g, B1, extra = gre_tissue(nsp, 450 + n + nsp, n)
        case(f"d_{tag}", "d", gre_train(T2, g, B1, extra, 90, phi0=phi0, plain=stops), var, f"rows_deriv_kernel<{4 if nsp > 2 else nsp}, 4, 2>", 64,
             cap=50, exact=exact)
    # (e) drun_kernel: fused echoes ending in each growth phase (R = 1, 2, 4: fewer than 8 echoes, 8 - 15, 16 or more) and truncated
    T1, T2, B1, extra = tissue(1, 500, n=13)
    # (relaxation partials of fused echoes take the logarithmic form, DRUN_LOGD; a plan with the B1 partial alone has none)
    for necho, var in [(5, ["T2"]), (12, ["T1", "T2"]), (20, ["T1", "T2", "B1"]), (40, ["B1", "T2"]), (25, ["B1"])]:
        case(f"e_echo_{necho}", "e", echo_train(T1, T2, B1, extra, necho, tau=5.0, alpha=120.0), var,
             ("drun", len(var), 0, False, var != ["B1"]), 64, cap=63, packed=False)
    case("e_echo_logd", "e", echo_train(T1, T2, B1, extra, 34, tau=5.0, alpha=120.0), ["T1", "T2"], ("drun", 2, 0, False, True), 64, cap=63, packed=False)
    T1, T2, B1, _ = tissue(2, 501)
    for V in (1, 2, 3):
        var = ["T2", "B1", "T1"][:V]
        case(f"e_fold_{V}", "e", mrf_train(T1, T2, B1, 45, 7), var, ("drun", V, 0, True, False) if V < 3 else ("split",), 64, cap=63, packed=False)
    # the spoiled repetitions at 64 orders: the library folds a spoiler into a repetition at 16 / 32 orders only (packed_dfold_kernel,
    # below), so at 64 orders the train runs record by record on rows_deriv_kernel -- pinned, so that a fold added there shows up here
    for V, exact in ((1, True), (2, False)):
        case(f"d_spoiled_{V}", "d", mrf_train(T1, T2, B1, 14, 9, spoiled=True, phi=58.5), ["T1", "B1"][:V], f"rows_deriv_kernel<2, 4, {V}>", 64,
             exact=exact, packed=False)
    # (f) packed_dfold_kernel: the folded repetitions at 16 / 32 orders, spoiled and unspoiled
    for cap, KP in ((10, 16), (20, 32)):
        for V in (1, 2, 3):
            var = ["T1", "B1", "T2"][:V]
            case(f"f_{cap}_{V}", "f", mrf_train(T1, T2, B1, 30, 8), var, f"packed_dfold_kernel<{V}, {KP}>", KP, cap=cap)
    for V, exact in ((1, False), (3, True)):
        case(f"f_spoiled_{V}", "f", mrf_train(T1, T2, B1, 14, 9, spoiled=True, phi=58.5), ["T1", "T2", "B1"][:V], f"packed_dfold_kernel<{V}, 16>", 16,
             exact=exact)


_define()


def full_tuples(c):
    return (c["head"] or []) + c["tuples"]


def options_of(c):
    return {**({"max_nstate": c["cap"]} if c["cap"] else {}), **({"kvalue": c["kvalue"]} if c["kvalue"] else {})}


def g_cases():
    """name -> (tuples, variables, options) of the simulate() cases below (their floors: FLOORS, by the same names)"""
    out = {}
    for nvar in (4, 5):
        T1, T2, B1, extra = tissue(1, 600 + nvar, n=5)
        out[f"g_passes_{nvar}"] = (echo_train(T1, T2, B1, extra, 150), TRAIN_VARS[:nvar], {})
    T1, T2, B1, extra = tissue(1, 610, n=3)
    out["g_passes_1024"] = (echo_train(T1, T2, B1, extra, 300), ["T2", "B1"], {})
    T2, g, B1, extra = gre_tissue(2, 620)
    out["g_probes"] = (gre_train(T2, g, B1, extra, 12), ["T2", "zzz", "g"], {"max_nstate": 20})
    return out
