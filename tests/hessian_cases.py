"""The second-order cases that tests/test_gpu_hessian_paths.py runs on the device and tests/test_hessian_recurrence_host.py
measures on the CPU: oracle tuples (trailing dict with "order1" / "order2"), the variable pair of the pass, the capacity and
the kernel name the pass must get from choose_kernel -- and the per-column check both use (tests/jacobian_cases.py):

    err_v = max|got[..., v] - ref[..., v]| / max|ref[..., v]|   <=   16 x the case's float64 floor   (never above 1e-11)

over the rows of a pass: S, S_a, (S_b,) H_ab."""
import numpy as np

from epgpy_amd import epg
from tests.jacobian_cases import CAP, MARGIN, tissue
from tests.jacobian_recurrence import column_errors

# float64 floors: max over the rows of a pass of max|f64 recurrence - longdouble recurrence| / max|row| (the state row: / max(1,
# max|row|)), measured on the CPU by tests/test_hessian_recurrence_host.py and rounded up by half.  16 x a floor may not exceed
# 1e-11: a case that needs more gets other inputs, not a wider cap.
FLOORS = {
    "h_64_diag": 2.9e-14, "h_64_diag_top": 3.4e-14, "h_64_pair": 1.0e-14, "h_64_pair_top": 1.1e-14,
    "h_128_diag": 5.2e-15, "h_128_diag_top": 5.4e-15, "h_128_pair": 6.4e-15, "h_128_pair_top": 6.4e-15,
    "h_256_diag": 3.2e-14, "h_256_diag_top": 3.2e-14, "h_256_pair": 8.1e-14, "h_256_pair_top": 8.1e-14,
    "h_512_diag": 6.3e-15, "h_512_diag_top": 6.3e-15, "h_512_pair": 6.8e-15, "h_512_pair_top": 6.8e-15,
    "h_512_pair_nsp3": 6.3e-15, "h_512_pair_nsp0": 1.7e-14,
    "h_select": 1.8e-15, "h_plain": 6.9e-16, "h_plain_exact": 5.4e-16, "h_z0": 1.5e-15, "h_coeff": 1.4e-15,
    # the G13 sequences (tests/sequences.py::hessian_cases): per entry column of their Hessian probes
    "g13_tutorial": 1.5e-15, "g13_grid": 9.2e-16,
}


def check(name, got, want, floor=None):
    """per row of a pass (jacobian_cases.check): 16 x floor; a row whose reference is identically zero must be exactly zero"""
    errs = column_errors(got, want)
    bound = CAP if floor is None else MARGIN * floor
    assert bound <= CAP, (name, bound)
    print(name, "per-row errors", [float(f"{e:.3g}") for e in errs], "bound", bound)
    assert max(errs) <= bound, (name, errs, bound)
    return errs


# ------------------------------------------------------------------------------------------------ sequences (oracle tuples)
def echo_train2(T1, T2, B1, extra, necho, tau=2.5, alpha=150.0):
    """the echo train of jacobian_cases with second-order declarations: 90 degree excitation, [S E T S E ADC] x necho;
    variables T2 (relaxation), B1 (both pulses) and fa (refocusing angle), every pair among them"""
    exc = ("T", 90 * B1, 90, {"order1": {"B1": {"alpha": 90}}, "order2": [("B1", "B1")]})
    rfc = ("T", alpha * B1, 0, {"order1": {"B1": {"alpha": alpha}, "fa": {"alpha": 1.0}},
                                "order2": [("B1", "B1"), ("B1", "fa"), ("fa", "fa"), ("B1", "T2"), ("T2", "fa")]})
    rlx = ("E", tau, T1, T2, 0, {"order1": {"T2": {"T2": 1}}, "order2": [("T2", "T2"), ("B1", "T2"), ("T2", "fa")]})
    sh, adc = ("S", 1), ("ADC",)
    return [exc] + ([sh, rlx, rfc, sh, rlx] + extra + [adc]) * necho


def g13_tuples(name):
    """tests/sequences.py::hessian_cases as oracle tuples: (tuples, simulate options)"""
    if name == "tutorial":
        inv = ("T", 150, 0, {"order2": "alpha"})
        rlx = ("E", 4.5, 1400, 30, 0, {"order2": "T2"})
        sh = ("S", 1)
        return [("T", 90, 90)] + [sh, rlx, inv, sh, rlx, ("ADC",)] * 6, {}
    T2 = np.array([40.0, 90.0])
    g = np.array([[0.0, 0.02, -0.01]])
    rf = ("T", 35, 20, {"order1": {"b1": {"alpha": 35.0}, "ph": {"phi": 1.0}}, "order2": [("b1", "b1"), ("b1", "ph"), ("b1", "T2")]})
    rl = ("E", 6, 900, T2, g, {"order1": ["T2", "g"], "order2": [("T2", "T2"), ("T2", "g"), ("b1", "T2")]})
    return [rf, rl, ("ADC",), ("S", 1), rf, ("S", 1), rl, ("ADC",), ("S", -1), rf, rl, ("ADC",)], {"max_nstate": 5}


def ops_of(tuples):
    """oracle tuples -> product operators; one operator object per tuple object"""
    made, ops = {}, []
    for t in tuples:
        if id(t) not in made:
            kind = t[0]
            opts = t[-1] if isinstance(t[-1], dict) else {}
            kw = {k: opts[k] for k in ("order1", "order2") if k in opts}
            args = t[1:-1] if isinstance(t[-1], dict) else t[1:]
            if kind == "T":
                op = epg.T(args[0], args[1], **kw)
            elif kind == "E":
                op = epg.E(*args, **kw)
            elif kind == "P":
                op = epg.P(*args, **kw)
            elif kind == "S":
                op = epg.S(args[0])
            elif kind == "ADC":
                op = epg.ADC if len(args) == 0 or args[0] == "F0" else epg.Adc(args[0])
            else:
                op = {"SPOILER": epg.SPOILER, "RESET": epg.RESET}[kind]
            made[id(t)] = op
        ops.append(made[id(t)])
    return ops


def entry_errors(got, want):
    """per entry (i1, i2) of a Hessian [record, *grid, n1, n2]: max|got - want| / max|want|; an entry whose reference is
    identically zero must be exactly zero (inf otherwise)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    flat = lambda x: x.reshape(x.shape[:-2] + (1, x.shape[-2] * x.shape[-1]))[..., 0, :]
    errs = column_errors(np.concatenate([np.zeros_like(flat(got)[..., :1]), flat(got)], axis=-1),
                         np.concatenate([np.zeros_like(flat(want)[..., :1]), flat(want)], axis=-1))
    return errs[1:]


def hess_name(K, nsp, diag):
    nsp = 4 if nsp > 2 else nsp
    if K == 512 and not diag and nsp == 1:      # (the one instantiation that would need scratch: DESIGN 4.10)
        nsp = 2
    return f"hess_kernel<{K // 64}, {nsp}, {'true' if diag else 'false'}>"


CASES = {}


def case(name, tuples, pair, kernel, K, *, cap=None, exact=False, probe="F0", shape=None):
    assert name not in CASES, name
    CASES[name] = dict(tuples=tuples, pair=tuple(pair), kernel=kernel, K=K, cap=cap, exact=exact, probe=probe, shape=shape)


def _define():
    # every instantiation: K x DIAG, the index spaces 1, 2, 3 (kernels' NSP = 1, 2, 4) spread over them; unbounded trains of
    # K / 2 - 2 echoes fill the orders, trains of K / 2 + 3 echoes truncated at K - 2 act in the top register
    plan = [(64, True, 1, ("fa", "fa")), (64, False, 2, ("B1", "T2")), (128, True, 3, ("T2", "T2")), (128, False, 1, ("T2", "fa")),
            (256, True, 2, ("B1", "B1")), (256, False, 3, ("B1", "fa")), (512, True, 1, ("T2", "T2")), (512, False, 1, ("B1", "T2"))]
    for K, diag, nsp, pair in plan:
        T1, T2, B1, extra = tissue(nsp, 7000 + K + int(diag), n=5 if K == 512 else (9 if K >= 256 or nsp == 3 else 13))
        extra = [e[:-1] for e in extra]           # (the extra relaxation of three index spaces: no partials here)
        tag = f"h_{K}_{'diag' if diag else 'pair'}"
        case(tag, echo_train2(T1, T2, B1, extra, K // 2 - 2), pair, hess_name(K, nsp, diag), K)
        case(tag + "_top", echo_train2(T1, T2, B1, extra, K // 2 + 3), pair, hess_name(K, nsp, diag), K, cap=K - 2)
    # the other K = 512 pair kernels (each at the register file of a whole SIMD): three index spaces, and none -- every voxel of
    # the grid then shares every table (the grid comes from the `shape` option: 5 identical voxels)
    T1, T2, B1, extra = tissue(3, 7513, n=9)
    extra = [e[:-1] for e in extra]
    case("h_512_pair_nsp3", echo_train2(T1, T2, B1, extra, 254), ("T2", "fa"), hess_name(512, 3, False), 512)
    case("h_512_pair_nsp0", echo_train2(900.0, 110.0, 0.93, [], 254), ("B1", "fa"), hess_name(512, 0, False), 512, shape=(5,))
    # term selection: per-operator order2 lists -- the pulse declares (b1, T2), the relaxation does not: the cross term
    # (dE/dT2) S_b1 must be absent, (dT/db1) S_T2 present
    T2 = np.linspace(40.0, 90.0, 7)
    rf = ("T", 35, 20, {"order1": {"b1": {"alpha": 35.0}, "ph": {"phi": 1.0}}, "order2": [("b1", "b1"), ("b1", "ph"), ("b1", "T2")]})
    rl = ("E", 6, 900, T2, 0.01, {"order1": ["T2", "g"], "order2": [("T2", "T2"), ("T2", "g")]})
    seq = [rf, rl, ("ADC",), ("S", 1), rf, ("S", 1), rl, ("ADC",), ("S", -1), rf, rl, ("ADC",)] * 2
    case("h_select", seq, ("T2", "b1"), hess_name(64, 1, False), 64)
    # a coefficient dict on a shared variable, diagonal pair
    case("h_coeff", seq, ("b1", "b1"), hess_name(64, 1, True), 64)
    # Z0 probe
    case("h_z0", seq, ("T2", "g"), hess_name(64, 1, False), 64, probe="Z0")
    # SPOILER and RESET, with and without EPGX_DERIV_THROUGH_PLAIN_OPS
    stops = [rf, rl, ("ADC",), ("S", 1), rf, rl, ("SPOILER",), rf, ("S", 1), rl, ("ADC",), ("RESET",), rf, rl, ("S", 1), rf, rl, ("ADC",)]
    case("h_plain", stops, ("T2", "b1"), hess_name(64, 1, False), 64)
    case("h_plain_exact", stops, ("T2", "b1"), hess_name(64, 1, False), 64, exact=True)


_define()
