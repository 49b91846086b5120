"""The derivative cases through integer n-D shifts and diffusion that tests/test_gpu_nd_jacobian_paths.py runs on the device
and tests/test_nd_jacobian_recurrence_host.py measures on the CPU -- oracle tuples with a trailing {"order1": ..} (built on
tests/nd_cases.py), the variables, grid, options, the stored coordinates, the capacity K, `exact` (the device's
DERIV_THROUGH_PLAIN_OPS, the recurrence's through_plain) and the kernel name each case must get from choose_kernel
(csrc/epgx_planner.cpp) -- and the per-column check both use, against tests/nd_jacobian_recurrence.py in np.clongdouble:

    err_v = max|got[..., v] - ref[..., v]| / max|ref[..., v]|   <=   16 x the case's float64 floor   (never above 1e-11)

`floor`: there is no float64 oracle for any of this (oracle.simulate_nd has no partials, oracle.simulate_jacobian no n-D, and
the reference raises on such sequences), so the floor of a case is the per-column error of the SAME recurrence run in
np.complex128 against the np.clongdouble run -- the rule of the 1-D `D` case of tests/jacobian_cases.py -- measured by the host
test and tabulated in FLOORS between one and two times the measurement.  The operator-by-operator cases (group h) bound every
stored coordinate of every final derivative state by its own maximum, with COORD_FLOORS (the same rule, per coordinate) and the
cap of tests/nd_cases.py, 2e-12.

Steering the capacity: with the truncation box max_nstate = n, as tests/nd_cases.py does (61 / 41 stored coordinates at K = 64,
113 / 85 at 128, 221 / 145 at 256, 481 / 265 at 512, 1013 / 545 at 1024).

Groups: (a) deriv_kernel<M, NSP, V> from equilibrium, gather shifts without D, M = 1 .. 8  (b) deriv_kernel<16, NSP, 1>: the
two-pass gather  (c) the same kernels with D in the walk, each with exact=False and exact=True  (d) from a start state given
with coords=  (e) vectorised shifts  (f) 70 voxels  (g) through simulate()  (h) operator by operator (H_CASES):
op(sm) over a case's operators, sm.order1[var].states per coordinate.  Through that path `exact` is False whatever the case says: D
is a plain Operator there (epgpy_amd/diffusion.py), its __call__ never reaches sm.order1; S moves the derivative states
(diff.propagate_plain), SPOILER leaves them alone and RESET clears them (epgpy_amd/operator.py)."""
import numpy as np

from tests import nd_cases as nc, sequences as sq
from tests.jacobian_recurrence import column_errors
from tests.nd_cases import DT2, DT3, FILL2, FILL2_FAST, FILL3, KV, STRONG_KV, angle, box_coords, random_box_state, tissue  # noqa: F401

MARGIN = 16
CAP = 1e-11            # per column, the value of tests/jacobian_cases.py
COORD_CAP = 2e-12      # per coordinate (group h), the value of tests/nd_cases.py
MEASURED = {}          # group -> (largest error / floor, case)
CLOSEST = {}           # group -> (largest error / bound, case)
TRAIN_VARS = ["T2", "T1", "B1", "fa", "tau"]
RL = {"T1": {"T1": 1}, "T2": {"T2": 1}, "tau": {"tau": 1}}
NOMINAL = {"T2": 100.0, "T1": 900.0, "B1": 1.0, "fa": 60.0, "tau": 1.5}     # the magnitude a finite-difference step scales with

# float64 floors per column (max over columns), measured by tests/test_nd_jacobian_recurrence_host.py::test_floor_table_is_honest
FLOORS = {
    "a_64_61_1_3": 4.3e-16, "a_64_41_2_2": 5.4e-16, "a_64_61_3_1": 4.8e-16, "a_128_113_2_1": 5.5e-16, "a_128_85_3_3": 1.2e-15,
    "a_128_113_1_2": 9.6e-16, "a_256_221_3_2": 7.7e-16, "a_256_145_1_1": 8.3e-16, "a_256_221_2_3": 2.2e-15, "a_512_481_2_3": 1.1e-15,
    "a_512_265_1_2": 9.0e-16, "a_512_481_3_1": 5.1e-16, "b_545_1": 5.0e-16, "b_1013_2": 1.4e-15, "b_545_3": 1.1e-15,
    "c_scalar_k": 1.2e-15, "c_scalar_k_x": 8.7e-16, "c_scalar": 8.0e-16, "c_scalar_x": 5.6e-16, "c_field": 1.5e-15,
    "c_field_x": 1.8e-15, "c_tensor2": 1.2e-15, "c_tensor2_x": 9.6e-16, "c_tensor3": 6.8e-16, "c_tensor3_x": 7.8e-16,
    "c_1013": 1.2e-15, "c_1013_x": 1.1e-15, "c_strong_x": 1.1e-15, "d_64_in": 4.6e-16, "d_256_in": 4.7e-16,
    "d_1024_in": 2.7e-16, "e_lead1": 6.8e-16, "e_lead1_x": 5.3e-16, "e_lead2_box": 5.9e-16, "e_lead2_box_x": 8.3e-16,
    "f_70": 1.7e-15, "g_passes_256": 1.4e-15, "g_passes_1024": 1.3e-15, "g_probes": 7.1e-16,
}


# group h: float64 floors per coordinate of the final derivative states (tests/test_nd_jacobian_recurrence_host.py)
COORD_FLOORS = {"a_64_61_1_3": 3.5e-15, "c_scalar_k": 4.0e-15, "c_scalar_k_x": 4.0e-15, "e_lead1": 6.4e-16}
H_CASES = ["a_64_61_1_3", "c_scalar_k", "c_scalar_k_x", "e_lead1"]
H_EXACT = False        # what the operator-by-operator path does for D, whatever the case's `exact` says


def h_reference(name, dtype=np.clongdouble):
    """{variable: final derivative table} of a group-h case: its operators without the probes, D not acting on derivative states"""
    from tests.nd_jacobian_recurrence import nd_jacobian_recurrence
    c = CASES[name]
    tuples = [t for t in c["tuples"] if t[0] != "ADC"]
    return nd_jacobian_recurrence(tuples, c["variables"], shape=c["grid"], kvalue=c["opts"].get("kvalue", 1.0),
                                  max_nstate=c["opts"].get("max_nstate"), through_plain=H_EXACT, dtype=dtype, return_state=True)[2]


def table_coords(table):
    """the coordinates a table holds as sorted symmetric rows [*lead, R, kdim] (the form of StateMatrix.coords)"""
    keys = sorted(table)
    coords = np.array(keys, dtype=np.int64).reshape((len(keys),) + tuple(table.lead) + (table.kdim,))
    return np.moveaxis(coords, 0, -2)


def check_coordinates(name, group, got_half, want_rows, floor):
    """tests/nd_cases.py check_coordinates on a derivative state: every stored coordinate by its own maximum over voxels and
    components; a row whose coordinate the reference does not hold exactly zero"""
    from tests.signal_recurrence import order_errors
    errs = order_errors(got_half, want_rows)
    bound = MARGIN * floor
    assert bound <= COORD_CAP, (name, bound)
    worst = max(errs) if errs else 0.0
    if worst / floor > MEASURED.get(group, (0.0, None))[0]:
        MEASURED[group] = (worst / floor, name)
        CLOSEST[group] = (worst / bound, name)
    print(name, "coordinates: largest error", float(f"{worst:.3g}"), "=", float(f"{worst / floor:.3g}"), "floors; bound", bound)
    assert worst <= bound, (name, worst, bound)
    return errs


def check(name, group, got, want, floor):
    """per column, tests/jacobian_recurrence.py column_errors: a column whose reference is identically zero must be exactly zero"""
    errs = column_errors(got, want)
    bound = MARGIN * floor
    assert bound <= CAP, (name, bound)
    worst = max(errs)
    if worst / floor > MEASURED.get(group, (0.0, None))[0]:
        MEASURED[group] = (worst / floor, name)
        CLOSEST[group] = (worst / bound, name)
    print(name, "per-column errors", [float(f"{e:.3g}") for e in errs], "=", float(f"{worst / floor:.3g}"), "floors; bound", bound)
    assert worst <= bound, (name, errs, bound)
    return errs


# ------------------------------------------------------------------------------------------------ sequences (oracle tuples)
def o1_T(a, i):
    """B1 on every T with the coefficient alpha, fa on every other T"""
    return {"order1": {"B1": {"alpha": a}, **({"fa": {"alpha": 1.0}} if i % 2 else {})}}


def jwalk(T1, T2, B1, deltas, steps, *, tau=1.5, every=3, diffusion=None, tail=()):
    """nd_cases.walk carrying partials: B1 and fa on the rotations, T1 / T2 / tau on the relaxations"""
    a, p = angle(0)
    seq = [("T", a * B1, p, o1_T(a, 0))]
    for i in range(steps):
        d = deltas[i % len(deltas)]
        seq.append(("S", d))
        if i % every == every - 1:
            seq.append(("ADC", "Z0"))
        if diffusion is not None and diffusion(i, d) is not None:
            seq.append(diffusion(i, d))
        a, p = angle(i + 1)
        seq += [("E", tau, T1 if (np.ndim(T1) < 2 or i % 2 == 0) else 900.0, T2, {"order1": RL}), ("T", a * B1, p, o1_T(a, i + 1))]
        if i % every == every - 1:
            seq.append(("ADC",))
    return seq + list(tail) + [("ADC",), ("ADC", "Z0")]


def with_partials(tuples):
    """plain nd_cases tuples (scalar angles, B1 = 1) with order1 added"""
    out, i = [], 0
    for t in tuples:
        if t[0] == "T":
            assert np.ndim(t[1]) == 0
            out.append(t + (o1_T(float(t[1]), i),))
            i += 1
        elif t[0] == "E":
            out.append(t + ({"order1": RL},))
        else:
            out.append(t)
    return out


def with_probe(tuples, kind):
    """every ADC as the probe kind a Jacobian probe of simulate() records"""
    return [(("ADC",) if kind == "F0" else ("ADC", kind)) if t[0] == "ADC" else t for t in tuples]


def ops_of(tuples):
    """oracle tuples -> product operators (n-D shifts, D with k= / field=, order1 on T / E)"""
    from epgpy_amd import epg
    ops = []
    for t in tuples:
        o1 = t[-1]["order1"] if isinstance(t[-1], dict) else None
        args = t[1:-1] if isinstance(t[-1], dict) else t[1:]
        if t[0] == "T" and o1 is not None:
            ops.append(epg.T(args[0], args[1], order1=o1))
        elif t[0] == "E" and o1 is not None:
            ops.append(epg.E(*args, order1=o1))
        else:
            ops.extend(sq.nd_to_ops(epg, [t]))
    return ops


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def kn(nsp):
    return 4 if nsp > 2 else nsp


def dname(K, nsp, V):
    return f"deriv_kernel<{K // 64}, {kn(nsp)}, {V}>"


def case(name, group, tuples, variables, grid, K, nsp, *, opts=None, rows=None, exact=False, start=None, ref=None):
    """rows: the stored coordinates the plan must end with; exact: DERIV_THROUGH_PLAIN_OPS; start: (box n, kdim) of a random
    start state given with coords=; ref: the case whose tuples this one shares (its reference differs with `exact`)"""
    assert name not in CASES, name
    CASES[name] = dict(group=group, tuples=tuples, variables=list(variables), grid=tuple(grid), kernel=dname(K, nsp, len(variables)), K=K,
                       nsp=kn(nsp), V=len(variables), opts=dict(opts or {}), rows=rows, exact=exact, start=start, twin=ref, seed=len(CASES))


def variables_at(i, V):
    return [TRAIN_VARS[(i + j) % 5] for j in range(V)]


GRIDS = {1: 5, 2: (3, 2), 3: (2, 3)}
BOXES = {61: 5, 41: 4, 113: 7, 85: 6, 221: 10, 145: 8, 481: 15, 265: 11, 545: 16, 1013: 22}
NEAR_FULL = {}         # M -> the near-full case of group a / b (mutation vi of the host test)


def grid_of(nsp, n):
    return (n,) if nsp == 1 else tuple(n)


def _define():
    # (a) deriv_kernel<M, NSP, V> from equilibrium, LDS mode 3: per M one case filled to within a few rows of K, one just above K / 2
    # (the last register of a lane full / empty) and a third near-full one, so that every V and every NSP occurs once per M
    table = {64: [(61, 3, 1), (41, 2, 2), (61, 1, 3)], 128: [(113, 1, 2), (85, 3, 3), (113, 2, 1)],
             256: [(221, 2, 3), (145, 1, 1), (221, 3, 2)], 512: [(481, 3, 2), (265, 2, 1), (481, 1, 3)]}
    n = 0
    for K, rowsets in table.items():
        for rows, V, nsp in rowsets:
            box = BOXES[rows]
            T1, T2, B1 = tissue(nsp, 700 + K + rows + nsp, GRIDS[nsp])
            seq = jwalk(T1, T2, B1, FILL2 if box <= 8 else FILL2_FAST, 2 * box + 3, every=4)
            name = f"a_{K}_{rows}_{nsp}_{V}"
            case(name, "a", seq, variables_at(n, V), grid_of(nsp, GRIDS[nsp]), K, nsp, opts={"max_nstate": box, "kvalue": KV}, rows=rows)
            if rows > K // 2 + K // 4:
                NEAR_FULL.setdefault(K // 64, name)
            n += 1
    # (b) deriv_kernel<16, NSP, 1>: the two-pass gather on the state and on the derivative state, Z0 probes right after a gather
    for rows, nsp, var in [(545, 1, "T2"), (1013, 2, "B1"), (545, 3, "tau")]:
        box = BOXES[rows]
        g = 2 if nsp == 1 else (2, 2)
        T1, T2, B1 = tissue(nsp, 800 + rows + nsp, g)
        # (1013 rows: eight balanced-ternary steps fill the whole box -- every coordinate is a sum of +-1, +-3, +-9, +-9 per axis -- so
        # that the last register of a lane is populated well before the sequence's midpoint and its content walks home to a probe)
        fill = [[1, 0], [3, 0], [9, 0], [9, 0], [0, 1], [0, 3], [0, 9], [0, 9]] if rows == 1013 else []
        seq = jwalk(T1, T2, B1, fill + [FILL2_FAST[i % 9] for i in range(box + 8 - len(fill))], box + 8, every=6)
        name = f"b_{rows}_{nsp}"
        case(name, "b", seq, [var], grid_of(nsp, g), 1024, nsp, opts={"max_nstate": box, "kvalue": KV}, rows=rows)
        if rows == 1013:
            NEAR_FULL[16] = name
    # (c) D in the walk, every case with exact=False and exact=True (the same tuples, two references): a scalar with k=, a scalar
    # without, a per-voxel field, tensors in 2-D and 3-D; M = 1, 2, 4 and 16; one strongly attenuated case under exact=True
    field = ("field", np.array([0.4, 0.9, 1.4, 2.0, 2.7]) * 1e-3)
    for tag, K, rows, nsp, V, fill, dif, every in [
            ("scalar_k", 64, 61, 1, 2, FILL2, lambda i, d: ("D", 1.0, 0.8e-3, d) if i % 3 == 0 else None, 4),
            ("scalar", 128, 113, 2, 1, FILL2, lambda i, d: ("D", 1.0, 0.8e-3) if i % 3 == 1 else None, 4),
            ("field", 256, 221, 1, 3, FILL2_FAST, lambda i, d: ("D", 1.0, field, d) if i % 3 == 0 else None, 5),
            ("tensor2", 64, 61, 3, 3, FILL2, lambda i, d: ("D", 1.5, DT2, d) if i % 2 == 0 else None, 4),
            ("tensor3", 64, None, 2, 2, FILL3, lambda i, d: ("D", 1.5, DT3, d) if i % 2 == 0 else ("D", 1.0, DT3), 3),
            ("1013", 1024, 1013, 1, 1, FILL2_FAST, lambda i, d: ("D", 1.0, 0.5e-3, d) if i % 4 == 1 else None, 6)]:
        box = 2 if tag == "tensor3" else BOXES[rows]
        g = (2 if nsp == 1 else (2, 2)) if K == 1024 else GRIDS[nsp]
        T1, T2, B1 = tissue(nsp, 900 + K + nsp + V, g)
        steps = box + 8 if K == 1024 else (9 if tag == "tensor3" else 2 * box + 3)
        seq = jwalk(T1, T2, B1, fill, steps, every=every, diffusion=dif)
        var = variables_at(V + K // 64, V)
        for exact in (False, True):
            case(f"c_{tag}" + ("_x" if exact else ""), "c", seq, var, grid_of(nsp, g), K, nsp, opts={"max_nstate": box, "kvalue": KV}, rows=rows,
                 exact=exact, ref=f"c_{tag}" if exact else None)
    # (the tuples of nd_cases e_strong but for the excitation: at exactly 90 degrees the B1 partial of the first record is cos(90 deg),
    # rounding alone, next to a column maximum of 1e-8 -- ill-conditioned for that column; 80 degrees)
    strong = with_partials([("T", 80.0, 90.0)] + list(nc.CASES["e_strong"]["tuples"][1:]))
    case("c_strong_x", "c", strong, ["T2", "B1"], (5,), 64, 1, opts={"kvalue": STRONG_KV}, exact=True)
    # (d) from a start state on every coordinate of the box (the a.in load of the strided layout next to zeroed derivative states)
    for K, box, nsp, V, exact in [(64, 5, 1, 2, True), (256, 10, 2, 3, False), (1024, 22, 3, 1, True)]:
        g = 3 if nsp == 1 else (2, 2)
        T1, T2, B1 = tissue(nsp, 400 + K, g)
        o1 = lambda a, i: ("T", a * B1, [30.0, 25.0, -70.0][i], o1_T(a, i))
        rl = {"order1": RL}
        seq = [o1(55.0, 0), ("E", 2.0, T1, T2, rl), ("E", 1.0, 900.0, T2, rl), ("ADC", "Z0"), ("S", [1, 0]), ("D", 1.5, 0.7e-3, [1, 0]), ("ADC",),
               ("S", [-2, 1]), ("ADC", "Z0"), o1(40.0, 1), ("S", 1), ("E", 2.0, T1, T2, rl), ("SPOILER",) if K == 64 else ("D", 2.0, DT2), o1(65.0, 2),
               ("S", [0, -1]), ("ADC",), ("ADC", "Z0")]
        case(f"d_{K}_in", "d", seq, variables_at(K // 64, V), grid_of(nsp, g), K, nsp, opts={"max_nstate": box, "kvalue": KV},
             rows=((2 * box + 1) ** 2 + 1) // 2, exact=exact, start=(box, 2))
    # (e) vectorised shifts: K1 / K2 of nd_cases group f, a D table per voxel class, a shared shift, an int S(1), SPOILER / RESET inside
    # (K1 with its first two voxel classes: 2 x 3 voxels)
    for tag, src, grid in [("lead1", "f_lead1", (2, 3)), ("lead2_box", "f_lead2_box", (2, 3))]:
        seq = with_partials([("S", t[1][:2]) if (t[0] == "S" and tag == "lead1" and np.ndim(t[1]) == 3) else t for t in nc.CASES[src]["tuples"]])
        for exact in (False, True):
            case(f"e_{tag}" + ("_x" if exact else ""), "e", seq, ["T2", "B1"], grid, 64, 2, opts=nc.CASES[src]["opts"], exact=exact,
                 ref=f"e_{tag}" if exact else None)
    # (f) 70 voxels at K = 64: the block permutation (quad) and a ragged last block
    T1, T2, B1 = tissue(2, 555, (14, 5))
    case("f_70", "f", jwalk(T1, T2, B1, FILL2, 13, every=4, diffusion=lambda i, d: ("D", 1.0, 0.8e-3, d) if i % 3 == 0 else None), ["T2", "B1"],
         (14, 5), 64, 2, opts={"max_nstate": 5, "kvalue": KV}, rows=61, exact=True)


_define()

def g_cases():
    """name -> (tuples, variables, grid, options of simulate(), exact) of the simulate() cases (their floors: FLOORS)"""
    out = {}
    T1, T2, B1 = tissue(1, 610, 3)
    dif = lambda i, d: ("D", 1.0, 0.8e-3, d) if i % 3 == 0 else None
    out["g_passes_256"] = (with_probe(jwalk(T1, T2, B1, FILL2_FAST, 23, every=5, diffusion=dif), "F0"), list(TRAIN_VARS), (3,),
                           {"max_nstate": 10, "kvalue": KV}, True)
    T1, T2, B1 = tissue(1, 611, 2)
    out["g_passes_1024"] = (with_probe(jwalk(T1, T2, B1, FILL2_FAST, 30, every=6), "F0"), ["T2", "B1"], (2,), {"max_nstate": 22, "kvalue": KV}, False)
    seq = jwalk(900.0, 80.0, 1.0, FILL2, 13, every=4, diffusion=dif)
    out["g_probes"] = (seq, ["T2", "zzz", "B1"], (1,), {"max_nstate": 5, "kvalue": KV}, False)
    return out


# ------------------------------------------------------------------------------------------------ references and plans
def start_of(c):
    if c["start"] is None:
        return None
    return random_box_state(2000 + c["seed"], c["grid"], *c["start"])


def reference(name, dtype=np.clongdouble, return_state=False):
    from tests.nd_jacobian_recurrence import nd_jacobian_recurrence
    c = CASES[name]
    return nd_jacobian_recurrence(c["tuples"], c["variables"], shape=c["grid"], kvalue=c["opts"].get("kvalue", 1.0),
                                  max_nstate=c["opts"].get("max_nstate"), init=start_of(c), through_plain=c["exact"], dtype=dtype,
                                  return_state=return_state)


def compile_case(c):
    """(encoder, K): the derivative plan as _simulate_jacobian compiles it, from equilibrium or from the start state's coordinates"""
    from epgpy_amd import functions as _functions, kspace, _lib
    start = start_of(c)
    ks0 = None if start is None else kspace.KSpace.from_coords(start[1])
    enc, _, _ = _functions.compile_sequence(ops_of(c["tuples"]), shape=c["grid"], options=c["opts"], variables=c["variables"],
                                            nstate0=0 if ks0 is None else ks0.nstate, kspace0=ks0, dense_start=start is not None)
    assert enc.grid == c["grid"], (enc.grid, c["grid"])
    enc.deriv_flags |= _lib.DERIV_THROUGH_PLAIN_OPS if c["exact"] else 0
    assert not enc.packable(derivatives=True)
    return enc, enc.capacity(at_least=(ks0.nstate + 1) if ks0 is not None else 0)


def launch(c, want_name):
    """one derivative plan through _lib.run: ask for the kernel, hand its name to `want_name` BEFORE the launch, launch,
    download -> records [record, *grid, 1 + V]"""
    from epgpy_amd import _lib
    from epgpy_amd.statematrix import fold
    enc, K = compile_case(c)
    assert K == c["K"], (K, c["K"])
    assert c["rows"] is None or enc.kspace.nrow - enc.kspace.centre == c["rows"], (enc.kspace.nrow - enc.kspace.centre, c["rows"])
    assert enc.peak + 1 <= K
    start = start_of(c)
    ctx = _lib.get_context(0)
    plan = enc.device_plan(ctx, K)
    nvox, nrow = enc.nvox, 1 + c["V"]
    state = None
    if start is not None:
        state = _lib.DeviceState(ctx, nvox, K)
        state.upload(fold(start[0], K), np.ones(nvox))
    name = _lib.kernel_for(ctx, plan, K, state_in=state)
    want_name(name)
    nrec = sum(t[0] == "ADC" for t in c["tuples"])
    assert enc.n_adc == nrec * nrow
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, nvox, state, None, K, sig.ptr.value, nvox, 0)
    raw = sig.download(np.complex128, (nrec, nrow) + c["grid"])
    return np.moveaxis(raw, 1, -1)
