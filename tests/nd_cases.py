"""The n-D shift and diffusion cases that tests/test_gpu_nd_paths.py runs on the device and tests/test_nd_recurrence_host.py
measures on the CPU -- oracle tuples (the forms of tests/sequences.py nd_cases / nd_vector_cases), grid, options, the stored
coordinates, the capacity K and the kernel name each case must get from choose_kernel (csrc/epgx_planner.cpp) -- and the checks
both use, against the extended-precision recurrence of tests/nd_recurrence.py:

    check_records:      for every record r      max_vox|got[r] - want[r]|  <=  16 floor max_vox|want[r]|
    check_coordinates:  for every stored coordinate c   max|got[.., c] - want[.., c]|  <=  16 floor max over voxels and components
                        |want[.., c, :]|;  a row whose coordinate the reference does not hold, and every order from the plan's row
                        count up to K, exactly zero

`floor`: the largest per-record (per-coordinate) error of the float64 oracle, oracle.simulate_nd(prune=False), on that case,
measured by the host test and tabulated in FLOORS (rounded up to two digits).  Cases the oracle cannot run (a start state, P,
PD, RESET) take the recurrence itself in float64, as tests/signal_recurrence.py does for R and D.

Conditions that keep the tests honest, each checked on the CPU for every case (tests/test_nd_recurrence_host.py):
  1. no case skips a record or a coordinate: the bounds cover all of them;
  2. every bounded coordinate is genuinely populated: its reference maximum is at least POPULATED = 1e-9 of the state's maximum
     (angles and relaxation times are generic: no populated coordinate cancels);
  3. every float64 floor is finite and 16 x floor <= 2e-12;
  4. the union of the asserted kernel names covers rows_kernel<{1,2,4}, 1, false>, run_kernel<{1,2,4,8,16}, {1,2,4}, false>
     and run_kernel<{1,4,16}, ., true>  (REQUIRED_NAMES).

Steering the capacity: the number of stored coordinates is set with the truncation box max_nstate = n rather than with long
sequences; the half set of a filled 2-D box has ((2 n + 1)^2 + 1) / 2 coordinates, of a 3-D box ((2 n + 1)^3 + 1) / 2.

Groups: (a) rows_kernel<NSP, 1, false> at 16 orders and the same plans on run_kernel<1, NSP, false>  (b) run_kernel<M, NSP, false>,
M = 1 .. 8  (c) run_kernel<16, NSP, false>: the two-pass gather  (d) a state output, with and without a start state given with
coords=  (e) diffusion  (f) vectorised shifts."""
import itertools

import numpy as np

from tests import sequences as sq

MARGIN = 16
CAP = 2e-12
POPULATED = 1e-9
MEASURED = {}          # group -> (largest error / floor, case)
CLOSEST = {}           # group -> (largest error / bound, case)

FLOORS = {
    "b_128_113_2": 8.4e-15,
    "a_13_1_5": 2.4e-15, "a_16_1_65": 5.2e-15, "a_14_1_4": 3.2e-15, "a_16_2_6": 5.4e-15, "a_13_2_65": 2.9e-15,
    "a_14_3_6": 3.3e-15, "a_16_3_65": 5.9e-15, "a_13_0_1": 7.5e-16, "b_64_61_2": 2.4e-15, "b_64_41_3": 3.8e-15,
    "b_128_113_3": 2.9e-15, "b_128_85_1": 1.8e-15, "b_256_221_2": 1.0e-14, "b_256_145_3": 4.2e-15, "b_512_481_3": 7.1e-15,
    "b_512_265_1": 3.4e-15, "b_64_61_2_d": 4.5e-15, "b_64_61_3": 6.5e-15, "b_128_113_1": 3.3e-15, "b_128_113_3_d": 3.1e-15,
    "b_256_221_1": 4.7e-15, "b_256_221_2_d": 5.5e-15, "b_512_481_2": 5.5e-15, "b_512_481_3_d": 6.6e-15, "c_545_1": 3.1e-15,
    "c_1013_2_d": 5.5e-15, "c_1013_3": 6.6e-15, "c_545_3_d": 5.8e-15, "d_64_in": 1.0e-15, "d_64_eq": 1.6e-15,
    "d_256_in": 9.1e-16, "d_256_eq": 1.7e-15, "d_1024_in": 1.8e-15, "d_1024_eq": 2.0e-15, "e_scalar_k": 9.4e-15,
    "e_scalar": 5.0e-14, "e_field_k": 5.0e-14, "e_field": 9.4e-15, "e_tensor2": 8.7e-15, "e_tensor3": 5.0e-14,
    "e_tensor3_nok": 5.0e-14, "e_strong": 9.6e-16, "f_lead1": 7.2e-16, "f_lead1_box": 8.0e-16, "f_lead2": 6.9e-16,
    "f_lead2_box": 7.3e-16,
}


def _assert_bound(case, group, what, errs, floor):
    bound = MARGIN * floor
    assert bound <= CAP, (case, bound)
    worst = max(errs) if errs else 0.0
    at = int(np.argmax(errs)) if errs else -1
    if worst / floor > MEASURED.get(group, (0.0, None))[0]:
        MEASURED[group] = (worst / floor, case)
        CLOSEST[group] = (worst / bound, case)
    print(case, what, "largest error", float(f"{worst:.3g}"), "at", at, "=", float(f"{worst / floor:.3g}"), "floors; bound", bound)
    assert worst <= bound, (case, what, at, worst, bound)
    return errs


def check_records(case, group, got, want, floor):
    from tests.signal_recurrence import record_errors
    return _assert_bound(case, group, "records", record_errors(got, want), floor)


def check_coordinates(case, group, got_half, want_rows, floor):
    """got_half [*grid, 3, K]: the device buffer; want_rows [*grid, R, 3]: the reference laid out on the plan's rows"""
    from tests.signal_recurrence import order_errors
    return _assert_bound(case, group, "coordinates", order_errors(got_half, want_rows), floor)


# ------------------------------------------------------------------------------------------------ sequences (oracle tuples)
def tissue(nsp, seed, n):
    """(T1, T2, B1) over 1, 2 or 3 index spaces (the kernels' NSP = 1, 2, 4).  1: per-voxel tables on a grid (n,); 2: T2 on the first,
    B1 on the second axis of (a, b); 3: T1 dense over (a, b) as well"""
    rng = np.random.default_rng(seed)
    if nsp == 1:
        return 900.0, rng.uniform(60, 140, n), rng.uniform(0.9, 1.1, n)
    a, b = n
    T1 = rng.uniform(700, 1500, (a, b)) if nsp == 3 else 900.0
    return T1, rng.uniform(60, 140, (a, 1)), rng.uniform(0.9, 1.1, (1, b))


def angle(i):
    """generic flip angles and phases: nothing cancels, nothing is a multiple of 90 degrees"""
    return 35.0 + 50.0 * ((i * 0.6180339887) % 1.0), 360.0 * ((i * 0.4142135623) % 1.0) - 180.0


def walk(T1, T2, B1, deltas, steps, *, tau=1.5, every=3, diffusion=None, tail=()):
    """T, then `steps` x [S(delta_i), E, T] with the deltas taken in turn, an F0 / Z0 probe every `every` steps -- the Z0 probe
    right after the shift -- and `diffusion(i)` (a D tuple or None) after each shift"""
    a, p = angle(0)
    seq = [("T", a * B1, p)]
    for i in range(steps):
        d = deltas[i % len(deltas)]
        seq.append(("S", d))
        if i % every == every - 1:
            seq.append(("ADC", "Z0"))
        if diffusion is not None and diffusion(i, d) is not None:
            seq.append(diffusion(i, d))
        a, p = angle(i + 1)
        # (three index spaces: relaxation over the dense grid and over the first axis in turn, rotations over the second axis)
        seq += [("E", tau, T1 if (np.ndim(T1) < 2 or i % 2 == 0) else 900.0, T2), ("T", a * B1, p)]
        if i % every == every - 1:
            seq.append(("ADC",))
    return seq + list(tail) + [("ADC",), ("ADC", "Z0")]


FILL2 = [[1, 0], [-2, 1], [0, 1], [1, 1], [1, -1], [2, 1], [-1, 2]]       # S([1, 0]) then S([-2, 1]): populated coordinates cross k = 0
FILL2_FAST = [[1, 0], [-2, 1], [3, 2], [-1, 3], [4, -1], [2, -3], [0, 1], [-3, 1], [1, 4]]
FILL3 = [[1, 0, 0], [-2, 1, 0], [0, 1, 1], [1, -1, 1], [0, 0, 1], [1, 1, -1], [-1, 0, 2]]
DT2 = np.array([[1.0, 0.3], [0.3, 1.8]]) * 1e-3
DT3 = np.array([[1.0, 0.2, 0.0], [0.2, 2.0, 0.1], [0.0, 0.1, 0.5]]) * 1e-3
KV = [900.0, 700.0, 500.0]      # rad/m per order and axis: the three axes differ
STRONG_KV = [4e5, 3e5, 2e5]     # the strongly attenuated case: tr(b D) of about 5 per lobe and 7 per echo half


def box_coords(n, kdim):
    """every coordinate of the box |c_i| <= n, rows sorted lexicographically (symmetric about the centre): [R, kdim]"""
    return np.array(list(itertools.product(range(-n, n + 1), repeat=kdim)), dtype=np.int64)


def random_box_state(seed, grid, n, kdim):
    """a valid start state on every coordinate of the box (F-(c) = conj F+(-c), Z(-c) = conj Z(c), Z(0) real), amplitudes falling
    with the distance from the centre: (states [*grid, R, 3], coords [R, kdim])"""
    rng = np.random.default_rng(seed)
    coords = box_coords(n, kdim)
    R = len(coords)
    c0 = (R - 1) // 2
    fall = 0.3 * np.exp(-np.max(np.abs(coords), axis=1) * (3.0 / max(n, 1)))
    shape = tuple(grid) + (R,)
    f = (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)) * fall
    z = (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)) * fall
    z = 0.5 * (z + z[..., ::-1].conj())
    z[..., c0] = z[..., c0].real
    return np.stack([f, f[..., ::-1].conj(), z], axis=-1), coords


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def case(name, group, tuples, grid, kernel, K, *, opts=None, rows=None, out=False, start=None, packed=True, ref=None):
    """rows: the number of stored coordinates the plan must end with (asserted on the CPU and before the launch); out: a state
    output, compared per coordinate; start: (box n, kdim) of a random start state given with coords=; packed=False: the plan
    of a 16-order case at K = 64; ref: the case whose reference this one shares"""
    assert name not in CASES, name
    CASES[name] = dict(group=group, tuples=tuples, grid=tuple(grid), kernel=kernel, K=K, opts=dict(opts or {}), rows=rows, out=out,
                       start=start, packed=packed, ref=ref or name, seed=len(CASES))


def kn(nsp):
    return 4 if nsp > 2 else nsp


GRIDS = {1: 5, 2: (3, 2), 3: (2, 3)}


def _define():
    # (a) sixteen orders, four voxels per wavefront: 13 stored coordinates (2-D box of 2), 14 (3-D box of 1), exactly 16 (a 2-D
    # walk along one axis, box of 15); 1, 4, 5 and 65 voxels; each plan again with packed=False at K = 64
    fills = {13: (FILL2, 2, 9), 14: (FILL3, 1, 9), 16: ([[1, 0], [2, 0], [-1, 0]], 15, 14)}
    for nsp, rows, n in [(1, 13, 5), (1, 16, 65), (1, 14, 4), (2, 16, (3, 2)), (2, 13, (13, 5)), (3, 14, (2, 3)), (3, 16, (5, 13))]:
        T1, T2, B1 = tissue(nsp, 100 + nsp + rows, n)
        deltas, box, steps = fills[rows]
        dif = (lambda i, d: ("D", 2.0, 1.1e-3, d)) if rows != 16 else (lambda i, d: ("D", 2.0, 0.9e-3) if i % 2 else None)
        seq = walk(T1, T2, B1, deltas, steps, diffusion=dif)
        grid = (n,) if nsp == 1 else n
        nm = f"a_{rows}_{nsp}_{int(np.prod(grid))}"
        case(nm, "a", seq, grid, f"rows_kernel<{kn(nsp)}, 1, false>", 16, opts={"max_nstate": box, "kvalue": KV}, rows=rows)
        case(nm + "_wide", "a", seq, grid, f"run_kernel<1, {kn(nsp)}, false>", 64, opts={"max_nstate": box, "kvalue": KV}, rows=rows,
             packed=False, ref=nm)
    case("a_13_0_1", "a", walk(900.0, 80.0, 1.0, FILL2, 9, diffusion=lambda i, d: ("D", 2.0, 1.1e-3, d)), (1,), "rows_kernel<0, 1, false>", 16,
         opts={"max_nstate": 2, "kvalue": KV}, rows=13)
    # (b) run_kernel<M, NSP, false> from equilibrium, LDS mode 3: per M one case filled to within a few coordinates of K and one just
    # above K / 2; NSP through per-voxel, per-axis and dense parameters; GS_CONJ in both tables, GS_ZERO sources (asserted on the plan)
    for K, full, half in [(64, (2, 5, 61), (2, 4, 41)), (128, (2, 7, 113), (2, 6, 85)), (256, (2, 10, 221), (2, 8, 145)),
                          (512, (2, 15, 481), (2, 11, 265))]:
        for j, (kdim, box, rows) in enumerate((full, half)):
            nsp = 1 + (K // 64 + j) % 3
            T1, T2, B1 = tissue(nsp, 200 + K + j, GRIDS[nsp])
            seq = walk(T1, T2, B1, FILL2 if box <= 8 else FILL2_FAST, 2 * box + 3, every=4)
            grid = (GRIDS[nsp],) if nsp == 1 else GRIDS[nsp]
            case(f"b_{K}_{rows}_{nsp}", "b", seq, grid, f"run_kernel<{K // 64}, {kn(nsp)}, false>", K, opts={"max_nstate": box, "kvalue": KV},
                 rows=rows)
    for K, box, rows, nsp in [(64, 5, 61, 2), (64, 5, 61, 3), (128, 7, 113, 1), (128, 7, 113, 2), (128, 7, 113, 3), (256, 10, 221, 1), (256, 10, 221, 2),
                              (512, 15, 481, 2), (512, 15, 481, 3)]:      # the NSP each M has not had yet, with diffusion
        T1, T2, B1 = tissue(nsp, 250 + K + nsp, GRIDS[nsp])
        seq = walk(T1, T2, B1, FILL2 if box <= 8 else FILL2_FAST, 2 * box + 3, every=5, diffusion=lambda i, d: ("D", 1.0, 0.8e-3, d) if i % 3 == 0 else None)
        grid = (GRIDS[nsp],) if nsp == 1 else GRIDS[nsp]
        nm = f"b_{K}_{rows}_{nsp}"
        case(nm + ("_d" if nm in CASES else ""), "b", seq, grid, f"run_kernel<{K // 64}, {kn(nsp)}, false>", K, opts={"max_nstate": box, "kvalue": KV}, rows=rows)
    # (c) run_kernel<16, NSP, false>: 545 (box of 16) and 1013 (box of 22) stored coordinates, with and without D, the Z0 probe of
    # `walk` right after a gather (the second pass is what it records), the box truncating
    for box, rows, nsp, dif in [(16, 545, 1, False), (22, 1013, 2, True), (22, 1013, 3, False), (16, 545, 3, True)]:
        T1, T2, B1 = tissue(nsp, 300 + box + nsp, 2 if nsp == 1 else (2, 2))
        seq = walk(T1, T2, B1, FILL2_FAST, box + 8, every=6, diffusion=(lambda i, d: ("D", 1.0, 0.5e-3, d) if i % 4 == 1 else None) if dif else None)
        grid = (2,) if nsp == 1 else (2, 2)
        case(f"c_{rows}_{nsp}" + ("_d" if dif else ""), "c", seq, grid, f"run_kernel<16, {kn(nsp)}, false>", 1024,
             opts={"max_nstate": box, "kvalue": KV}, rows=rows)
    # (d) a state output: from equilibrium into a buffer pre-filled with 7 + 7i, and from a start state on every coordinate of the box
    # (the upper part of K: 61 of 64, 221 of 256, 1013 of 1024), records and final state
    for K, box, nsp in [(64, 5, 1), (256, 10, 2), (1024, 22, 3)]:
        g = 3 if nsp == 1 else (2, 2)
        T1, T2, B1 = tissue(nsp, 400 + K, g)
        grid = (g,) if nsp == 1 else g
        tail = [("S", [1, 0]), ("D", 1.5, 0.7e-3, [1, 0]), ("ADC",), ("S", [-2, 1]), ("ADC", "Z0"), ("T", 40.0 * B1, 25.0), ("S", 1),
                ("E", 2.0, T1, T2), ("SPOILER",) if K == 64 else ("D", 2.0, DT2), ("T", 65.0 * B1, -70.0), ("S", [0, -1])]
        seq = [("T", 55.0 * B1, 30.0), ("E", 2.0, T1, T2), ("E", 1.0, 900.0, T2), ("ADC", "Z0")] + tail + [("ADC",), ("ADC", "Z0")]
        case(f"d_{K}_in", "d", seq, grid, f"run_kernel<{K // 64}, {kn(nsp)}, true>", K, opts={"max_nstate": box, "kvalue": KV},
             rows=((2 * box + 1) ** 2 + 1) // 2, out=True, start=(box, 2))
        seq = walk(T1, T2, B1, FILL2, 4, every=2, diffusion=lambda i, d: ("D", 1.5, 0.7e-3, d))
        case(f"d_{K}_eq", "d", seq, grid, f"run_kernel<{K // 64}, {kn(nsp)}, false>", K, opts={"max_nstate": box, "kvalue": KV}, out=True)
    # (e) diffusion, a kvalue per axis: scalar D with and without k=, a per-voxel field, tensors in 2-D and 3-D, D before the first
    # n-D shift (1-D orders), D with k= right after the matching S, one strongly attenuated case
    T2 = np.array([60.0, 90.0, 140.0, 75.0, 110.0])
    field = ("field", np.array([0.4, 0.9, 1.4, 2.0, 2.7]) * 1e-3)
    head = [("T", 70.0, 30.0), ("S", 1), ("D", 3.0, 1.2e-3), ("E", 3.0, 900.0, T2), ("T", 50.0, -40.0), ("S", 1), ("D", 3.0, 1.2e-3, [1]), ("ADC",)]

    def dseq(D, kdim, k=True):
        d1, d2 = ([1, 0], [-2, 1]) if kdim == 2 else ([1, 0, 1], [-2, 1, 0])
        return head + [("T", 65.0, 15.0), ("S", d1), ("D", 4.0, D, d1) if k else ("D", 4.0, D), ("E", 4.0, 900.0, T2), ("ADC", "Z0"), ("T", 100.0, -20.0),
                       ("S", d2), ("D", 6.0, D, d2) if k else ("D", 6.0, D), ("ADC",), ("T", 80.0, 70.0), ("S", d1), ("D", 2.0, D), ("E", 2.0, 900.0, T2),
                       ("ADC",), ("ADC", "Z0")]
    for nm, D, kdim, k in [("scalar_k", 1.3e-3, 2, True), ("scalar", 1.3e-3, 3, False), ("field_k", field, 3, True), ("field", field, 2, False),
                           ("tensor2", DT2, 2, True), ("tensor3", DT3, 3, True), ("tensor3_nok", DT3, 3, False)]:
        seq = dseq(D, kdim, k)
        if nm.startswith("tensor"):      # (a tensor needs coordinates of its dimension: no D on 1-D orders)
            seq = [t for t in seq if not (t[0] == "D" and np.ndim(t[2]) == 0 and not isinstance(t[2], tuple))]
        if kdim == 3:                    # (38 stored coordinates)
            case("e_" + nm, "e", seq, (5,), "run_kernel<1, 1, false>", 64, opts={"kvalue": KV})
            continue
        case("e_" + nm, "e", seq, (5,), "rows_kernel<1, 1, false>", 16, opts={"kvalue": KV})
        case("e_" + nm + "_wide", "e", seq, (5,), "run_kernel<1, 1, false>", 64, opts={"kvalue": KV}, packed=False, ref="e_" + nm)
    strong = [("T", 90.0, 90.0), ("ADC",), ("S", [2, -1, 1]), ("D", 32.0, DT3, [2, -1, 1]), ("E", 32.0, 1000.0, T2), ("T", 170.0, 5.0),
              ("S", [2, -1, 1]), ("D", 32.0, DT3, [2, -1, 1]), ("E", 32.0, 1000.0, T2), ("ADC",)]
    case("e_strong", "e", strong, (5,), "rows_kernel<1, 1, false>", 16, opts={"kvalue": STRONG_KV})
    case("e_strong_wide", "e", strong, (5,), "run_kernel<1, 1, false>", 64, opts={"kvalue": STRONG_KV}, packed=False, ref="e_strong")
    # (f) vectorised shifts: one vector per voxel of the leading axis (and of the two leading axes), then D (a table per voxel
    # class), a shared shift, an int shift, SPOILER / RESET inside; a box in which some classes are inside and some outside
    K1 = np.array([[1, 0, 0], [2, 1, 0], [1, -1, 2], [0, 2, -1]])[:, None, :]
    K2 = np.array([[[1, 1], [2, -1], [0, 1]], [[-1, 2], [3, 0], [1, -2]]])            # [2, 3, kdim]: the two leading axes
    T2b = np.array([[50.0, 90.0, 150.0]])

    def vseq(Kv, Dv, shared):
        return [("T", 80.0, 60.0), ("S", Kv), ("D", 5.0, Dv), ("E", 5.0, 1000.0, T2b), ("ADC", "Z0"), ("T", 150.0, 10.0), ("S", Kv), ("D", 5.0, Dv),
                ("ADC",), ("T", 60.0, 20.0), ("S", shared), ("D", 3.0, 1.2e-3, shared), ("E", 3.0, 1000.0, T2b), ("ADC", "Z0"), ("T", 100.0, -30.0),
                ("S", 1), ("ADC",), ("SPOILER",), ("T", 50.0, 45.0), ("S", Kv), ("T", 75.0, -15.0), ("S", -1), ("ADC",), ("RESET",), ("ADC", "Z0"),
                ("T", 40.0, 35.0), ("S", Kv), ("D", 2.0, Dv), ("T", 140.0, 0.0), ("S", Kv), ("ADC",), ("ADC", "Z0")]
    for nm, Kv, Dv, shared, grid, opts, K in [
            ("lead1", K1, DT3, [1, 0, 0], (4, 3), {}, 64), ("lead1_box", K1, 1.1e-3, [1, 0, 0], (4, 3), {"max_nstate": 2}, 16),
            ("lead2", K2, DT2, [0, 1], (2, 3), {}, 64), ("lead2_box", K2, 0.8e-3, [0, 1], (2, 3), {"max_nstate": 3}, 64)]:
        kernel = "rows_kernel<2, 1, false>" if K == 16 else "run_kernel<1, 2, false>"
        seq = vseq(Kv, Dv, shared)
        case("f_" + nm, "f", seq, grid, kernel, K, opts={**opts, "kvalue": KV})
        if K == 16:
            case("f_" + nm + "_wide", "f", seq, grid, "run_kernel<1, 2, false>", 64, opts={**opts, "kvalue": KV}, packed=False, ref="f_" + nm)


_define()

REQUIRED_NAMES = sorted([f"rows_kernel<{n}, 1, false>" for n in (1, 2, 4)]
                        + [f"run_kernel<{m}, {n}, false>" for m in (1, 2, 4, 8, 16) for n in (1, 2, 4)]
                        + ["run_kernel<1, 1, true>", "run_kernel<4, 2, true>", "run_kernel<16, 4, true>"])


# ------------------------------------------------------------------------------------------------ references
def start_of(c):
    """(states [*grid, R, 3], coords [R, kdim]) of the case's start state, or None"""
    if c["start"] is None:
        return None
    return random_box_state(2000 + c["seed"], c["grid"], *c["start"])


def reference(name, oracle=False):
    """(records, final table) in extended precision; oracle: (records, (states, coords)) of oracle.simulate_nd(prune=False) --
    or, for what that cannot run, (records, table) of the recurrence in float64"""
    from tests.nd_recurrence import nd_recurrence
    c = CASES[name]
    opts = dict(kvalue=c["opts"].get("kvalue", 1.0), max_nstate=c["opts"].get("max_nstate"))
    if oracle and c["start"] is None and not any(t[0] in ("RESET", "PD", "P") for t in c["tuples"]):
        from oracle import epg_numpy as onp
        return onp.simulate_nd(c["tuples"], shape=c["grid"], prune=False, return_states=True, **opts)
    return nd_recurrence(c["tuples"], shape=c["grid"], init=start_of(c), return_state=True,
                         dtype=np.complex128 if oracle else np.clongdouble, **opts)


def rows_on(final, coords, grid):
    """a final state -- the recurrence's table, or the oracle's (states, coords) -- laid out on the rows `coords`: [*grid, R, 3]"""
    from tests.nd_recurrence import layout, NDState, coord_keys
    if isinstance(final, dict):
        return layout(final, coords, grid)
    states, own = final
    table = NDState()
    own = np.asarray(own)
    table.lead, table.kdim = tuple(own.shape[:-2]), own.shape[-1]
    while table.lead and table.lead[-1] == 1:
        table.lead = table.lead[:-1]
    mid = (own.shape[-2] - 1) // 2
    for r, key in enumerate(coord_keys(own)):
        if states[..., r, :].any() or states[..., 2 * mid - r, 0].any():
            table[key] = (np.broadcast_to(states[..., r, 0], grid), np.broadcast_to(states[..., r, 2], grid))
    return layout(table, coords, grid)


# ------------------------------------------------------------------------------------------------ the plan
def ops_of(tuples):
    from epgpy_amd import epg
    return sq.nd_to_ops(epg, tuples)


def compile_case(c):
    """(encoder, K): the plan as simulate() compiles it, from equilibrium or from the start state's coordinates"""
    from epgpy_amd import functions as _functions, kspace
    start = start_of(c)
    ks0 = None if start is None else kspace.KSpace.from_coords(start[1])
    enc, _, _ = _functions.compile_sequence(ops_of(c["tuples"]), shape=c["grid"], options=c["opts"], nstate0=0 if ks0 is None else ks0.nstate,
                                            kspace0=ks0, dense_start=start is not None)
    assert enc.grid == c["grid"], (enc.grid, c["grid"])
    # (a state output from equilibrium: at the case's capacity, the orders above the plan's rows stay zero up to K)
    K = enc.packable_nd() if (c["packed"] and start is None and not c["out"] and enc.packable_nd()) else enc.capacity(at_least=c["K"] if c["out"] else 0)
    return enc, K


def launch(c, want_name=None):
    """one plan through _lib.run at the case's capacity: ask for the kernel, hand its name to `want_name` BEFORE the launch,
    launch, download -> (name, records [record, *grid], half state [*grid, 3, K] or None, coords of the plan's rows)"""
    from epgpy_amd import _lib
    from epgpy_amd.statematrix import fold
    enc, K = compile_case(c)
    assert K == c["K"], (K, c["K"])
    assert c["rows"] is None or enc.kspace.nrow - enc.kspace.centre == c["rows"], (enc.kspace.nrow - enc.kspace.centre, c["rows"])
    assert enc.peak + 1 <= K
    start = start_of(c)
    ctx = _lib.get_context(0)
    plan = enc.device_plan(ctx, K)
    nvox = enc.nvox
    state = None
    if start is not None or c["out"]:
        state = _lib.DeviceState(ctx, nvox, K)
        state.upload(fold(start[0], K) if start is not None else np.full((nvox, 3, K), 7.0 + 7.0j), np.ones(nvox))
    s_in, s_out = (state if start is not None else None), (state if c["out"] else None)
    name = _lib.kernel_for(ctx, plan, K, state_in=s_in, state_out=s_out)
    if want_name is not None:
        want_name(name)
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, nvox, s_in, s_out, K, sig.ptr.value, nvox, 0)
    records = sig.download(np.complex128, (enc.n_adc,) + c["grid"])
    half = state.download()[0].reshape(c["grid"] + (3, K)) if c["out"] else None
    return name, records, half, enc.kspace.coords
