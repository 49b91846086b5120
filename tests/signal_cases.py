"""The plain-signal cases that tests/test_gpu_signal_paths.py runs on the device and tests/test_signal_recurrence_host.py
measures on the CPU -- oracle tuples, the capacity, the start state, and the kernel name each case must get from choose_kernel
(csrc/epgx_api.hip) -- and the two checks both use, against the extended-precision recurrence (tests/signal_recurrence.py):

    check_records:  for every record r   max_vox|got[r] - want[r]|  <=  16 floor max_vox|want[r]|
    check_orders:   for every order k    max|got[.., k] - want[.., k]|  <=  16 floor max over voxels and components |want[.., k, :]|
                    and every order of the device buffer above the reference's n, up to the capacity K, exactly zero

`floor`: the largest per-record (per-order) error of the float64 oracle on that case, measured by the host test and tabulated
in FLOORS (rounded up to two digits); 16 x floor may not exceed 2e-12.  A bound scaled by the whole array admits an error of
1e-12 in a record of 1e-5 -- the fifth digit of a late echo; these do not.

Groups: (a) rows_kernel<NSP, R, RUNS>  (b) rows_grow_kernel<NSP>  (c) run_contig_kernel<M, NSP, HAS_IN>
(d) run_contig_grow_kernel<M, NSP>  (e) K = 2048  (f) run_kernel<M, NSP, HAS_IN> with a state output.

Run as a script -- `signal_cases.py OUT.npz NAME ...` -- it launches the named cases and writes their records: the device
test starts it as a child process with EPGX_CGROW=0 EPGX_SPLIT_GROW=0 EPGX_ROWS=0 for the kernels that from equilibrium are reached only
with those measurement knobs (the library reads them once per process)."""
import sys

import numpy as np

MARGIN = 16            # four bits over the float64 floor: re-association of fused E . T . E tables, run-time fold, sum / difference cell
CAP = 2e-12            # no case may need more per record or per order
MEASURED = {}          # group -> largest per-record / per-order error seen

# float64 floors: the largest per-record (and, where a state is compared, per-order) error of the oracle against the recurrence,
# measured on the CPU by tests/test_signal_recurrence_host.py and rounded up to two digits.  A floor is never raised to make a
# device case pass; a case whose ORACLE needs 16 x floor > 2e-12 gets other inputs.
FLOORS = {
    "a_16_runs_1": 2.0e-15, "a_16_plain_1": 2.0e-15, "a_32_runs_1": 2.7e-15, "a_32_plain_1": 3.6e-15, "a_64_runs_1": 4.9e-14,
    "a_64_plain_1": 2.5e-14, "a_128_1": 7.2e-15, "a_16_runs_2": 1.8e-15, "a_16_plain_2": 1.9e-15, "a_32_runs_2": 2.4e-15,
    "a_32_plain_2": 5.6e-15, "a_64_runs_2": 2.2e-14, "a_64_plain_2": 4.2e-15, "a_128_2": 9.1e-15, "a_16_runs_3": 3.0e-15,
    "a_16_plain_3": 1.5e-15, "a_32_runs_3": 3.0e-15, "a_32_plain_3": 2.5e-15, "a_64_runs_3": 5.2e-14,
    "a_64_plain_3": 5.5e-15, "a_128_3": 1.1e-14, "b_echo_7": 8.5e-16, "b_echo_8": 5.4e-16, "b_echo_9": 2.1e-15,
    "b_echo_15": 3.5e-15, "b_echo_16": 2.8e-15, "b_echo_17": 4.7e-15, "b_echo_40": 1.8e-15, "b_stops_1": 2.7e-15,
    "b_stops_2": 6.1e-15, "b_stops_3": 6.5e-15, "b_decay_60": 4.5e-15, "c_128_in_1": 4.2e-16, "c_128_eq_1": 7.7e-15,
    "c_128_in_2": 5.0e-16, "c_128_eq_2": 2.1e-15, "c_128_in_3": 3.2e-16, "c_128_eq_3": 8.1e-15, "c_256_in_1": 1.2e-15,
    "c_256_eq_1": 1.2e-14, "c_256_in_2": 6.7e-16, "c_256_eq_2": 1.7e-14, "c_256_in_3": 5.6e-16, "c_256_eq_3": 2.9e-14,
    "c_512_in_1": 3.3e-16, "c_512_eq_1": 1.7e-14, "c_512_in_2": 6.2e-16, "c_512_eq_2": 7.4e-15, "c_512_in_3": 1.1e-15,
    "c_512_eq_3": 2.8e-15, "c_1024_in_1": 8.7e-16, "c_1024_eq_1": 1.1e-13, "c_1024_in_2": 5.4e-16, "c_1024_eq_2": 9.1e-15,
    "c_1024_in_3": 4.1e-16, "c_1024_eq_3": 4.4e-15, "d_128_1": 2.5e-15, "d_128_2": 2.8e-15, "d_128_3": 5.7e-15,
    "d_256_1": 6.1e-15, "d_256_2": 1.8e-15, "d_256_3": 6.7e-15, "d_512_1": 5.8e-15, "d_512_2": 1.3e-14, "d_512_3": 1.8e-14,
    "d_1024_1": 1.4e-14, "d_1024_2": 3.4e-14, "d_1024_3": 4.6e-14, "e_legs_1": 6.5e-14, "e_legs_2": 2.6e-14,
    "e_legs_3": 9.7e-15, "f_64_eq_1": 1.2e-15, "f_64_in_1": 7.8e-16, "f_64_eq_2": 2.9e-15, "f_64_in_2": 1.0e-15,
    "f_64_eq_3": 2.6e-15, "f_64_in_3": 9.6e-16, "f_128_eq_1": 1.1e-15, "f_128_in_1": 8.8e-16, "f_128_eq_2": 1.3e-15,
    "f_128_in_2": 8.3e-16, "f_128_eq_3": 1.1e-15, "f_128_in_3": 7.6e-16, "f_256_eq_1": 1.4e-15, "f_256_in_1": 8.3e-16,
    "f_256_eq_2": 1.2e-15, "f_256_in_2": 8.5e-16, "f_256_eq_3": 1.3e-15, "f_256_in_3": 7.6e-16, "f_512_eq_1": 7.1e-16,
    "f_512_in_1": 1.2e-15, "f_512_eq_2": 1.9e-15, "f_512_in_2": 1.3e-15, "f_512_eq_3": 2.5e-15, "f_512_in_3": 1.6e-15,
    "f_1024_eq_1": 1.2e-15, "f_1024_in_1": 9.3e-16, "f_1024_eq_2": 1.1e-15, "f_1024_in_2": 9.3e-16, "f_1024_eq_3": 1.5e-15,
    "f_1024_in_3": 1.5e-15,
}


def floor_of(name):
    return FLOORS[name]


def _assert_bound(group, what, errs, floor):
    bound = MARGIN * floor
    assert bound <= CAP, (group, bound)
    worst = max(errs) if errs else 0.0
    MEASURED[group] = max(MEASURED.get(group, 0.0), worst)
    at = int(np.argmax(errs)) if errs else -1
    print(group, what, "largest error", float(f"{worst:.3g}"), "at", at, "=", float(f"{worst / floor:.3g}"), "floors; bound", bound)
    assert worst <= bound, (group, what, at, worst, bound)
    return errs


def check_records(group, got, want, floor):
    """per record r: max over voxels |got[r] - want[r]| <= 16 floor max over voxels |want[r]|; a record whose reference is
    identically zero must be exactly zero"""
    from tests.signal_recurrence import record_errors
    return _assert_bound(group, "records", record_errors(got, want), floor)


def check_orders(group, got_half, want_state, floor):
    """per order k of the device's half buffer [*grid, 3, K] against the reference state [*grid, 2 n + 1, 3]; orders above n,
    up to K, and orders the sequence never populated must be exactly zero"""
    from tests.signal_recurrence import order_errors
    return _assert_bound(group, "orders", order_errors(got_half, want_state), floor)


# ------------------------------------------------------------------------------------------------ sequences (oracle tuples)
def tissue(nsp, seed, n=7, t2=(40.0, 100.0)):
    """(T1, T2, B1, extra records per echo); T2 within a factor of three, so that no voxel's decay sets the scale of a late
    record alone.  1 index space: per-voxel tables on one axis of n; 2: (T1, T2) on one axis, B1 on the other; 3 (the kernels'
    NSP = 4): (T1, T2) dense over two axes, B1 along the first, a further relaxation along the second.  `n` for 2 / 3 spaces:
    (a, b)"""
    rng = np.random.default_rng(seed)
    if nsp == 1:
        return rng.uniform(600, 2000, n), rng.uniform(*t2, n), rng.uniform(0.85, 1.15, n), []
    a, b = n
    if nsp == 2:
        return rng.uniform(600, 2000, (a, 1)), rng.uniform(*t2, (a, 1)), rng.uniform(0.85, 1.15, (1, b)), []
    T2 = rng.uniform(*t2, (1, b))
    return rng.uniform(600, 2000, (a, 1)), T2, rng.uniform(0.85, 1.15, (a, 1)), [("E", 0.1, 1200.0, T2, 0)]


def echoes(T1, T2, B1, extra, necho, tau=2.5, alpha=150.0):
    """`extra`, then [S E T S E ADC] x necho, the SAME tuple objects in every echo (one operator object each: the library folds the run)"""
    rfc, rlx, sh, adc = ("T", alpha * B1, 0.0), ("E", tau, T1, T2, 0), ("S", 1), ("ADC",)
    return prep(extra) + [sh, rlx, rfc, sh, rlx, adc] * necho


def prep(extra):
    """the records of the third index space, once and between probes (nothing fuses across a probe): inside every echo they
    would break the runs of identical records that the rows kernels fold"""
    return [("ADC", "Z0")] + extra + [("ADC", "Z0", 15.0)] if extra else []


def cpmg(T1, T2, B1, extra, necho, tau=None, alpha=150.0):
    """90 degree excitation and an echo train; tau: half the echo spacing (default: the train lasts at most 150 ms)"""
    tau = min(2.5, 75.0 / necho) if tau is None else tau
    return [("T", 90 * B1, 90.0)] + echoes(T1, T2, B1, extra, necho, tau, alpha)


def runs_train(T1, T2, B1, extra, nlong, tau=2.5):
    """runs of identical records of length 1, 2 and `nlong`: three refocusing angles"""
    return ([("T", 90 * B1, 90.0)] + echoes(T1, T2, B1, extra, 1, tau, 120.0) + echoes(T1, T2, B1, extra, 2, tau, 160.0)
            + echoes(T1, T2, B1, extra, nlong, tau, 140.0))


def irregular(T1, T2, B1, extra, nops, seed):
    """no two records alike and no repeating pattern (nothing for the run-length fold): rotations about changing axes, relaxation
    with precession, precession, shifts by +1 (sometimes -1), F0 / Z0 probes with and without a phase"""
    rng = np.random.default_rng(seed)
    seq = [("T", 70 * B1, 30.0)]
    for _ in range(nops):
        r = rng.random()
        if r < 0.25:
            seq.append(("T", float(rng.uniform(10, 170)) * B1, float(rng.uniform(-180, 180))))
        elif r < 0.45:
            seq.append(("E", float(rng.uniform(0.5, 4)), T1, T2, float(rng.uniform(-0.03, 0.03))))
        elif r < 0.5:
            seq.append(("P", float(rng.uniform(0.5, 4)), float(rng.uniform(-0.05, 0.05))))
        elif r < 0.8:
            seq.append(("S", 1 if rng.random() < 0.85 else -1))
        else:
            seq.append(("ADC", "F0" if rng.random() < 0.75 else "Z0", None if rng.random() < 0.6 else float(rng.uniform(0, 360))))
        if extra and r < 0.1:
            seq += extra
    return seq + [("ADC",), ("ADC", "Z0")]


def stops_train(T1, T2, B1, extra):
    """an echo train with S(-1), SPOILER, RESET, PD with and without reset and Z0 probes inside"""
    exc = ("T", 90 * B1, 90.0)
    pd = np.linspace(0.6, 0.9, np.size(T1)).reshape(np.shape(T1))
    return ([exc] + echoes(T1, T2, B1, extra, 10) + [("S", -1), ("ADC", "Z0"), ("ADC", "F0", 40.0), ("SPOILER",), ("ADC",), ("ADC", "Z0")]
            + echoes(T1, T2, B1, extra, 6, alpha=120.0) + [("RESET",), ("ADC", "Z0"), exc] + echoes(T1, T2, B1, extra, 8)
            + [("PD", pd), exc] + echoes(T1, T2, B1, extra, 12, alpha=160.0) + [("PD", 0.8, False), ("E", 3.0, T1, T2, 0), ("ADC", "Z0"), ("ADC",)])


def mixed(T1, T2, B1, extra, diffusion=True, dense=True):
    """what only run_kernel takes: shifts by |n| >= 2 (staged through LDS), 1-D diffusion, a combined operator E . T . E (one
    general-matrix record), R and P records; F0 / Z0 probes on the way.  `dense` = False: the combined operator is a product of two
    rotations -- E . T . E over (T1, T2) x B1 would be a table over the dense grid, a third index space"""
    e, t = ("E", 2.0, T1, T2, 0.01), ("T", 50 * B1, 35.0)
    first = [e, t, e] if dense else [t, ("T", 25 * B1, -70.0)]
    seq = [("T", 60 * B1, 20.0), ("S", 2), ("E", 3.0, T1, T2, 0), ("C", first), ("S", 1), ("ADC",), ("ADC", "Z0")]
    if diffusion:
        seq.append(("D", 0.5, 1e-3))
    seq += [("S", -3), ("R", 0.05 + 0.2j, 0.02, 0.03), ("P", 1.5, 0.02), ("T", 110 * B1, -40.0), ("S", 2)] + extra + [("ADC",), ("ADC", "Z0", 25.0)]
    seq += [("C", [t, e] if dense else [t, t]), ("S", 3), ("E", 2.0, T1, T2, 0), ("T", 35 * B1, 80.0), ("S", -2), ("ADC",), ("S", 4), ("T", 80 * B1, 10.0), ("S", -1), ("ADC",)]
    return seq


def ops_of(tuples):
    """oracle tuples -> product operators; one operator object per tuple object (echo trains repeat theirs)"""
    from epgpy_amd import epg
    made, ops = {}, []

    def one(t):
        kind, args = t[0], t[1:]
        if kind == "T":
            return epg.T(args[0], args[1])
        if kind == "E":
            return epg.E(*args)
        if kind == "P":
            return epg.P(*args)
        if kind == "R":
            return epg.R(args[0], args[1], r0=args[2])
        if kind == "S":
            return epg.S(args[0])
        if kind == "D":
            return epg.D(args[0], args[1])
        if kind == "ADC":
            what, phase = (args[0] if args else "F0"), (args[1] if len(args) > 1 else None)
            return epg.ADC if (what == "F0" and phase is None) else epg.Adc(what, phase=phase)
        if kind == "PD":
            return epg.PD(args[0], reset=(len(args) < 2 or args[1]))
        if kind == "C":
            op = one(args[0][0])
            for f in args[0][1:]:
                op = op @ one(f)
            return op
        return {"SPOILER": epg.SPOILER, "RESET": epg.RESET}[kind]

    for t in tuples:
        if id(t) not in made:
            made[id(t)] = one(t)
        ops.append(made[id(t)])
    return ops


def random_half_state(seed, grid, nstate, K):
    """a valid start state (F-(k) = conj F+(-k), Z(-k) = conj Z(k)) up to order `nstate`, amplitudes decaying with the order as
    a train's do: (half [nvox, 3, K] for DeviceState.upload, full [*grid, 2 nstate + 1, 3] for the recurrence)"""
    rng = np.random.default_rng(seed)
    nvox = int(np.prod(grid))
    fall = 0.3 * np.exp(-np.abs(np.arange(-nstate, nstate + 1)) * (6.0 / max(nstate, 1)))
    fp = (rng.uniform(-1, 1, (nvox, 2 * nstate + 1)) + 1j * rng.uniform(-1, 1, (nvox, 2 * nstate + 1))) * fall
    z = (rng.uniform(-1, 1, (nvox, nstate + 1)) + 1j * rng.uniform(-1, 1, (nvox, nstate + 1))) * fall[nstate:]
    z[:, 0] = z[:, 0].real
    full = np.zeros((nvox, 2 * nstate + 1, 3), dtype=np.complex128)
    full[:, :, 0] = fp
    full[:, :, 1] = fp[:, ::-1].conj()
    full[:, nstate:, 2] = z
    full[:, :nstate, 2] = z[:, :0:-1].conj()
    half = np.zeros((nvox, 3, K), dtype=np.complex128)
    for c in range(3):
        half[:, c, : nstate + 1] = full[:, nstate:, c]
    return half, full.reshape(tuple(grid) + full.shape[1:])


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}
KNOBS = {"EPGX_CGROW": "0", "EPGX_SPLIT_GROW": "0", "EPGX_ROWS": "0"}      # the child process of the cases marked `child` (at K = 128 the
# rows kernel would take the launch next)


def case(name, group, tuples, kernel, K, *, cap=None, start=None, out=False, kvalue=None, child=False, ref=None):
    """start: order up to which a random start state is filled (uploaded: HAS_IN); out: a state output, compared per order;
    child: runs in the child process with KNOBS; ref: the case whose reference this one shares (same inputs, another kernel)"""
    assert name not in CASES, name
    CASES[name] = dict(group=group, tuples=tuples, kernel=kernel, K=K, cap=cap, start=start, out=out, kvalue=kvalue, child=child,
                       ref=ref or name, seed=len(CASES))


def kn(nsp):
    return 4 if nsp > 2 else nsp


def tf(flag):
    return "true" if flag else "false"


def small_grid(nsp, rows):
    """voxel counts: the smallest that exercise the lane layout -- four voxels per wavefront: 7 (6 on two axes): a full group and
    a ragged one; one wavefront per voxel: 3 (2 x 2 on two axes)"""
    if nsp == 1:
        return 7 if rows else 3
    return (3, 2) if rows else (2, 2)


def _define():
    # (a) rows_kernel<NSP, R, RUNS>: R = K / 16 orders per lane.  RUNS: runs of identical records of length 1, 2 and long;
    # not RUNS: sequences with nothing to fold.  At K = 64 the run-length list goes to rows_grow_kernel unless fewer than a
    # tenth of the record executions run below 64 orders: 340 echoes.  At K = 128 the growing kernel takes trains with 60 % of
    # the records below 64 orders: 100 echoes have 32.  Truncation at K - 1 in the trains with runs (a record that truncates below
    # K - 1 is not folded into a run: such a train goes to RUNS = false) and below K - 1 in the others.
    for nsp in (1, 2, 3):
        t = tissue(nsp, 100 + nsp, small_grid(nsp, True))
        case(f"a_16_runs_{nsp}", "a", runs_train(*t, 17), f"rows_kernel<{kn(nsp)}, 1, true>", 16, cap=15)
        case(f"a_16_plain_{nsp}", "a", irregular(*t, 70, 10 + nsp), f"rows_kernel<{kn(nsp)}, 1, false>", 16, cap=(12, 15, 9)[nsp - 1])
        case(f"a_32_runs_{nsp}", "a", runs_train(*t, 27), f"rows_kernel<{kn(nsp)}, 2, true>", 32, cap=31)
        case(f"a_32_plain_{nsp}", "a", irregular(*t, 130, 20 + nsp), f"rows_kernel<{kn(nsp)}, 2, false>", 32, cap=(31, 22, 28)[nsp - 1])
        case(f"a_64_runs_{nsp}", "a", cpmg(*t, 340, tau=0.25), f"rows_kernel<{kn(nsp)}, 4, true>", 64, cap=63)
        case(f"a_64_plain_{nsp}", "a", irregular(*t, 150, 30 + nsp), f"rows_kernel<{kn(nsp)}, 4, false>", 64, cap=(40, 63, 33)[nsp - 1])
        case(f"a_128_{nsp}", "a", cpmg(*t, 100), f"rows_kernel<{kn(nsp)}, 8, false>", 128, cap=(100, 127, 126)[nsp - 1])
    # (b) rows_grow_kernel<NSP>: phases of 16 / 32 / 64 orders per voxel; n echoes populate 2 n orders: both sides of each phase
    # cut, a train whose tail narrows again through the reach rule, S(-1) / SPOILER / RESET / PD / Z0 inside, 60 decaying echoes
    for necho, nsp in [(7, 1), (8, 2), (9, 3), (15, 3), (16, 1), (17, 2), (40, 3)]:
        t = tissue(nsp, 200 + necho, small_grid(nsp, True))
        case(f"b_echo_{necho}", "b", cpmg(*t, necho, tau=2.5), f"rows_grow_kernel<{kn(nsp)}>", 64, cap=63)
    for nsp in (1, 2, 3):
        t = tissue(nsp, 250 + nsp, small_grid(nsp, True))
        case(f"b_stops_{nsp}", "b", stops_train(*t), f"rows_grow_kernel<{kn(nsp)}>", 64, cap=63)
    t = tissue(1, 260, 5, t2=(20.0, 60.0))
    case("b_decay_60", "b", cpmg(*t, 60, tau=2.5, alpha=180.0), "rows_grow_kernel<1>", 64, cap=63)
    # (c) run_contig_kernel<M, NSP, HAS_IN>, M = K / 64 consecutive orders per lane.  From a start state filled up to K - 10: three
    # echoes fill the orders up to K - 4, two more are truncated at K - 2, in the top register.  From equilibrium the growing
    # kernel takes these launches: the child process (EPGX_CGROW=0); K / 2 - 2 echoes fill the orders up to K - 4
    for K in (128, 256, 512, 1024):
        for nsp in (1, 2, 3):
            t = tissue(nsp, 300 + K + nsp, small_grid(nsp, False))
            case(f"c_{K}_in_{nsp}", "c", echoes(*t, 5), f"run_contig_kernel<{K // 64}, {kn(nsp)}, true>", K, cap=K - 2, start=K - 10)
            necho = K // 2 - 2 if (nsp == 1 or K <= 256) else 70
            case(f"c_{K}_eq_{nsp}", "c", cpmg(*t, necho), f"run_contig_kernel<{K // 64}, {kn(nsp)}, false>", K, child=True,
                 cap=None if necho == K // 2 - 2 else K - 1)
    # (d) run_contig_grow_kernel<M, NSP>: phases of 64, 128, 256, 512 orders per voxel; echo counts around 63, 127, 255, 511
    # populated orders (at K = 128 the kernel needs 60 % of the records below 64 orders: 32 of at most 53)
    for K in (128, 256, 512, 1024):
        for nsp, d in ((1, -1), (2, 0), (3, 1)):
            t = tissue(nsp, 400 + K + nsp, small_grid(nsp, False))
            case(f"d_{K}_{nsp}", "d", cpmg(*t, K // 4 + d), f"run_contig_grow_kernel<{K // 64}, {kn(nsp)}>", K)
    # (e) K = 2048, four wavefronts per voxel: 900 echoes reach 1800 orders, past the joins at 512, 1024 and 1536 (two voxels: the reference costs seconds per voxel),
    # 300 echoes 600 orders on two and three index spaces; in two legs, and -- the child process, EPGX_SPLIT_GROW=0 -- in one
    for nsp, necho in ((1, 900), (2, 300), (3, 300)):
        t = tissue(nsp, 500 + nsp, 2 if nsp == 1 else (2, 2))
        seq = cpmg(*t, necho)
        case(f"e_legs_{nsp}", "e", seq, f"run_kernel<8, {kn(nsp)}, false> + run_split_kernel<4, {kn(nsp)}, true>", 2048)
        case(f"e_split_{nsp}", "e", seq, f"run_split_kernel<4, {kn(nsp)}, false>", 2048, child=True, ref=f"e_legs_{nsp}")
    # (f) run_kernel<M, NSP, HAS_IN> with a state output, records and orders: from equilibrium (the orders above the few the
    # sequence reaches stay zero up to K) and from a start state filled up to K - 12, truncated at K - 1
    for K in (64, 128, 256, 512, 1024):
        for nsp in (1, 2, 3):
            t = tissue(nsp, 600 + K + nsp, small_grid(nsp, False))
            case(f"f_{K}_eq_{nsp}", "f", mixed(*t, dense=nsp != 2), f"run_kernel<{K // 64}, {kn(nsp)}, false>", K, out=True, kvalue=3e3)
            case(f"f_{K}_in_{nsp}", "f", mixed(*t, diffusion=nsp != 2, dense=nsp != 2), f"run_kernel<{K // 64}, {kn(nsp)}, true>", K, out=True, start=K - 12, cap=K - 1,
                 kvalue=1e3)


_define()

# every name choose_kernel returns for a plan without derivative states (V = 0) that the launch tables instantiate
ALL_NAMES = sorted(
    [f"rows_kernel<{n}, {r}, {tf(runs)}>" for n in (1, 2, 4) for r in (1, 2, 4, 8) for runs in (True, False) if not (runs and r == 8)]
    + [f"rows_grow_kernel<{n}>" for n in (1, 2, 4)]
    + [f"run_contig_kernel<{m}, {n}, {tf(i)}>" for m in (2, 4, 8, 16) for n in (1, 2, 4) for i in (True, False)]
    + [f"run_contig_grow_kernel<{m}, {n}>" for m in (2, 4, 8, 16) for n in (1, 2, 4)]
    + [f"run_split_kernel<4, {n}, false>" for n in (1, 2, 4)]
    + [f"run_kernel<8, {n}, false> + run_split_kernel<4, {n}, true>" for n in (1, 2, 4)]
    + [f"run_kernel<{m}, {n}, {tf(i)}>" for m in (1, 2, 4, 8, 16) for n in (1, 2, 4) for i in (True, False)])


def grid_of_case(c):
    from tests.signal_recurrence import signal_grid
    return signal_grid(c["tuples"])


def options_of(c):
    return {**({"max_nstate": c["cap"]} if c["cap"] else {}), **({"kvalue": c["kvalue"]} if c["kvalue"] else {})}


def start_of(c):
    """(half, full) of the case's start state, or None"""
    if c["start"] is None:
        return None
    return random_half_state(1000 + c["seed"], grid_of_case(c), c["start"], c["K"])


def reference(name, oracle=False):
    """(records, final state) of a case in extended precision (oracle: the float64 oracle's)"""
    from tests.signal_recurrence import signal_recurrence, oracle_signal
    c = CASES[name]
    start = start_of(c)
    fn = oracle_signal if oracle else signal_recurrence
    return fn(c["tuples"], shape=grid_of_case(c), max_nstate=c["cap"], init=None if start is None else start[1],
              kvalue=c["kvalue"] or 1.0, return_state=True)


def launch(c, want_name=None):
    """one plan through _lib.run at the case's capacity: ask for the kernel, hand its name to `want_name` BEFORE the launch,
    launch, download -> (name, records [record, *grid], half state [*grid, 3, K] or None)"""
    from epgpy_amd import _lib
    from epgpy_amd import functions as _functions
    grid, K = grid_of_case(c), c["K"]
    start = start_of(c)
    enc, _, _ = _functions.compile_sequence(ops_of(c["tuples"]), shape=grid, options=options_of(c),
                                            nstate0=c["start"] or 0, dense_start=start is not None)
    assert enc.grid == tuple(grid), (enc.grid, grid)
    assert enc.peak + 1 <= K, (enc.peak, K)                          # the capacity holds every order the plan can populate
    ctx = _lib.get_context(0)
    plan = enc.device_plan(ctx, K)
    nvox = enc.nvox
    state = None
    if start is not None or c["out"]:
        state = _lib.DeviceState(ctx, nvox, K)
        # (an output alone: filled with a value no order may keep -- the launch writes all K orders)
        state.upload(start[0] if start is not None else np.full((nvox, 3, K), 7.0 + 7.0j), np.ones(nvox))
    s_in, s_out = (state if start is not None else None), (state if c["out"] else None)
    name = _lib.kernel_for(ctx, plan, K, state_in=s_in, state_out=s_out)
    if want_name is not None:
        want_name(name)                                              # BEFORE the launch
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, nvox, s_in, s_out, K, sig.ptr.value, nvox, 0)
    records = sig.download(np.complex128, (enc.n_adc,) + tuple(grid))
    # (the kernels record the raw F0 / Z0; a probe's phase is applied on the host, as simulate() does, in complex128)
    phases = [t[2] if len(t) > 2 else None for t in c["tuples"] if t[0] == "ADC"]
    assert len(phases) == enc.n_adc
    for r, ph in enumerate(phases):
        if ph is not None:
            records[r] *= np.exp(1j * np.pi * ph / 180)
    half = state.download()[0].reshape(tuple(grid) + (3, K)) if c["out"] else None
    return name, records, half


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import signal_cases as me             # (the module under its package name: one CASES table)

    res = {}
    for case_name in sys.argv[2:]:
        cc = me.CASES[case_name]

        def exact(name, want=cc["kernel"]):
            assert name == want, (name, want)

        res[case_name] = me.launch(cc, exact)[1]
    np.savez(sys.argv[1], **res)
