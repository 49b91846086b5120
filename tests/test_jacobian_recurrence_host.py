"""CPU: the extended-precision Jacobian recurrence (tests/jacobian_recurrence.py) and the per-column check built on it.

  * it equals the float64 oracle to float64 rounding, column by column; the largest per-column error of a case is that
    case's FLOAT64 FLOOR -- what honest float64 arithmetic in the reference's order achieves.  FLOORS keeps them; the
    device tests (tests/test_gpu_jacobian_paths.py) hold every kernel to 16 x the floor of its case;
  * it is right independently of anyone's partial formulas: central differences of its own undifferentiated run;
  * the per-column check rejects errors that the whole-array `close` of tests/test_gpu_parity.py admits."""
import numpy as np
import pytest

from oracle import epg_numpy as onp
from tests import sequences as sq
from tests.jacobian_recurrence import jacobian_recurrence, grid_of, column_errors
from tests.jacobian_cases import FLOORS


def stock_cases():
    """name -> (tuples, variables without 'magnitude', options)"""
    rng = np.random.default_rng(777)
    T1, T2, B1 = rng.uniform(300, 2500, 9), rng.uniform(20, 300, 9), rng.uniform(0.7, 1.3, 9)
    T2b = np.linspace(40, 120, 7)
    out = {"jac_mse": (sq.jac_mse(T1, T2, B1, 12), {}),
           "jac_long": (sq.jac_long(T1[:3], T2[:3], B1[:3], 70), {}),
           "jac_spgr": (sq.jac_spgr(58.5 * np.arange(12) ** 2, np.linspace(-0.03, 0.03, 5)[None, :], T2b), {"max_nstate": 20}),
           "jac_params": (sq.jac_params(), {}),
           "jac_plain_ops": (sq.jac_plain_ops(T2b), {}),
           "jac_plain_ops_exact": (sq.jac_plain_ops(T2b), {"through_plain": True})}
    return {name: (tuples, [v for v in variables if v != "magnitude"], kw) for name, ((tuples, _, variables), kw) in out.items()}


def device_cases():
    """every case of tests/test_gpu_jacobian_paths.py: a start state enters as the operators that prepare it"""
    from tests import jacobian_cases as paths
    out = {}
    for name, c in paths.CASES.items():
        kw = {"max_nstate": c["cap"], "through_plain": c["exact"], **({"kvalue": c["kvalue"]} if c["kvalue"] else {})}
        plain = [t[:-1] if isinstance(t[-1], dict) else t for t in c["tuples"]]
        out[name] = (paths.full_tuples(c), c["variables"], dict(kw, shape=grid_of(plain)))
    for name, (tuples, variables, kw) in paths.g_cases().items():
        out[name] = (tuples, variables, kw)
    return out


def all_cases():
    return {**stock_cases(), **device_cases()}


def measure_floor(tuples, variables, kw):
    want = jacobian_recurrence(tuples, variables, probe="F0", **kw)
    if any(t[0] == "D" for t in tuples):      # the oracle's derivative driver has no diffusion: the same recurrence in float64
        got = jacobian_recurrence(tuples, variables, probe="F0", dtype=np.complex128, **kw)
    else:
        got = onp.simulate_jacobian(tuples, ["magnitude"] + list(variables), **kw)
    return max(column_errors(got, want, zero_atol=1e-17))


@pytest.mark.parametrize("name", list(all_cases()))
def test_recurrence_equals_oracle_to_float64_rounding(name):
    tuples, variables, kw = all_cases()[name]
    floor = measure_floor(tuples, variables, kw)
    print(name, "float64 floor", floor)
    assert floor <= FLOORS[name], (name, floor)
    assert 16 * FLOORS[name] <= 1e-11, name


def test_floor_table_names_every_case():
    assert set(FLOORS) == set(all_cases())


def test_start_state_equals_its_preparation():
    """init= (zero partials) against the same operators in front of the sequence"""
    from tests import jacobian_cases as paths
    c = paths.CASES["b_128_2_1"]
    grid = grid_of([t[:-1] if isinstance(t[-1], dict) else t for t in c["tuples"]])
    whole = jacobian_recurrence(paths.full_tuples(c), c["variables"], probe="F0", shape=grid)
    n = sum(abs(t[1]) for t in c["head"] if t[0] == "S")
    # the state after the head, from a run that records nothing: rebuilt here from a probe-free restatement
    head_state = _state_after(c["head"], grid, n)
    assert np.abs(head_state[..., -1, 0]).max() > 0          # the top order is populated
    assert np.abs(head_state[..., n + n // 2:, :]).max() > 0
    parts = jacobian_recurrence(c["tuples"], c["variables"], probe="F0", shape=grid, init=head_state)
    assert max(column_errors(parts.astype(np.complex128), whole)) <= 1e-14


def _state_after(head, grid, n):
    """float64 state matrix [*grid, 2 n + 1, 3] after the plain operators `head` (the oracle's own driver)"""
    _, states = onp.simulate(list(head) + [("ADC",)], shape=grid, return_states=True)
    assert states.shape[-2] == 2 * n + 1
    return states


# ------------------------------------------------------------------------------------------------ finite differences
def _fd_sequence(p):
    """every differentiable parameter kind once, as a function of the parameter vector; no plain operators"""
    T2 = np.array([40.0, 70.0, 110.0]) * p["T2"] / 70.0
    e_o1 = {"tau": {"tau": 1}, "T1": {"T1": 1}, "T2s": {"T2": T2 / p["T2"]}, "g": {"g": 1}}
    return [("T", p["alpha"], p["phi"], {"order1": True}), ("E", p["tau"], p["T1"], T2, p["g"], {"order1": e_o1}), ("ADC",), ("ADC", "Z0"),
            ("S", 1), ("P", p["ptau"], p["pg"], {"order1": {"ptau": {"tau": 1}, "pg": {"g": 1}}}),
            ("R", p["rT"] + 0.3j, p["rL"], p["r0"], {"order1": ["rT", "rL", "r0"]}),
            ("T", 1.3 * p["alpha"], -30.0, {"order1": {"alpha": {"alpha": 1.3}}}), ("S", 1), ("ADC",), ("ADC", "Z0"),
            ("S", -2), ("T", 40.0, p["phi"] + 15.0, {"order1": {"phi": "phi"}}), ("S", 2), ("ADC",),
            ("SPOILER",), ("E", p["tau"] / 2, p["T1"], T2, 0, {"order1": {"tau": {"tau": 0.5}, "T1": "T1"}}),
            ("T", 0.5 * p["alpha"], 10.0, {"order1": {"alpha": {"alpha": 0.5}}}), ("ADC",), ("ADC", "Z0")]


FD_POINT = {"alpha": 60.0, "phi": 20.0, "tau": 4.0, "T1": 700.0, "T2": 70.0, "g": 0.02, "ptau": 3.0, "pg": -0.015, "rT": 0.1, "rL": 0.2, "r0": 0.25}
# parameter -> the variable that collects it (T2 enters as a per-voxel array with per-voxel coefficients)
FD_VARS = {"alpha": "alpha", "phi": "phi", "tau": "tau", "T1": "T1", "T2": "T2s", "g": "g", "ptau": "ptau", "pg": "pg", "rT": "rT", "rL": "rL", "r0": "r0"}


@pytest.mark.parametrize("param", list(FD_POINT))
def test_recurrence_against_central_differences(param):
    """h = 1e-7 |p|: truncation ~ h^2 and rounding ~ 1e-19 / h are both ~ 1e-12 relative; bound 1e-9 of the column's maximum,
    for F0 and Z0 probes (through_plain=True: the spoiler acts on the derivative states, as it does on the perturbed signal)"""
    seq = _fd_sequence
    var = FD_VARS[param]
    for probe in (None, "F0", "Z0"):
        jac = jacobian_recurrence(seq(FD_POINT), [var], probe=probe, through_plain=True)
        h = np.longdouble(1e-7) * abs(FD_POINT[param])
        up = jacobian_recurrence(seq(dict(FD_POINT, **{param: FD_POINT[param] + h})), [], probe=probe, through_plain=True)
        dn = jacobian_recurrence(seq(dict(FD_POINT, **{param: FD_POINT[param] - h})), [], probe=probe, through_plain=True)
        fd = (up[..., 0] - dn[..., 0]) / (2 * h)
        scale = np.max(np.abs(fd))
        if param == "phi" and probe == "Z0":     # Z0 does not depend on the RF phase: both hold rounding only (1e-19 / h)
            assert scale < 1e-12 and np.max(np.abs(jac[..., 1])) < 1e-15
            continue
        assert scale > 1e-6
        assert np.max(np.abs(jac[..., 1] - fd)) <= 1e-9 * scale, (param, probe)


# ------------------------------------------------------------------------------------------------ the check bites
def test_per_column_check_bites_where_close_does_not():
    from tests.test_gpu_parity import close
    from tests.jacobian_cases import check
    rng = np.random.default_rng(777)                 # the seeded grid of test_gpu_parity.test_jacobian_vs_oracle, its checked slice
    T1, T2, B1 = rng.uniform(300, 2500, 777), rng.uniform(20, 300, 777), rng.uniform(0.7, 1.3, 777)
    tuples, _, variables = sq.jac_mse(T1[:64], T2[:64], B1[:64], necho=12)
    variables = variables[1:]
    want = jacobian_recurrence(tuples, variables, probe="F0")
    good = want.astype(np.complex128)
    floor = FLOORS["jac_mse"]
    check("host", good, want, floor)
    t1, t2 = 1 + variables.index("T1"), 1 + variables.index("T2")
    wrong_column = good.copy()
    wrong_column[..., t1] *= 1 + 1e-9
    wrong_entry = good.copy()
    # one entry at the highest record: the largest that the whole-array bound still admits (1e-9 of it below 1e-12 max|J|)
    last = np.abs(good[-1, :, t2])
    vox = int(np.argmax(np.where(last <= 1e-3, last, 0.0)))
    assert last[vox] > 1e-4
    wrong_entry[-1, vox, t2] *= 1 + 1e-9
    for bad in (wrong_column, wrong_entry):
        close(bad, good, 1e-12)                      # the whole-array bound admits both
        with pytest.raises(AssertionError):
            check("host", bad, want, floor)
    from tests.jacobian_cases import MEASURED
    MEASURED.pop("host", None)
