"""CPU: what a one-pair second-order pass hands to epgx_plan_create -- the cross-term bits (epgx_dop::reserved), the combined
second-order tables and the pass list -- derived by the static walk over the sequence (diff.hessian_terms, Encoder.alive), and
the launch planner's side of it (tests/host/planner_hess_check.cpp).  No device involved."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from epgpy_amd import epg, _lib, _build, diff, functions, transition
from tests import hessian_cases as hc
from tests import sequences as sq

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
A, B = _lib.HESS_CROSS_A, _lib.HESS_CROSS_B


def compile_pass(seq, a, b, **options):
    a, b = diff.Pair(a, b)
    variables = [a, diff.hessian_key(a, b)] if a == b else [a, b, diff.hessian_key(a, b)]
    enc, records, _ = functions.compile_sequence(seq, None, options=options, variables=variables, fuse=False, collapse=False,
                                                 hessian=(a, b))
    arrays = enc.plan_arrays(enc.capacity())
    return enc, arrays


def bits_of(arrays):
    """per operator that can carry partials (T / E): (opcode letter, cross bits, [slot filled?])"""
    out = []
    for op, dop in zip(arrays["ops"], arrays["dops"]):
        if op["opcode"] in (_lib.OP_T, _lib.OP_E):
            out.append(("T" if op["opcode"] == _lib.OP_T else "E", int(dop["reserved"]), [int(o) >= 0 for o in dop["coef_off"]]))
    return out


def grid_sequence():
    return next((seq, opts) for name, seq, _, opts in sq.hessian_cases(epg) if name == "grid")


def test_grid_case_selects_cross_terms_per_operator():
    """G13 "grid": rf declares (b1, T2) and so does rl -- pair (T2, b1): (dE/dT2) S_b1 at every rl (b1 is alive from the first
    pulse on), (dT/db1) S_T2 at the second and third rf; neither operator has a second-order table for this pair"""
    seq, opts = grid_sequence()
    enc, arrays = compile_pass(seq, "b1", "T2", **opts)
    assert enc.variables == ["T2", "b1", ("order2", "T2", "b1")]
    assert arrays["n_vars"] == 3 and arrays["deriv_flags"] & _lib.DERIV_SECOND and arrays["deriv_flags"] & _lib.PLAN_NO_FOLD
    assert arrays["fuse"] is None and arrays["fuse_partial"] is None and "chain" not in arrays
    assert bits_of(arrays) == [("T", 0, [False, True, False]), ("E", A, [True, False, False]),
                               ("T", B, [False, True, False]), ("E", A, [True, False, False]),
                               ("T", B, [False, True, False]), ("E", A, [True, False, False])]
    # every probe owns four rows
    assert [int(op["ia"]) for op in arrays["ops"] if op["opcode"] == _lib.OP_ADC] == [0, 4, 8] and arrays["n_adc"] == 12


def test_a_pair_missing_from_an_operators_order2_takes_no_cross_term_there():
    """tests/hessian_cases.py "h_select": the relaxation does not list (b1, T2) -- its cross term must be absent"""
    seq = hc.ops_of(hc.CASES["h_select"]["tuples"])
    _, arrays = compile_pass(seq, "T2", "b1")
    got = bits_of(arrays)
    assert all(bits == 0 for kind, bits, _ in got if kind == "E")
    assert [bits for kind, bits, _ in got if kind == "T"] == [0] + [B] * 5


def test_diagonal_pair_second_order_table_and_doubled_cross_term():
    """pair (b1, b1) with order1 = {"b1": {"alpha": 35}}: slot 0 = 35 dT/dalpha, slot 1 = 35^2 d2T/dalpha^2 (a parameter pair
    counts once), the doubled cross term from the second pulse on; the relaxation carries nothing"""
    seq, opts = grid_sequence()
    enc, arrays = compile_pass(seq, "b1", "b1", **opts)
    assert arrays["n_vars"] == 2 and enc.variables == ["b1", ("order2", "b1", "b1")]
    got = bits_of(arrays)
    assert got == [("T", 0, [True, True, False]), ("E", 0, [False, False, False]), ("T", A, [True, True, False]),
                   ("E", 0, [False, False, False]), ("T", A, [True, True, False]), ("E", 0, [False, False, False])]
    rf = seq[0]
    want = diff.pack_matrix_partial(transition.rotation_partials2(rf.alpha, rf.phi)[("alpha", "alpha")]) * 35.0 ** 2
    dop = next(d for op, d in zip(arrays["ops"], arrays["dops"]) if op["opcode"] == _lib.OP_T)
    off = int(dop["coef_off"][1])
    assert np.allclose(arrays["coef"][off:off + 10], want.reshape(-1), rtol=1e-15, atol=0)
    assert [int(op["ia"]) for op in arrays["ops"] if op["opcode"] == _lib.OP_ADC] == [0, 3, 6]


def test_order2_coefficients_enter_the_second_order_table():
    """order2 = {pair: {parameter: c}}: the table is c dOp/dparameter + c1 c2 d2Op/dp1 dp2"""
    rf = epg.T(30.0, 10.0, order1={"x": {"alpha": 2.0}}, order2={("x", "x"): {"alpha": 0.5, "phi": -3.0}})
    tab = rf._second_table("x", "x")
    first = rf._partial_tables({"alpha", "phi"})
    second = diff.pack_matrix_partial(transition.rotation_partials2(rf.alpha, rf.phi)[("alpha", "alpha")])
    assert np.allclose(tab, 0.5 * first["alpha"] - 3.0 * first["phi"] + 4.0 * second, rtol=1e-14, atol=1e-18)
    assert rf._second_table("x", "y") is None
    bad = epg.T(30.0, 10.0, order1={"x": {"alpha": 2.0}}, order2={("x", "x"): {"alpha": np.array([1.0, 2.0])}})
    with pytest.raises(NotImplementedError, match="array-valued"):
        bad._second_table("x", "x")


def test_auto_cross_derivatives_follow_the_alive_variables():
    """the tutorial: order2="alpha" / "T2" (auto_cross_derivatives) -- pair (T2, alpha): (dT/dalpha) S_T2 at every pulse (a
    relaxation came first), (dE/dT2) S_alpha at every relaxation after the first pulse"""
    seq = next(seq for name, seq, _, _ in sq.hessian_cases(epg) if name == "tutorial")
    _, arrays = compile_pass(seq, "alpha", "T2")
    got = bits_of(arrays)
    assert got[0] == ("T", 0, [False, False, False])                 # the excitation declares nothing
    assert got[1] == ("E", 0, [True, False, False])                  # alpha is not alive yet
    assert [bits for kind, bits, _ in got[2:] if kind == "T"] == [B] * 6
    assert [bits for kind, bits, _ in got[2:] if kind == "E"] == [A] * 11


def test_operators_with_order1_alone_never_start_a_second_order_state():
    """the reference runs its order-2 step only once an operator declares order2 (DiffOperator.__call__): no cross bits"""
    rf, rl = epg.T(30.0, 0.0, order1="alpha"), epg.E(5.0, 1000.0, 80.0, order1="T2")
    _, arrays = compile_pass([rf, rl, epg.S(1), rf, rl, epg.ADC], "alpha", "T2")
    assert all(bits == 0 and not filled[2] for _, bits, filled in bits_of(arrays))
    # ... and take all of them once some operator has: here the first pulse's (alpha, alpha)
    rf2 = epg.T(30.0, 0.0, order2="alpha")
    _, arrays = compile_pass([rf2, rl, epg.S(1), rf, rl, epg.ADC], "alpha", "T2")
    assert [bits for _, bits, _ in bits_of(arrays)] == [0, A, B, A]


def test_passes_are_deduplicated_and_magnitude_rows_are_routed():
    _, seq, probes, _ = next(c for c in sq.hessian_cases(epg) if c[0] == "tutorial")
    passes = functions.hessian_passes(functions.flatten_sequence(seq), probes)
    assert passes == [("alpha", "alpha"), ("T2", "alpha"), ("T2", "T2")]
    layout = functions._HessianLayout(passes, 4 * 3 * 6, 3, (1,), 6)
    assert layout.first == {"alpha": (0, 1), "T2": (1, 1)}           # first-order rows: from the first pass that carries them
    assert layout.nrow(0) == 3 and layout.nrow(1) == 4 and layout.row(1, 2, 1, 3) == (2 * 3 + 1) * 4 + 3
    # "magnitude" partners no pass carries get a diagonal pass; variables no operator declares get none (zeros)
    passes = functions.hessian_passes(functions.flatten_sequence(seq), [epg.Hessian(["magnitude", "alpha"], ["T2", "zzz"])])
    assert passes == [("T2", "alpha")]
    passes = functions.hessian_passes(functions.flatten_sequence(seq), [epg.Hessian(["magnitude"], ["T2"]), epg.Jacobian(["alpha"])])
    assert passes == [("T2", "T2"), ("alpha", "alpha")]


def test_hessian_probes_are_refused_where_no_second_order_pass_is_compiled():
    """a Hessian has a device kind now: the paths that compile first-order or plain plans (compile_sequence without a pair --
    simulate_sharded's ShardedPlan among them) must refuse it, not record the plain signal in its place"""
    from epgpy_amd import distributed
    _, seq, probes, opts = next(c for c in sq.hessian_cases(epg) if c[0] == "tutorial")
    for pb in (probes, [epg.Hessian(["T2"], ["alpha"])], [epg.ADC, epg.Hessian("alpha", probe="Z0")]):
        with pytest.raises(NotImplementedError, match="Hessian"):
            distributed.ShardedPlan(seq, rank=0, world_size=1, probes=pb)
        with pytest.raises(NotImplementedError, match="Hessian"):
            functions.compile_sequence(seq, pb, variables=["alpha"])
    with pytest.raises(NotImplementedError, match="Hessian"):          # a Hessian standing in the sequence itself
        distributed.ShardedPlan(seq[:-1] + [epg.Hessian("alpha")], rank=0, world_size=2)
    with pytest.raises(NotImplementedError, match="Hessian"):
        distributed.simulate_sharded(seq, probe=probes, compute=lambda sp: None)
    distributed.ShardedPlan(seq, rank=0, world_size=1, probes=[epg.Jacobian(["alpha"])], variables=["alpha"])     # as before


def test_mode_auto_keeps_the_stepwise_path_and_the_probe_kind():
    assert epg.Hessian("T2")._device_kind() == epg.Jacobian("T2")._device_kind() is not None
    assert epg.Hessian("T2", probe="Z0")._device_kind() == epg.Jacobian("T2", probe="Z0")._device_kind()
    assert epg.Hessian("T2", probe="F")._device_kind() is None


def test_boundary_agrees():
    """include/epgx.h <-> _lib.py <-> INTEGRATION.md: the flag values of a second-order plan, the build unit"""
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    for name, value in [("EPGX_DERIV_SECOND", _lib.DERIV_SECOND), ("EPGX_HESS_CROSS_A", A), ("EPGX_HESS_CROSS_B", B),
                        ("EPGX_PLAN_NO_FOLD", _lib.PLAN_NO_FOLD), ("EPGX_DERIV_THROUGH_PLAIN_OPS", _lib.DERIV_THROUGH_PLAIN_OPS)]:
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert len({_lib.DERIV_SECOND, _lib.PLAN_NO_FOLD, _lib.DERIV_THROUGH_PLAIN_OPS}) == 3
    assert _lib.DOP_DTYPE.fields["reserved"][1] == 12 and _lib.DOP_DTYPE.itemsize == 40
    assert any(src == "epgx_hess.hip" for _, src, _ in _build.UNITS)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "EPGX_DERIV_SECOND" in doc and "hess_kernel" in doc
    assert _lib.HESS_MAX_K == 512 and _lib.max_vars(_lib.HESS_MAX_K) == 3 and _lib.max_vars(2 * _lib.HESS_MAX_K) < 3


def test_planner_names_hess_kernel(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "planner_hess_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", exe, os.path.join(HERE, "host", "planner_hess_check.cpp"),
                           os.path.join(ROOT, "epgpy_amd", "csrc", "epgx_planner.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.rstrip().endswith("planner_hess_check: all checks passed")
