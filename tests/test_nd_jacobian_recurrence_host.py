"""CPU: the extended-precision n-D derivative recurrence (tests/nd_jacobian_recurrence.py), the case table built on it
(tests/nd_jacobian_cases.py) and the host planner behind gather shifts and diffusion of derivative plans.

  * reduction: with no variables the recurrence returns nd_recurrence's records bit for bit on every case;
  * 1-D agreement: on sequences that shift by int S(+-1) / S(+-2) and diffuse in 1-D it agrees with tests/jacobian_recurrence.py
    (which shares only the closed forms) to 64 eps of np.clongdouble per column;
  * definition: on every case with exact=True column 1 + v agrees with a central finite difference of the plain nd_recurrence
    to 1e-9 of the column's maximum; with exact=False the same difference DISAGREES on the D cases by far more than the bound;
  * FLOORS is honest: measured <= table <= 2 x measured and 16 x floor <= the cap, every case has a floor;
  * every case matches its table (capacity, rows, NSP, kernel name) and the names cover what the device test must launch;
  * no derivative column is vacuous;
  * a NumPy emulation of gather_shift / apply_D on the state AND on V derivative half-states, driven by the tables
    compile_sequence emits for the derivative plan, reproduces the recurrence on every case to the case's bound; the
    mutations (i) to (v) each break at least one named case, (vi) the near-full case of every M = 2, 4, 8, 16."""
import numpy as np
import pytest

from epgpy_amd import _lib
from tests import nd_cases as nc, nd_jacobian_cases as jc
from tests.jacobian_recurrence import _Arith, _normalise, _rotation, _scalar, column_errors, jacobian_recurrence, SCALAR_PARAMS, T_PARAMS
from tests.nd_jacobian_recurrence import nd_jacobian_recurrence, strip
from tests.nd_recurrence import nd_recurrence
from tests.signal_recurrence import half_of
from tests.test_nd_recurrence_host import emulate as plain_emulate

CASES = jc.CASES
G = jc.g_cases()
_REF, _PLAN, _FLOOR = {}, {}, {}


def reference(name):
    if name not in _REF:
        _REF[name] = jc.reference(name)
    return _REF[name]


def g_reference(name, dtype=np.clongdouble):
    tuples, variables, grid, opts, exact = G[name]
    return nd_jacobian_recurrence(tuples, variables, shape=grid, kvalue=opts["kvalue"], max_nstate=opts.get("max_nstate"), through_plain=exact,
                                  dtype=dtype)


def plan_of(name):
    """(encoder, K, [table per S / D tuple, in order], stored coordinates, index spaces) of a case's derivative plan"""
    if name not in _PLAN:
        enc, K = jc.compile_case(CASES[name])
        tables = [build(K) for _, build in enc.deferred]
        rows = enc.kspace.nrow - enc.kspace.centre
        peak = enc.peak
        enc.plan_arrays(K)
        _PLAN[name] = (K, tables, rows, len(enc.spaces), peak)
    return _PLAN[name]


# ------------------------------------------------------------------------------------------------ reduction, 1-D agreement
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["twin"] is None] + list(G))
def test_without_variables_it_is_nd_recurrence_bit_for_bit(name):
    if name in G:
        tuples, _, grid, opts, _ = G[name]
        start = None
    else:
        c = CASES[name]
        tuples, grid, opts, start = c["tuples"], c["grid"], c["opts"], jc.start_of(c)
    kw = dict(shape=grid, kvalue=opts.get("kvalue", 1.0), max_nstate=opts.get("max_nstate"), init=start)
    got = nd_jacobian_recurrence(tuples, [], **kw)
    want = nd_recurrence(strip(tuples), **kw)
    assert got.shape == want.shape + (1,) and got.dtype == want.dtype
    assert np.array_equal(got[..., 0], want) and np.array_equal(np.signbit(got[..., 0].real), np.signbit(want.real))


@pytest.mark.parametrize("name", ["a_128_lds", "a_128_diffusion"])
def test_it_agrees_with_the_1d_recurrence(name):
    from tests import jacobian_cases as paths
    from tests.jacobian_recurrence import grid_of
    c = paths.CASES[name]
    grid = grid_of(strip(c["tuples"]))
    want = jacobian_recurrence(c["tuples"], c["variables"], probe="F0", max_nstate=c["cap"], through_plain=c["exact"], shape=grid,
                               kvalue=c["kvalue"] or 1.0)
    got = nd_jacobian_recurrence(c["tuples"], c["variables"], max_nstate=c["cap"], through_plain=c["exact"], shape=grid, kvalue=c["kvalue"] or 1.0)
    errs = column_errors(got, want)
    print(name, "against the 1-D recurrence, per column, in eps of clongdouble:", [float(e / np.finfo(np.clongdouble).eps) for e in errs])
    assert max(errs) <= 64 * np.finfo(np.clongdouble).eps


# ------------------------------------------------------------------------------------------------ the definition
PARAM_AT = {"T": {"alpha": 1, "phi": 2}, "E": {"tau": 1, "T1": 2, "T2": 3, "g": 4}}


def stepped(tuples, var, h):
    """the plain tuples with every parameter that `var` declares moved by h x its coefficient (in extended precision)"""
    out = []
    for t in tuples:
        if not isinstance(t[-1], dict):
            out.append(t)
            continue
        base = list(t[:-1])
        o1 = _normalise(t[-1]["order1"], T_PARAMS if t[0] == "T" else SCALAR_PARAMS[t[0]])
        for p, coeff in o1.get(var, {}).items():
            at = PARAM_AT[t[0]][p]
            base[at] = np.asarray(base[at], dtype=np.longdouble) + h * np.asarray(coeff, dtype=np.longdouble)
        out.append(tuple(base))
    return out


def finite_difference(c, var):
    h = np.longdouble(1e-6) * jc.NOMINAL[var]
    kw = dict(shape=c["grid"], kvalue=c["opts"].get("kvalue", 1.0), max_nstate=c["opts"].get("max_nstate"), init=jc.start_of(c))
    up = nd_recurrence(stepped(c["tuples"], var, h), **kw)
    dn = nd_recurrence(stepped(c["tuples"], var, -h), **kw)
    return (up - dn) / (2 * h)


FD_CASES = [n for n, c in CASES.items() if c["exact"]] + [n for n, g in G.items() if g[4]]


def fd_case(name):
    if name in G:
        tuples, variables, grid, opts, _ = G[name]
        return dict(tuples=tuples, variables=variables, grid=grid, opts=opts, start=None, seed=0), g_reference(name)
    return CASES[name], reference(name)


@pytest.mark.parametrize("name", FD_CASES)
def test_exact_partials_are_the_finite_difference_of_the_plain_recurrence(name):
    c, want = fd_case(name)
    worst = 0.0
    for v, var in enumerate(c["variables"]):
        fd = finite_difference(c, var)
        scale = float(np.max(np.abs(fd)))
        assert scale > 0
        err = float(np.max(np.abs(want[..., 1 + v] - fd))) / scale
        worst = max(worst, err)
    print(name, "largest |column - central difference| / max|column|", worst)
    assert worst <= 1e-9, (name, worst)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["group"] == "c" and not c["exact"]])
def test_default_partials_are_not_the_finite_difference_where_d_acts(name):
    """exact=False leaves the derivative states unattenuated: the flag is not vacuous on these cases"""
    c = CASES[name]
    want = reference(name)
    bound = jc.MARGIN * jc.FLOORS[name]
    worst = 0.0
    for v, var in enumerate(c["variables"]):
        fd = finite_difference(c, var)
        worst = max(worst, float(np.max(np.abs(want[..., 1 + v] - fd))) / float(np.max(np.abs(fd))))
    print(name, "exact=False against the central difference:", worst, "bound of the case", bound)
    assert worst > 1e4 * bound and worst > 1e-6, (name, worst)


# ------------------------------------------------------------------------------------------------ floors
def measured(name):
    if name not in _FLOOR:
        if name in G:
            _FLOOR[name] = max(column_errors(g_reference(name, np.complex128), g_reference(name)))
        else:
            _FLOOR[name] = max(column_errors(jc.reference(name, dtype=np.complex128), reference(name)))
    return _FLOOR[name]


@pytest.mark.parametrize("name", list(CASES) + list(G))
def test_floor_table_is_honest(name):
    floor = measured(name)
    print(name, "float64 floor", floor, "table", jc.FLOORS.get(name))
    assert np.isfinite(floor) and floor <= jc.FLOORS[name] <= 2 * floor, (name, floor, jc.FLOORS.get(name))
    assert jc.MARGIN * jc.FLOORS[name] <= jc.CAP, name


def test_every_case_has_a_floor():
    assert set(jc.FLOORS) == set(CASES) | set(G)


def measured_coordinates(name):
    from tests.nd_recurrence import layout
    from tests.signal_recurrence import order_errors
    c = CASES[name]
    want, got = jc.h_reference(name), jc.h_reference(name, np.complex128)
    worst = 0.0
    assert any(len(want[var]) > 3 for var in c["variables"])
    for var in c["variables"]:
        if not want[var]:          # (a variable that nothing declares after the last RESET: no derivative state is left)
            assert not got[var]
            continue
        coords = jc.table_coords(want[var])
        rows_w, rows_g = layout(want[var], coords, c["grid"]), layout(got[var], coords, c["grid"])
        worst = max(worst, max(order_errors(np.ascontiguousarray(half_of(rows_g)), rows_w)))
    return worst


@pytest.mark.parametrize("name", jc.H_CASES)
def test_coordinate_floors_are_honest(name):
    worst = measured_coordinates(name)
    print(name, "per-coordinate float64 floor of the final derivative states", worst, "table", jc.COORD_FLOORS.get(name))
    assert worst <= jc.COORD_FLOORS[name] <= 2 * worst and jc.MARGIN * jc.COORD_FLOORS[name] <= jc.COORD_CAP


def test_operator_by_operator_d_is_a_plain_operator():
    """what `exact` is through op(sm), read from the code: D has no derivative-aware __call__ (it is Operator.__call__), so it never
    touches sm.order1; S does, through diff.propagate_plain"""
    from epgpy_amd import diffusion, operator, shift, diff
    assert diffusion.D.__call__ is operator.Operator.__call__ and not issubclass(diffusion.D, diff.Jacobian.__mro__[0])
    assert shift.S.__call__ is not operator.Operator.__call__
    assert jc.H_EXACT is False
    groups = [CASES[n]["group"] for n in jc.H_CASES]
    assert groups == ["a", "c", "c", "e"] and [CASES[n]["exact"] for n in jc.H_CASES[1:3]] == [False, True]
    assert set(jc.COORD_FLOORS) == set(jc.H_CASES)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", list(CASES))
def test_plan_matches_the_case(name):
    c = CASES[name]
    K, _, rows, nspaces, peak = plan_of(name)
    assert K == c["K"], (K, c["K"])
    assert c["rows"] is None or rows == c["rows"], (rows, c["rows"])
    assert peak + 1 <= K
    assert (nspaces if nspaces <= 2 else 4) == c["nsp"], (nspaces, c["nsp"])
    assert c["kernel"] == f"deriv_kernel<{K // 64}, {c['nsp']}, {c['V']}>"
    assert c["V"] == len(c["variables"]) and (c["start"] is None) == (c["group"] != "d")
    if c["twin"]:
        assert CASES[c["twin"]]["tuples"] is c["tuples"] and c["exact"] and not CASES[c["twin"]]["exact"]


def test_names_cover_the_required_kernels():
    have = {(c["K"] // 64, c["nsp"], c["V"]) for c in CASES.values()}
    for M in (1, 2, 4, 8):
        assert {v for m, _, v in have if m == M} >= {1, 2, 3}, M
        assert {n for m, n, _ in have if m == M} >= {1, 2, 4}, M
    assert {(16, n, 1) for n in (1, 2, 4)} <= have
    voxels = {int(np.prod(c["grid"])) for c in CASES.values()} | {int(np.prod(g[2])) for g in G.values()}
    assert {1, 70} <= voxels and max(voxels) <= 70
    assert all(int(np.prod(c["grid"])) <= 6 for c in CASES.values() if c["group"] in "abcde")
    for M, name in jc.NEAR_FULL.items():
        assert CASES[name]["K"] == 64 * M and 4 * CASES[name]["rows"] > 3 * 64 * M


def test_group_a_tables_hold_conjugated_sources_on_both_sides_and_empty_ones():
    for name, c in CASES.items():
        if c["group"] != "a":
            continue
        K, tables, _, _, _ = plan_of(name)
        gs = [np.ascontiguousarray(t).view(np.int32).reshape(3, K) for t in tables if t.shape[-1] * 2 == 3 * K and t.shape[:-1] == (1,)]
        conj_a = any(((t[0] >= 0) & ((t[0] & _lib.GS_CONJ) != 0)).any() for t in gs)
        conj_b = any(((t[1] >= 0) & ((t[1] & _lib.GS_CONJ) != 0)).any() for t in gs)
        assert conj_a and conj_b and any((t[:, : 4] < 0).any() for t in gs), name


@pytest.mark.parametrize("name", list(CASES) + list(G))
def test_no_column_is_vacuous(name):
    want = g_reference(name) if name in G else reference(name)
    declared = set(jc.TRAIN_VARS)
    variables = G[name][1] if name in G else CASES[name]["variables"]
    assert np.all(np.isfinite(want.astype(np.complex128)))
    for v, var in enumerate(variables):
        col = np.abs(want[..., 1 + v])
        if var not in declared:
            assert not col.any()
            continue
        top = float(col.max())
        assert top > 0, (name, var)
        per_record = col.reshape(col.shape[0], -1).max(axis=1)
        assert np.all((per_record == 0) | (per_record >= 1e-9 * top)), (name, var, per_record.min(), top)
    if name == "c_strong_x":
        assert 0 < np.max(np.abs(want[-1, ..., 0])) < 1e-6 * np.max(np.abs(want[0, ..., 0]))


# ------------------------------------------------------------------------------------------------ the planner, emulated
def emulate(name, *, gather=True, conj_b=True, d_on=None, swap_mirror=False, zero_top=0):
    """the case's tuples on the device's half layout -- the state and V derivative half-states [*grid, 3, K] in extended
    precision, shifts and diffusion through the plan's tables alone -> records [record, *grid, 1 + V].  Mutations: gather=False
    (i) derivative states are not gathered; conj_b=False (ii) GS_CONJ ignored on the B side of derivative states; d_on (iii / iv)
    whether D acts on derivative states, whatever `exact` says; swap_mirror (v) bT and its mirror swapped on derivative states;
    zero_top=M (vi) slots 64 (M - 1) .. K - 1 of every derivative half-state zeroed at the sequence's midpoint"""
    c = CASES[name]
    grid, variables = c["grid"], c["variables"]
    K, tables, _, _, _ = plan_of(name)
    tables = iter(tables)
    ar = _Arith(grid, np.clongdouble)
    st = np.zeros(grid + (3, K), ar.cplx)
    dens = np.ones(grid, ar.real)
    start = jc.start_of(c)
    if start is None:
        st[..., 2, 0] = dens
    else:
        h = half_of(start[0])
        st[..., : h.shape[-1]] = h
    dst = {v: np.zeros(grid + (3, K), ar.cplx) for v in variables}
    d_acts = c["exact"] if d_on is None else d_on
    out = []

    def full(x):
        return np.broadcast_to(x, grid + (3, K)).astype(ar.cplx)

    def rotate(R, x):
        A, B, Z = x[..., 0, :], x[..., 1, :], x[..., 2, :]
        return np.stack([R[..., i, 0, None] * A + R[..., i, 1, None] * B + R[..., i, 2, None] * Z for i in range(3)], axis=-2)

    for at, (t, base) in enumerate(zip(c["tuples"], strip(c["tuples"]))):
        kind = base[0]
        if zero_top and at == len(c["tuples"]) // 2:
            for v in variables:
                dst[v] = dst[v].copy()
                dst[v][..., 64 * (zero_top - 1):] = 0
        if kind == "T":
            R, dR = _rotation(ar, base[1], base[2])
            o1 = _normalise(t[-1]["order1"], T_PARAMS) if isinstance(t[-1], dict) else {}
            for v in variables:
                new = rotate(R, dst[v])
                for p, coeff in o1.get(v, {}).items():
                    new = new + ar.real(coeff) * rotate(dR[p], st)
                dst[v] = full(new)
            st = rotate(R, st)
        elif kind in ("E", "P"):
            diag, rec, parts = _scalar(ar, kind, base[1:])
            o1 = _normalise(t[-1]["order1"], SCALAR_PARAMS[kind]) if isinstance(t[-1], dict) else {}
            for v in variables:
                new = np.stack([dst[v][..., j, :] * ar.rows(diag[j]) for j in range(3)], axis=-2)
                for p, coeff in o1.get(v, {}).items():
                    term = full(np.stack([st[..., j, :] * ar.rows(parts[p][0][j]) for j in range(3)], axis=-2))
                    term[..., 2, 0] += parts[p][1] * dens
                    new = new + ar.real(coeff) * term
                dst[v] = full(new)
            st = full(np.stack([st[..., j, :] * ar.rows(diag[j]) for j in range(3)], axis=-2))
            if rec is not None:
                st[..., 2, 0] += rec * dens
        elif kind == "S":
            tab = np.ascontiguousarray(next(tables)).view(np.int32).reshape(3, K)
            ia, ib, iz = tab[0], tab[1], tab[2]
            ca, cb = (ia & _lib.GS_CONJ) != 0, (ib & _lib.GS_CONJ) != 0
            ja, jb, jz = ia & (K - 1), ib & (K - 1), iz & (K - 1)

            def gathered(x, keep_b=True):
                A, B, Z = x[..., 0, :], x[..., 1, :], x[..., 2, :]
                na = np.where(ca, B[..., ja].conj(), A[..., ja])
                nb = np.where(cb, A[..., jb].conj() if keep_b else A[..., jb], B[..., jb])
                return np.stack([np.where(ia < 0, 0, na), np.where(ib < 0, 0, nb), np.where(iz < 0, 0, Z[..., jz])], axis=-2)

            st = gathered(st)
            if gather:
                dst = {v: gathered(d, conj_b) for v, d in dst.items()}
        elif kind == "D":
            tab = np.asarray(next(tables))
            tab = tab.reshape(tab.shape[:-1] + (3, K))
            tab = tab.reshape(tab.shape[:-2] + (1,) * (len(grid) - (tab.ndim - 2)) + (3, K)).astype(ar.real)
            st = st * tab
            if d_acts:
                dtab = tab[..., [1, 0, 2], :] if swap_mirror else tab
                dst = {v: d * dtab for v, d in dst.items()}
        elif kind == "ADC":
            col = 0 if (len(base) < 2 or base[1] == "F0") else 2
            out.append(np.stack([st[..., col, 0]] + [dst[v][..., col, 0] for v in variables], axis=-1))
        elif kind == "SPOILER":
            st = st.copy()
            st[..., :2, :] = 0
            if c["exact"]:
                for v in variables:
                    dst[v] = dst[v].copy()
                    dst[v][..., :2, :] = 0
        elif kind == "RESET":
            st = np.zeros_like(st)
            st[..., 2, 0] = dens
            dst = {v: np.zeros(grid + (3, K), ar.cplx) for v in variables}
        else:
            raise ValueError(kind)
        st = full(st)
        dst = {v: full(d) for v, d in dst.items()}
    assert next(tables, None) is None
    return np.stack(out)


def emulation_error(name, **mutation):
    return max(column_errors(emulate(name, **mutation), reference(name)))


@pytest.mark.parametrize("name", list(CASES))
def test_planner_tables_reproduce_the_recurrence(name):
    err = emulation_error(name)
    bound = jc.MARGIN * jc.FLOORS[name]
    print(name, "emulated derivative plan: largest per-column error", err, "bound", bound)
    assert err <= bound, (name, err, bound)


def test_the_emulation_extends_the_plain_one():
    """column 0 of the emulated derivative plan is the plain emulation of tests/test_nd_recurrence_host.py on the same tuples.
    The two plans differ -- a plan with variables keeps the rows a SPOILER empties, so its row set and gather tables are larger --
    but the extra rows hold zeros in the state, and column 0 comes out the same"""
    for mine, theirs in [("e_lead2_box", "f_lead2_box"), ("e_lead2_box_x", "f_lead2_box")]:
        records, _ = plain_emulate(theirs)
        got = emulate(mine)[..., 0]
        assert np.array_equal(got, records), mine


def test_a_derivative_plan_keeps_the_rows_a_spoiler_empties():
    """T S SPOILER T S: the F-only rows of the first shift are empty in the state after the SPOILER, but not in a derivative
    state that is not spoiled (the default): the gather table of the second shift of a plan with variables must still take dF
    from them, and the plan without variables must not"""
    from epgpy_amd import epg, functions as _functions
    o1 = {"order1": {"B1": {"alpha": 60.0}}}
    tuples = [("T", 60.0, 10.0, o1), ("S", [1, 0]), ("SPOILER",), ("T", 50.0, 20.0, o1), ("S", [0, 1]), ("ADC",)]

    def last_table(variables):
        enc, _, _ = _functions.compile_sequence(jc.ops_of(tuples if variables else strip(tuples)), variables=variables)
        rows = enc.kspace.nrow - enc.kspace.centre
        return rows, np.ascontiguousarray(enc.deferred[-1][1](64)).view(np.int32).reshape(3, 64)
    rows_v, tab_v = last_table(["B1"])
    rows_p, tab_p = last_table([])
    sources = lambda tab: int(np.count_nonzero(tab[0] >= 0) + np.count_nonzero(tab[1] >= 0))
    assert rows_v > rows_p and sources(tab_v) > sources(tab_p), (rows_v, rows_p, sources(tab_v), sources(tab_p))
    # the coordinate (1, 1): F moved there from (1, 0), which only the first shift populated
    want = nd_jacobian_recurrence(tuples + [("T", 40.0, 0.0, o1), ("S", [-1, -1]), ("ADC",)], ["B1"])
    assert np.abs(want[-1, ..., 1]).max() > 0


MUTATIONS = {
    "i": (dict(gather=False), ["a_64_61_1_3", "a_128_85_3_3", "b_545_1", "e_lead1"]),
    "ii": (dict(conj_b=False), ["a_64_61_1_3", "a_256_221_3_2", "c_scalar_k"]),
    "iii": (dict(d_on=True), ["c_scalar_k", "c_scalar", "c_tensor2", "e_lead1"]),
    "iv": (dict(d_on=False), ["c_scalar_k_x", "c_field_x", "c_tensor3_x", "c_strong_x", "f_70"]),
    "v": (dict(swap_mirror=True), ["c_scalar_k_x", "c_tensor2_x", "c_strong_x", "f_70"]),
}


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_mutations_of_the_emulation_fail(which):
    mutation, names = MUTATIONS[which]
    failed = [name for name in names if emulation_error(name, **mutation) > jc.MARGIN * jc.FLOORS[name]]
    print("mutation", which, mutation, "breaks", failed, "of", names)
    assert failed


@pytest.mark.parametrize("M", [2, 4, 8, 16])
def test_the_last_register_of_a_lane_reaches_a_probe(M):
    """mutation (vi): the near-full case of this M with slots 64 (M - 1) .. K - 1 of the derivative states zeroed half way"""
    name = jc.NEAR_FULL[M]
    err = emulation_error(name, zero_top=M)
    print("mutation vi, M =", M, name, "error", err, "bound", jc.MARGIN * jc.FLOORS[name])
    assert err > jc.MARGIN * jc.FLOORS[name], (name, err)
