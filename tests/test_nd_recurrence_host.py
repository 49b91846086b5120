"""CPU: the extended-precision n-D recurrence (tests/nd_recurrence.py), the case table built on it (tests/nd_cases.py) and the
host planner behind gather shifts and diffusion (epgpy_amd/kspace.py, diffusion.py).

  * the recurrence, run in complex128, reproduces oracle.simulate_nd(prune=False) and the goldens g12_nd / g14_nd_vector to
    rounding: signals, and states paired by coordinate;
  * FLOORS is honest: for every case at least the float64 oracle's largest per-record (per-coordinate) error against the
    recurrence, and at most twice it; 16 x floor stays within 2e-12;
  * a NumPy emulation of what gather_shift and apply_D do with their tables -- plain indexing, conjugation by the GS_CONJ bit,
    zero for negative entries, three real factors per order -- driven by the tables compile_sequence emits (the deferred builders,
    at the case's K), reproduces the recurrence on every case to the case's bound, records and every stored coordinate: that
    tests KSpace.shifted, bmatrices, structural pruning and the table layout without a GPU;
  * the emulation with the conjugate of one side flipped, or with bT and its mirror swapped, fails at least one case;
  * the conditions of tests/nd_cases.py hold for every case."""
import numpy as np
import pytest

from epgpy_amd import _lib
from oracle import epg_numpy as onp
from tests import nd_cases as nc, sequences as sq
from tests.jacobian_recurrence import _Arith, _rotation, _scalar
from tests.nd_recurrence import nd_recurrence, coord_keys
from tests.signal_recurrence import record_errors, order_errors, half_of

OWN = [name for name, c in nc.CASES.items() if c["ref"] == name]
_REF, _PLAN = {}, {}


def reference(name):
    if name not in _REF:
        _REF[name] = nc.reference(name)
    return _REF[name]


def plan_of(name):
    """(plan rows' coords, K, [table per S / D tuple, in order]) of a case; the builders run at the case's K"""
    if name not in _PLAN:
        enc, K = nc.compile_case(nc.CASES[name])
        _PLAN[name] = (enc.kspace.coords, K, [build(K) for _, build in enc.deferred], enc.kspace.nrow - enc.kspace.centre)
    return _PLAN[name]


def half_rows(rows):
    return np.ascontiguousarray(half_of(rows))


# ------------------------------------------------------------------------------------------------ golden agreement
@pytest.mark.parametrize("which", ["g12_nd", "g14_nd_vector"])
def test_float64_recurrence_reproduces_the_oracle_and_the_goldens(golden, which):
    g = golden(which)
    for name, tuples, opts in (sq.nd_cases() if which == "g12_nd" else sq.nd_vector_cases()):
        ref, (states, coords) = onp.simulate_nd(tuples, prune=False, return_states=True, **opts)
        grid = ref.shape[1:]
        got, table = nd_recurrence(tuples, shape=grid, dtype=np.complex128, return_state=True, **opts)
        eps = np.finfo(float).eps
        assert max(record_errors(got, ref)) <= 8 * eps, name
        assert max(record_errors(got, g[name + "_signal"].reshape(ref.shape))) <= 64 * eps, name
        mine = nc.rows_on(table, coords, grid)
        assert max(order_errors(half_rows(mine), states)) <= 8 * eps, name
        # the golden's rows (the reference pruned what cancelled numerically, below 1e-8): every row it kept, by coordinate
        gs, gc = g[name + "_states"], g[name + "_coords"]
        mine_by_key = {key: mine[..., r, :] for r, key in enumerate(coord_keys(coords))}
        for r, key in enumerate(coord_keys(gc)):
            assert np.max(np.abs(mine_by_key[key] - gs[..., r, :])) <= 1e-13, (name, key)


# ------------------------------------------------------------------------------------------------ floors
_FLOOR = {}


def measured(name):
    """(largest per-record, largest per-coordinate) error of the float64 oracle against the recurrence"""
    if name not in _FLOOR:
        c = nc.CASES[name]
        want, table = reference(name)
        got, final = nc.reference(name, oracle=True)
        coords = plan_of(name)[0]
        per_coord = max(order_errors(half_rows(nc.rows_on(final, coords, c["grid"])).astype(np.complex128), nc.rows_on(table, coords, c["grid"])))
        _FLOOR[name] = (max(record_errors(got, want)), per_coord)
    return _FLOOR[name]


@pytest.mark.parametrize("name", OWN)
def test_floor_table_is_honest(name):
    rec, coord = measured(name)
    floor = max(rec, coord if nc.CASES[name]["out"] else 0.0)      # (the floor covers what the device test bounds)
    print(name, "float64 floor: records", rec, "coordinates", coord, "table", nc.FLOORS[name])
    assert np.isfinite(floor) and floor <= nc.FLOORS[name] <= 2 * floor, (name, floor, nc.FLOORS[name])
    assert nc.MARGIN * nc.FLOORS[name] <= nc.CAP, name


# ------------------------------------------------------------------------------------------------ the conditions
def test_names_cover_the_required_kernels_and_every_case_has_a_floor():
    assert set(nc.FLOORS) == set(OWN)
    names = {c["kernel"] for c in nc.CASES.values()}
    want = ["rows_kernel<1, 1, false>", "rows_kernel<2, 1, false>", "rows_kernel<4, 1, false>",
            "run_kernel<1, 1, false>", "run_kernel<1, 2, false>", "run_kernel<1, 4, false>",
            "run_kernel<2, 1, false>", "run_kernel<2, 2, false>", "run_kernel<2, 4, false>",
            "run_kernel<4, 1, false>", "run_kernel<4, 2, false>", "run_kernel<4, 4, false>",
            "run_kernel<8, 1, false>", "run_kernel<8, 2, false>", "run_kernel<8, 4, false>",
            "run_kernel<16, 1, false>", "run_kernel<16, 2, false>", "run_kernel<16, 4, false>",
            "run_kernel<1, 1, true>", "run_kernel<4, 2, true>", "run_kernel<16, 4, true>"]
    assert sorted(want) == nc.REQUIRED_NAMES
    assert set(want) <= names, sorted(set(want) - names)
    for c in nc.CASES.values():
        assert nc.CASES[c["ref"]]["tuples"] is c["tuples"]
        assert nc.CASES[c["ref"]]["grid"] == c["grid"] and nc.CASES[c["ref"]]["opts"] == c["opts"]
    voxels = {int(np.prod(c["grid"])) for c in nc.CASES.values()}
    assert {1, 4, 5, 65} <= voxels and max(voxels) <= 70


@pytest.mark.parametrize("name", list(nc.CASES))
def test_plan_matches_the_case(name):
    """capacity, stored coordinates and the number of index spaces (the NSP of the kernel name) as the table says"""
    c = nc.CASES[name]
    enc, K = nc.compile_case(c)
    assert K == c["K"], (K, c["K"])
    assert c["rows"] is None or enc.kspace.nrow - enc.kspace.centre == c["rows"]
    assert enc.peak + 1 <= K
    enc.plan_arrays(K)
    nsp = len(enc.spaces) if len(enc.spaces) <= 2 else 4
    m = 1 if c["kernel"].startswith("rows_kernel") else K // 64
    has_in = "true" if c["start"] is not None else "false"
    want = f"rows_kernel<{nsp}, 1, false>" if K == 16 else f"run_kernel<{m}, {nsp}, {has_in}>"
    assert c["kernel"] == want, (c["kernel"], want)


@pytest.mark.parametrize("name", OWN)
def test_conditions(name):
    c = nc.CASES[name]
    want, table = reference(name)
    assert want.shape[0] == sum(t[0] == "ADC" for t in c["tuples"]) and want.shape[1:] == c["grid"]
    assert np.all(np.isfinite(want.astype(np.complex128)))
    if c["out"]:      # every coordinate the bound covers is populated: none below 1e-9 of the state's maximum
        coords, K, _, nrows = plan_of(name)
        rows = half_rows(nc.rows_on(table, coords, c["grid"]))
        scale = np.max(np.abs(rows), axis=tuple(range(rows.ndim - 2)) + (rows.ndim - 2,))
        assert scale.shape == (nrows,) and nrows <= K
        assert np.all((scale == 0) | (scale >= nc.POPULATED * scale.max())), (name, scale.min(), scale.max())
        assert np.count_nonzero(scale) >= 0.9 * nrows
    if name == "e_strong":
        assert 0 < np.max(np.abs(want[-1])) < 1e-6 * np.max(np.abs(want[0]))


# ------------------------------------------------------------------------------------------------ the planner, emulated
def emulate(name, keep_conj_a=True, swap_mirror=False):
    """the case's tuples on the device's half layout A = F(c), B = conj F(-c), Z(c) [*grid, K] in extended precision, shifts and
    diffusion through the plan's tables alone -> (records, half [*grid, 3, K])"""
    c = nc.CASES[name]
    grid = c["grid"]
    _, K, tables, _ = plan_of(name)
    tables = iter(tables)
    ar = _Arith(grid, np.clongdouble)
    st = np.zeros(grid + (3, K), ar.cplx)
    dens = np.ones(grid, ar.real)
    start = nc.start_of(c)
    if start is None:
        st[..., 2, 0] = dens
    else:
        h = half_of(start[0])
        st[..., : h.shape[-1]] = h
    out = []
    for t in c["tuples"]:
        kind = t[0]
        A, B, Z = st[..., 0, :], st[..., 1, :], st[..., 2, :]
        if kind == "T":
            R, _ = _rotation(ar, t[1], t[2])
            st = np.stack([R[..., i, 0, None] * A + R[..., i, 1, None] * B + R[..., i, 2, None] * Z for i in range(3)], axis=-2)
        elif kind in ("E", "P"):
            diag, rec, _ = _scalar(ar, kind, t[1:])
            st = np.stack([A * ar.rows(diag[0]), B * ar.rows(diag[1]), Z * ar.rows(diag[2])], axis=-2)
            if rec is not None:
                st[..., 2, 0] += rec * dens
        elif kind == "S":
            tab = np.ascontiguousarray(next(tables)).view(np.int32).reshape(3, K)
            ia, ib, iz = tab[0], tab[1], tab[2]
            ca, cb = (ia & _lib.GS_CONJ) != 0, (ib & _lib.GS_CONJ) != 0
            ja, jb, jz = ia & (K - 1), ib & (K - 1), iz & (K - 1)
            na = np.where(ca, B[..., ja].conj() if keep_conj_a else B[..., ja], A[..., ja])
            nb = np.where(cb, A[..., jb].conj(), B[..., jb])
            st = np.stack([np.where(ia < 0, 0, na), np.where(ib < 0, 0, nb), np.where(iz < 0, 0, Z[..., jz])], axis=-2)
        elif kind == "D":
            tab = np.asarray(next(tables))
            tab = tab.reshape(tab.shape[:-1] + (3, K))
            tab = tab.reshape(tab.shape[:-2] + (1,) * (len(grid) - (tab.ndim - 2)) + (3, K)).astype(ar.real)
            if swap_mirror:
                tab = tab[..., [1, 0, 2], :]
            st = st * tab
        elif kind == "ADC":
            out.append(np.array(st[..., 0 if (len(t) < 2 or t[1] == "F0") else 2, 0]))
        elif kind == "SPOILER":
            st = st.copy()
            st[..., :2, :] = 0
        elif kind == "RESET":
            st = np.zeros_like(st)
            st[..., 2, 0] = dens
        else:
            raise ValueError(kind)
        st = np.broadcast_to(st, grid + (3, K)).astype(ar.cplx)
    assert next(tables, None) is None
    return np.stack(out), st


def emulation_errors(name, **mutation):
    c = nc.CASES[name]
    records, half = emulate(name, **mutation)
    want, table = reference(name)
    rows = nc.rows_on(table, plan_of(name)[0], c["grid"])      # (asserts: no coordinate the reference holds was pruned)
    return max(record_errors(records, want)), max(order_errors(half, rows))


@pytest.mark.parametrize("name", OWN)
def test_planner_tables_reproduce_the_recurrence(name):
    rec, coord = emulation_errors(name)
    bound = nc.MARGIN * nc.FLOORS[name]
    # (coordinates of a case whose state the device test does not read: against the float64 oracle's own per-coordinate error,
    # which FLOORS does not hold for them -- a diffusion factor of e^-60 carries the rounding of its exponent)
    cbound = bound if nc.CASES[name]["out"] else nc.MARGIN * max(nc.FLOORS[name], measured(name)[1])
    print(name, "emulated plan: records", rec, "coordinates", coord, "bounds", bound, cbound)
    assert rec <= bound and coord <= cbound, (name, rec, coord, bound, cbound)


def test_group_b_tables_hold_conjugated_sources_on_both_sides_and_empty_ones():
    for name in OWN:
        if nc.CASES[name]["group"] != "b":
            continue
        _, K, tables, _ = plan_of(name)
        gs = [np.ascontiguousarray(t).view(np.int32).reshape(3, K) for t in tables if t.shape[-1] * 2 == 3 * K and t.shape[:-1] == (1,)]
        conj_a = any(((t[0] >= 0) & ((t[0] & _lib.GS_CONJ) != 0)).any() for t in gs)
        conj_b = any(((t[1] >= 0) & ((t[1] & _lib.GS_CONJ) != 0)).any() for t in gs)
        assert conj_a and conj_b and any((t[:, : 4] < 0).any() for t in gs), name


MUTANTS = ["a_13_1_5", "b_64_61_2", "e_scalar_k", "e_tensor2", "f_lead1"]


@pytest.mark.parametrize("mutation", [{"keep_conj_a": False}, {"swap_mirror": True}])
def test_mutations_of_the_emulation_fail(mutation):
    """the conjugate of one side dropped; bT swapped with its mirror: each must break at least one case"""
    failed = [name for name in MUTANTS if max(emulation_errors(name, **mutation)) > nc.MARGIN * nc.FLOORS[name]]
    print(mutation, "fails", failed)
    assert failed
