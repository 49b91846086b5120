"""Forward-mode EPG recurrence with first- AND second-order partials: the checker of tests/test_gpu_hessian_paths.py.

A plain NumPy restatement of the reference's order-2 recurrence (diff.py:290-379) on the oracle's operator tuples
(tests/sequences.py), in the style of tests/jacobian_recurrence.py (whose number formats, closed-form first partials and shift
it reuses) and sharing nothing with epgpy_amd/diff.py.  Per variable pair (a, b) and operator

    H_ab <- Op H_ab  +  sum_p order2[ab][p] (dOp/dp) S  +  sum_{p1 p2} c1 c2 (d2Op/dp1 dp2) S  +  cross terms
    S_v  <- Op S_v + sum_p coeff[v][p] (dOp/dp) S                    S <- Op S

with the reference's selection of terms: the cross term (dOp/dv2) S_v1 enters when v1 is alive in the state (some earlier
operator declared it), v2 is a variable of the operator, and the pair is in the operator's order2 -- or, for an operator with
auto_cross_derivatives (order2 given as True, a name or a list of names), always; for v1 == v2 it enters twice.  The second
partials are closed forms of T and E / P / R.  `dtype`: np.clongdouble (the reference of the device tests) or np.complex128
(reproduces the reference's own numbers, tests/golden G13)."""
import numpy as np

from tests.jacobian_recurrence import SCALAR_PARAMS, T_PARAMS, _Arith, _normalise, _rotation, _scalar, _shift, grid_of

SECOND_ALLOWED = {
    "T": {("alpha", "alpha"), ("alpha", "phi"), ("phi", "phi")},
    "E": {("tau", "tau"), ("T1", "T1"), ("T2", "T2"), ("g", "g"), ("T1", "tau"), ("T2", "tau"), ("g", "tau"), ("T2", "g")},
    "P": {("tau", "tau"), ("g", "g"), ("g", "tau")},
    "R": {("rT", "rT"), ("rL", "rL"), ("r0", "r0")},
}


def pair_of(a, b=None):
    if b is None:
        a, b = a
    return (b, a) if a > b else (a, b)


def parse(opts, kind):
    """({variable: {parameter: coefficient}}, {sorted pair: {parameter: coefficient}}, auto_cross) of a tuple's trailing dict"""
    params = T_PARAMS if kind == "T" else SCALAR_PARAMS[kind]
    order1, order2 = opts.get("order1"), opts.get("order2")
    auto = isinstance(order2, (bool, str)) or (order2 is not None and all(isinstance(x, str) for x in order2))
    if not order1 and isinstance(order2, (bool, str)):
        order1 = order2
    order1 = _normalise(order1, params)
    if not order2:
        return order1, {}, auto
    if order2 is True:
        order2 = {pair_of(p): {} for p in SECOND_ALLOWED[kind]}
    elif isinstance(order2, str):
        order2 = {(order2, order2): {}}
    elif all(isinstance(x, str) for x in order2):
        order2 = {pair_of(a, b): {} for a in order2 for b in order2}
    elif not isinstance(order2, dict):
        order2 = {pair_of(p): {} for p in order2}
    else:
        order2 = {pair_of(p): dict(c) for p, c in order2.items()}
    return order1, order2, auto


def _rotation2(ar, alpha, phi):
    """{sorted parameter pair: d2R} per degree^2, element by element (R as in jacobian_recurrence._rotation)"""
    a, p = np.broadcast_arrays(ar.g(alpha) * ar.pi / 180, ar.g(phi) * ar.pi / 180)
    s, c = np.sin(a), np.cos(a)
    s2 = np.sin(a / 2) ** 2
    e1, e2 = np.exp(1j * p.astype(ar.cplx)), np.exp(2j * p.astype(ar.cplx))
    deg2 = (ar.pi / 180) ** 2
    z = np.zeros(a.shape, ar.cplx)

    def mat(rows):
        return np.stack([np.stack([z + x for x in row], axis=-1) for row in rows], axis=-2)

    dAA = mat([[-c / 2, e2 * c / 2, 1j * e1 * s],
               [e2.conj() * c / 2, -c / 2, -1j * e1.conj() * s],
               [0.5j * e1.conj() * s, -0.5j * e1 * s, -c]]) * deg2
    dAP = mat([[z, 1j * e2 * s, e1 * c],
               [-1j * e2.conj() * s, z, e1.conj() * c],
               [-0.5 * e1.conj() * c, -0.5 * e1 * c, z]]) * deg2
    dPP = mat([[z, -4 * e2 * s2, 1j * e1 * s],
               [-4 * e2.conj() * s2, z, -1j * e1.conj() * s],
               [0.5j * e1.conj() * s, -0.5j * e1 * s, z]]) * deg2
    return {("alpha", "alpha"): dAA, ("alpha", "phi"): dAP, ("phi", "phi"): dPP}


def _scalar2(ar, kind, args):
    """{sorted parameter pair: ((d2 F+, d2 F-, d2 Z), d2 recovery)} of E / P / R"""
    zero = ar.real(0)

    def transverse(x):
        return ((np.conj(x), x, zero), zero)

    if kind == "R":
        rT, rL, r0 = ar.g(args[0], cplx=True), ar.g(args[1]), ar.g(args[2])
        eT, eL, e0 = np.exp(-rT), np.exp(-rL), np.exp(-r0)
        return {("rT", "rT"): transverse(eT), ("rL", "rL"): ((zero, zero, eL), zero), ("r0", "r0"): ((zero, zero, zero), -e0)}
    if kind == "P":
        tau, g = ar.g(args[0]), ar.g(args[1])
        w = 2j * ar.pi * g.astype(ar.cplx)
        e = np.exp(-w * tau)
        return {("tau", "tau"): transverse(w * w * e), ("g", "g"): transverse(-4 * ar.pi ** 2 * tau ** 2 * e),
                ("g", "tau"): transverse(-2j * ar.pi * (1 - w * tau) * e)}
    tau, T1, T2 = ar.g(args[0]), ar.g(args[1]), ar.g(args[2])
    g = ar.g(args[3]) if len(args) > 3 else ar.real(0)
    w = 1 / T2 + 2j * ar.pi * np.asarray(g).astype(ar.cplx)
    e, eL = np.exp(-w * tau), np.exp(-tau / T1)

    def longitudinal(x):
        return ((zero, zero, x), -x)

    return {("tau", "tau"): ((np.conj(w * w * e), w * w * e, eL / T1 ** 2), -eL / T1 ** 2),
            ("T1", "T1"): longitudinal((-2 * tau / T1 ** 3 + tau ** 2 / T1 ** 4) * eL),
            ("T2", "T2"): transverse((-2 * tau / T2 ** 3 + tau ** 2 / T2 ** 4) * e),
            ("g", "g"): transverse(-4 * ar.pi ** 2 * tau ** 2 * e),
            ("T1", "tau"): longitudinal((1 - tau / T1) / T1 ** 2 * eL),
            ("T2", "tau"): transverse((1 - w * tau) / T2 ** 2 * e),
            ("g", "tau"): transverse(-2j * ar.pi * (1 - w * tau) * e),
            ("T2", "g"): transverse(-2j * ar.pi * tau ** 2 / T2 ** 2 * e)}


def hessian_recurrence(ops, pairs, *, probe=None, shape=None, max_nstate=None, through_plain=False, dtype=np.clongdouble):
    """{"S": [record, *grid], "first": {variable: [record, *grid]}, "second": {sorted pair: [record, *grid]}} at every ADC,
    for the variable pairs `pairs` and the variables in them (zeros where nothing was declared).

    ops: oracle tuples as in jacobian_recurrence, the trailing dict of T / E / P / R with "order1" and / or "order2"
    probe: "F0" / "Z0" for every ADC; None: what each ADC tuple says
    through_plain: SPOILER acts on the derivative states too (exact_partials=True on the device); resets always clear them"""
    pairs = list(dict.fromkeys(pair_of(p) for p in pairs))
    variables = sorted({v for p in pairs for v in p})
    plain = [op[:-1] if isinstance(op[-1], dict) else op for op in ops]
    grid = tuple(shape) if shape is not None else grid_of(plain)
    ar = _Arith(grid, dtype)
    n = 0
    reach = sum(abs(int(op[1])) for op in plain if op[0] == "S")
    nmax = min(reach, int(max_nstate)) if max_nstate else reach
    st = np.zeros(grid + (2 * nmax + 1, 3), ar.cplx)
    dens = np.ones(grid, ar.real)
    st[..., nmax, 2] = dens
    first, second = {}, {}
    alive, exist2 = set(), set()     # variables / pairs whose states exist (all of them, not only the requested ones)
    out = {"S": [], "first": {v: [] for v in variables}, "second": {p: [] for p in pairs}}

    def add(states, key, term):
        states[key] = states[key] + term if key in states else term

    for op, base in zip(ops, plain):
        kind = base[0]
        if kind == "T" or kind in SCALAR_PARAMS:
            order1, order2, auto = parse(op[-1] if isinstance(op[-1], dict) else {}, kind)
            if kind == "T":
                R, d1 = _rotation(ar, base[1], base[2])
                d2 = _rotation2(ar, base[1], base[2]) if order2 else {}

                def mul(m, x, with_eq=False):          # rows above order n hold nothing
                    y = np.zeros_like(x)
                    act = x[..., nmax - n: nmax + n + 1, :]
                    y[..., nmax - n: nmax + n + 1, :] = np.stack([sum(m[..., None, i, j] * act[..., j] for j in range(3)) for i in range(3)], axis=-1)
                    return y

                value = R
            else:
                diag, rec, d1 = _scalar(ar, kind, base[1:])
                d2 = _scalar2(ar, kind, base[1:]) if order2 else {}

                def mul(m, x, with_eq=False):
                    dg, r = m
                    y = np.zeros_like(x)
                    y[..., nmax - n: nmax + n + 1, :] = np.stack([x[..., nmax - n: nmax + n + 1, j] * ar.rows(dg[j]) for j in range(3)], axis=-1)
                    if with_eq and r is not None:
                        y[..., nmax, 2] += r * dens
                    return y

                value = (diag, rec)
                d1 = dict(d1)

            def scaled(term, c):
                return term * ar.g(c)[..., None, None]

            new2 = {p: mul(value if kind == "T" else (value[0], None), h) for p, h in second.items()}
            # the reference runs its order-2 step only once the state carries a second-order entry (of ANY pair) or the
            # operator declares one (DiffOperator.__call__)
            active = bool(exist2 or order2)
            if active:
                exist2 |= {pair for pair, coeffs in order2.items() if coeffs}
                exist2 |= {pair for pair in order2 if any(pair_of(p1, p2) in SECOND_ALLOWED[kind] for p1 in order1.get(pair[0], {})
                                                           for p2 in order1.get(pair[1], {}))}
                cross_all = {pair_of(v1, v2) for v1 in order1 for v2 in alive} if auto else set(order2)
                exist2 |= {pair_of(v1, v2) for v1 in alive for v2 in order1 if pair_of(v1, v2) in cross_all}
            else:
                order2 = {}
            # coefficients of the parameters' second derivatives w.r.t. the variable pairs, then second partials of the operator
            for pair, coeffs in order2.items():
                if pair not in pairs:
                    continue
                for p, c in coeffs.items():
                    add(new2, pair, scaled(mul(d1[p], st, True), c))
                prods = {pair_of(p1, p2): c1 * c2 for p1, c1 in order1.get(pair[0], {}).items() for p2, c2 in order1.get(pair[1], {}).items()}
                for pp, c in prods.items():
                    if pp in SECOND_ALLOWED[kind]:
                        add(new2, pair, scaled(mul(d2[pp], st, True), c))
            # cross terms: first partials of the operator on the first-order states that are alive
            cross = {pair_of(v1, v2) for v1 in order1 for v2 in first} if auto else set(order2)
            for v1 in (list(first) if active else []):
                for v2 in order1:
                    pair = pair_of(v1, v2)
                    if pair in cross and pair in pairs:
                        for p, c in order1[v2].items():
                            add(new2, pair, scaled(mul(d1[p], first[v1]), c) * (2 if v1 == v2 else 1))
            new1 = {v: mul(value if kind == "T" else (value[0], None), d) for v, d in first.items()}
            for var, coeffs in order1.items():
                if var in variables:
                    for p, c in coeffs.items():
                        add(new1, var, scaled(mul(d1[p], st, True), c))
            alive |= set(order1)
            first, second, st = new1, new2, mul(value, st, True)
        elif kind == "S":
            k = int(base[1])
            n = n + abs(k) if not max_nstate else max(n, min(n + abs(k), int(max_nstate)))
            st = _shift(st, k, n, nmax)
            first = {v: _shift(d, k, n, nmax) for v, d in first.items()}
            second = {p: _shift(h, k, n, nmax) for p, h in second.items()}
        elif kind == "ADC":
            what = probe or (base[1] if len(base) > 1 else "F0")
            col = 0 if what == "F0" else 2
            zeros = np.zeros(grid, ar.cplx)
            out["S"].append(st[..., nmax, col].copy())
            for v in variables:
                out["first"][v].append(np.broadcast_to(first[v][..., nmax, col], grid).copy() if v in first else zeros)
            for p in pairs:
                out["second"][p].append(np.broadcast_to(second[p][..., nmax, col], grid).copy() if p in second else zeros)
        elif kind == "SPOILER":
            st = st.copy()
            st[..., :2] = 0
            if through_plain:
                for d in list(first.values()) + list(second.values()):
                    d[..., :2] = 0
        elif kind in ("RESET", "PD"):
            if kind == "PD":
                dens = np.broadcast_to(ar.g(np.atleast_1d(base[1])), grid).astype(ar.real)
            if kind == "RESET" or len(base) < 3 or base[2]:
                st = np.zeros_like(st)
                st[..., nmax, 2] = dens
                first, second = {}, {}       # (alive / exist2 stay: a cleared state contributes zeros)
                if kind == "RESET":
                    n = 0
        elif kind not in ("WAIT", "NULL"):
            raise ValueError(f"unsupported operator {kind}")
        for states in (first, second):
            for key in states:
                if states[key].shape != st.shape:
                    states[key] = np.broadcast_to(states[key], st.shape).copy()
    nrec = len(out["S"])
    stack = lambda rows: np.stack(rows) if nrec else np.zeros((0,) + grid, ar.cplx)
    return {"S": stack(out["S"]), "first": {v: stack(r) for v, r in out["first"].items()},
            "second": {p: stack(r) for p, r in out["second"].items()}}


def hessian_array(res, variables1, variables2):
    """[record, *grid, n1, n2] as a Hessian probe returns it ("magnitude" rows / columns: the first derivatives)"""
    zeros = np.zeros_like(res["S"])
    rows = []
    for v1 in variables1:
        row = []
        for v2 in variables2:
            if v1 == "magnitude":
                row.append(res["first"].get(v2, zeros))
            elif v2 == "magnitude":
                row.append(res["first"].get(v1, zeros))
            else:
                row.append(res["second"].get(pair_of(v1, v2), zeros))
        rows.append(np.stack(row, axis=-1))
    return np.stack(rows, axis=-2)


def pass_rows(res, a, b):
    """[record, *grid, 3 | 4]: the rows one fused pass writes -- S, S_a, (S_b,) H_ab"""
    cols = [res["S"], res["first"][a]] + ([res["first"][b]] if a != b else []) + [res["second"][pair_of(a, b)]]
    return np.stack(cols, axis=-1)
