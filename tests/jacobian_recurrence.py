"""Forward-mode EPG recurrence with first-order partials in extended precision: the checker of tests/test_gpu_jacobian_paths.py.

A plain restatement of the reference's order-1 recurrence (diff.py:119-139, :264-288)

    dS_v <- Op(dS_v, no equilibrium)  +  sum_p coeff[v][p] (dOp/dp)(S)         S <- Op(S)

on the oracle's operator tuples (tests/sequences.py), written from the operators' closed forms and sharing nothing with
oracle/epg_numpy.py::simulate_jacobian.  Parameters enter as the float64 values the device receives; from there on every
operation -- exp, cos, sin included -- runs in `dtype` (np.clongdouble: 64-bit mantissas on x86-64, eps 1.1e-19), so the
result measures a kernel's arithmetic AND the float64 rounding of its tables.

State: [*grid, 2 nmax + 1, 3], rows k = -nmax .. nmax, columns F_k, conj(F_-k), Z_k, at a fixed nmax that holds every order the
sequence reaches; `n` tracks the reference's growing matrix (it decides what a shift truncates)."""
import numpy as np

T_PARAMS = ("alpha", "phi")
SCALAR_PARAMS = {"E": ("tau", "T1", "T2", "g"), "P": ("tau", "g"), "R": ("rT", "rL", "r0")}


def _normalise(order1, params):
    """the forms `order1=` takes (diff.py:153-198) -> {variable: {parameter: coefficient}}"""
    if not order1:
        return {}
    if order1 is True:
        return {p: {p: 1} for p in params}
    if isinstance(order1, str):
        return {order1: {order1: 1}}
    if isinstance(order1, (list, tuple, set)):
        return {p: {p: 1} for p in order1}
    return {v: ({c: 1} if isinstance(c, str) else dict(c)) for v, c in order1.items()}


def grid_of(ops):
    """the grid the operators' array parameters span: axes are leading grid axes, missing ones appended"""
    nparam = {"T": 2, "E": 4, "P": 2, "R": 3, "PD": 1}
    shapes = [np.shape(a) for op in ops for a in op[1:1 + nparam.get(op[0], 0)] if not isinstance(a, (dict, bool))]
    grid = [1] * max([len(s) for s in shapes] + [1])
    for s in shapes:
        for i, d in enumerate(s):
            if d != 1:
                assert grid[i] in (1, d), (grid, s)
                grid[i] = d
    return tuple(grid)


class _Arith:
    """number formats and grid alignment of one run"""

    def __init__(self, grid, dtype):
        self.grid, self.cplx = tuple(grid), np.dtype(dtype).type
        self.real = np.finfo(dtype).dtype.type
        self.pi = 4 * np.arctan(self.real(1))

    def g(self, x, cplx=False):
        """a parameter whose axes are the leading grid axes -> [*grid-like] (missing axes appended)"""
        x = np.asarray(x)
        x = x.astype(self.cplx if (cplx or np.iscomplexobj(x)) else self.real)
        return x.reshape(x.shape + (1,) * (len(self.grid) - x.ndim)) if x.ndim else x

    def rows(self, x):
        """[*grid-like] -> broadcastable against [*grid, rows]"""
        return np.asarray(x)[..., None]


def _rotation(ar, alpha, phi):
    """(R, dR/dalpha, dR/dphi) per degree, [*grid-like, 3, 3]:  R = Rz(phi) Rx(alpha) Rz(-phi), element by element"""
    a, p = np.broadcast_arrays(ar.g(alpha) * ar.pi / 180, ar.g(phi) * ar.pi / 180)
    s, c = np.sin(a), np.cos(a)
    c2, s2 = np.cos(a / 2) ** 2, np.sin(a / 2) ** 2
    e1, e2 = np.exp(1j * p.astype(ar.cplx)), np.exp(2j * p.astype(ar.cplx))
    deg = ar.pi / 180
    z = np.zeros(a.shape, ar.cplx)

    def mat(rows):
        return np.stack([np.stack([z + x for x in row], axis=-1) for row in rows], axis=-2)

    R = mat([[c2, e2 * s2, -1j * e1 * s],
             [e2.conj() * s2, c2, 1j * e1.conj() * s],
             [-0.5j * e1.conj() * s, 0.5j * e1 * s, c]])
    dA = mat([[-s / 2, e2 * s / 2, -1j * e1 * c],
              [e2.conj() * s / 2, -s / 2, 1j * e1.conj() * c],
              [-0.5j * e1.conj() * c, 0.5j * e1 * c, -s]]) * deg
    dP = mat([[z, 2j * e2 * s2, e1 * s],
              [-2j * e2.conj() * s2, z, e1.conj() * s],
              [-0.5 * e1.conj() * s, -0.5 * e1 * s, z]]) * deg
    return R, {"alpha": dA, "phi": dP}


def _scalar(ar, kind, args):
    """(diag [3 x [*grid-like]], recovery, {param: (ddiag, drecovery)}) of E / P / R; diag = (F+, F-, Z) factors"""
    zero = ar.real(0)
    if kind == "R":
        rT, rL, r0 = ar.g(args[0], cplx=True), ar.g(args[1]), ar.g(args[2])
        eT, eL, e0 = np.exp(-rT), np.exp(-rL), np.exp(-r0)
        diag, rec = (eT.conj(), eT, eL), 1 - e0
        parts = {"rT": ((-eT.conj(), -eT, zero), zero), "rL": ((zero, zero, -eL), zero), "r0": ((zero, zero, zero), e0)}
        return diag, rec, parts
    if kind == "P":
        tau, g = ar.g(args[0]), ar.g(args[1])
        w = 2j * ar.pi * g.astype(ar.cplx)               # F- turns by exp(-w tau), F+ by its conjugate
        e = np.exp(-w * tau)
        parts = {"tau": ((np.conj(-w * e), -w * e, zero), zero), "g": ((np.conj(-2j * ar.pi * tau * e), -2j * ar.pi * tau * e, zero), zero)}
        return (e.conj(), e, ar.real(1) + 0 * tau), None, parts
    tau, T1, T2 = ar.g(args[0]), ar.g(args[1]), ar.g(args[2])
    g = ar.g(args[3]) if len(args) > 3 else ar.real(0)
    w = 1 / T2 + 2j * ar.pi * np.asarray(g).astype(ar.cplx)
    e, eL = np.exp(-w * tau), np.exp(-tau / T1)
    dg = -2j * ar.pi * tau * e
    parts = {"tau": ((np.conj(-w * e), -w * e, -eL / T1), eL / T1),
             "T1": ((zero, zero, tau / T1 ** 2 * eL), -tau / T1 ** 2 * eL),
             "T2": ((tau / T2 ** 2 * e.conj(), tau / T2 ** 2 * e, zero), zero),
             "g": ((dg.conj(), dg, zero), zero)}
    return (e.conj(), e, eL), 1 - eL, parts


def _shift(st, k, keep, nmax):
    """F+ up / F- down by k rows, zero fill; F+ / F- above order `keep` <- 0 (Z does not move)"""
    new = np.zeros_like(st)
    rows = st.shape[-2]
    if abs(k) < rows:
        if k > 0:
            new[..., k:, 0], new[..., : rows - k, 1] = st[..., : rows - k, 0], st[..., k:, 1]
        elif k < 0:
            new[..., : rows + k, 0], new[..., -k:, 1] = st[..., -k:, 0], st[..., : rows + k, 1]
        else:
            new[..., :2] = st[..., :2]
    new[..., 2] = st[..., 2]
    new[..., : nmax - keep, :2] = 0
    new[..., nmax + keep + 1:, :2] = 0
    return new


def jacobian_recurrence(ops, variables, *, probe=None, shape=None, max_nstate=None, through_plain=False, init=None,
                        kvalue=1.0, dtype=np.clongdouble, return_state=False):
    """[record, *grid, 1 + len(variables)]: column 0 the probed state, column 1 + v its derivative w.r.t. variables[v] (zeros
    for a name no operator declares) at every ADC.

    ops: oracle tuples ("T", alpha, phi) ("E", tau, T1, T2[, g]) ("P", tau, g) ("R", rT, rL, r0) ("S", n) ("D", tau, D)
         ("ADC"[, "F0" | "Z0"[, phase]]) ("SPOILER",) ("RESET",) ("PD", pd[, reset]), a trailing {"order1": ...} on T / E / P / R
    probe: "F0" / "Z0" for every ADC (a Jacobian probe's own kind); None: what each ADC tuple says
    through_plain: SPOILER / D act on the derivative states too (exact_partials=True on the device); resets always clear them
    init: start state [*grid-like, 2 n0 + 1, 3] in the StateMatrix layout (rows k = -n0 .. n0), its partials zero
    max_nstate: shifts truncate F+ / F- above this order; kvalue: rad/m per order, for D
    return_state: also the final state [*grid, 2 n + 1, 3], rows k = -n .. n at the reference's growing n -> (records, state)"""
    plain = [op[:-1] if isinstance(op[-1], dict) else op for op in ops]
    grid = tuple(shape) if shape is not None else grid_of(plain)
    ar = _Arith(grid, dtype)
    n = 0 if init is None else (np.shape(init)[-2] - 1) // 2
    reach = n + sum(abs(int(op[1])) for op in plain if op[0] == "S")
    nmax = max(n, min(reach, int(max_nstate))) if max_nstate else reach
    st = np.zeros(grid + (2 * nmax + 1, 3), ar.cplx)
    dens = np.ones(grid, ar.real)
    if init is None:
        st[..., nmax, 2] = dens
    else:
        init = np.asarray(init)
        init = init.reshape(init.shape[:-2] + (1,) * (len(grid) - (init.ndim - 2)) + init.shape[-2:])
        st[..., nmax - n: nmax + n + 1, :] = init
    dst = {}
    orders = np.arange(-nmax, nmax + 1).astype(ar.real)
    out = []
    for op, base in zip(ops, plain):
        kind = base[0]
        if kind == "T":
            order1 = _normalise(op[-1].get("order1") if isinstance(op[-1], dict) else None, T_PARAMS)
            R, dR = _rotation(ar, base[1], base[2])

            def mul(m, x):          # rows above order n hold nothing
                y = np.zeros_like(x)
                act = x[..., nmax - n: nmax + n + 1, :]
                y[..., nmax - n: nmax + n + 1, :] = np.stack([sum(m[..., None, i, j] * act[..., j] for j in range(3)) for i in range(3)], axis=-1)
                return y

            new = {v: mul(R, d) for v, d in dst.items()}
            for var, coeffs in order1.items():
                if var not in variables:
                    continue
                for p, c in coeffs.items():
                    term = mul(dR[p], st) * ar.g(c)[..., None, None]
                    new[var] = new[var] + term if var in new else term
            dst, st = new, mul(R, st)
        elif kind in SCALAR_PARAMS:
            order1 = _normalise(op[-1].get("order1") if isinstance(op[-1], dict) else None, SCALAR_PARAMS[kind])
            diag, rec, parts = _scalar(ar, kind, base[1:])

            def mul(dg, r, x, with_eq):
                y = np.zeros_like(x)
                y[..., nmax - n: nmax + n + 1, :] = np.stack([x[..., nmax - n: nmax + n + 1, j] * ar.rows(dg[j]) for j in range(3)], axis=-1)
                if with_eq and r is not None:
                    y[..., nmax, 2] += r * dens
                return y

            new = {v: mul(diag, None, d, False) for v, d in dst.items()}
            for var, coeffs in order1.items():
                if var not in variables:
                    continue
                for p, c in coeffs.items():
                    term = mul(parts[p][0], parts[p][1], st, True) * ar.g(c)[..., None, None]
                    new[var] = new[var] + term if var in new else term
            dst, st = new, mul(diag, rec, st, True)
        elif kind == "S":
            k = int(base[1])
            n = n + abs(k) if not max_nstate else max(n, min(n + abs(k), int(max_nstate)))
            st = _shift(st, k, n, nmax)
            dst = {v: _shift(d, k, n, nmax) for v, d in dst.items()}
        elif kind == "D":
            att = np.exp(-(orders * ar.real(kvalue) / 1000) ** 2 * (ar.g(base[1]) / 1000)[..., None] * ar.g(base[2])[..., None])
            st = st * att[..., None]
            if through_plain:
                dst = {v: d * att[..., None] for v, d in dst.items()}
        elif kind == "ADC":
            what = probe or (base[1] if len(base) > 1 else "F0")
            col = 0 if what == "F0" else 2
            rec = np.zeros(grid + (1 + len(variables),), ar.cplx)
            rec[..., 0] = st[..., nmax, col]
            for v, var in enumerate(variables):
                if var in dst:
                    rec[..., 1 + v] = dst[var][..., nmax, col]
            if len(base) > 2 and base[2] is not None:
                rec = rec * np.exp(1j * ar.g(base[2], cplx=True) * ar.pi / 180)[..., None]
            out.append(rec)
        elif kind == "SPOILER":
            st = st.copy()
            st[..., :2] = 0
            if through_plain:
                for d in dst.values():
                    d[..., :2] = 0
        elif kind in ("RESET", "PD"):
            if kind == "PD":
                dens = np.broadcast_to(ar.g(np.atleast_1d(base[1])), grid).astype(ar.real)
            if kind == "RESET" or len(base) < 3 or base[2]:
                st = np.zeros_like(st)
                st[..., nmax, 2] = dens
                dst = {}
                if kind == "RESET":
                    n = 0
        elif kind not in ("WAIT", "NULL"):
            raise ValueError(f"unsupported operator {kind}")
        for v in dst:
            if dst[v].shape != st.shape:
                dst[v] = np.broadcast_to(dst[v], st.shape).copy()
    records = np.stack(out) if out else np.zeros((0,) + grid + (1 + len(variables),), ar.cplx)
    if return_state:
        return records, st[..., nmax - n: nmax + n + 1, :].copy()
    return records


def column_errors(got, want, zero_atol=0.0):
    """[err_v]: max|got[..., v] - want[..., v]| over records and voxels / max|want[..., v]| (column 0, the signal itself:
    / max(1, max|want[..., 0]|)); a column whose reference is identically zero must be exactly zero (inf otherwise).
    `zero_atol`: what such a column may hold instead -- only for the float64 oracle, whose triple-product rotations leave
    1e-18 where the closed form has none"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    errs = []
    for v in range(want.shape[-1]):
        scale = float(np.max(np.abs(want[..., v]))) if want[..., v].size else 0.0
        diff = float(np.max(np.abs(got[..., v].astype(np.clongdouble) - want[..., v]))) if want[..., v].size else 0.0
        if v == 0:
            scale = max(1.0, scale)
        errs.append((0.0 if diff <= zero_atol else np.inf) if scale == 0.0 else diff / scale)
    return errs
