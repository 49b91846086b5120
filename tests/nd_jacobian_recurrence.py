"""First-order partials through integer n-D shifts and diffusion in extended precision: the checker of
tests/test_gpu_nd_jacobian_paths.py.  A forward-mode layer over tests/nd_recurrence.py:

    nd_jacobian_recurrence(ops, variables, shape=, kvalue=, max_nstate=, init=, through_plain=)
                                        -> records [record, *grid, 1 + V]   (np.clongdouble)
    nd_jacobian_recurrence(..., return_state=True)
                                        -> (records, {coordinate: (F, Z)}, {variable: {coordinate: (dF, dZ)}})

The state is the table of nd_recurrence -- an integer coordinate key -> (F, Z), F at every signed coordinate, no sorted rows,
no gather tables, no mirror column, no pruning -- and every variable has one more such table ON THE SAME KEYS.  The reference
cannot say what these derivatives are: it prunes the rows of each derivative state on its own and then fails to broadcast them
against the state's rows.  The library keeps derivative states on the plan's rows; what they hold is defined by the
mathematical derivative, which is what this forward-mode recurrence states (and a central finite difference of the plain
nd_recurrence confirms, tests/test_nd_jacobian_recurrence_host.py).

    T E P  + {"order1": ..}   dS_v <- Op(dS_v, no recovery) + sum_p coeff (dOp/dp)(S), the closed forms of
                              tests/jacobian_recurrence.py on the row (F(c), conj F(-c), Z(c)); the recovery term's partial
                              at coordinate 0 only
    S(delta)                  every derivative table moves exactly as the state does: the same keys, the same box rule
                              (WHOLE_ROWS included)
    D                         the state is attenuated; the derivative tables take the same factors (the mirror included:
                              dF(-c) takes bT of -c) only with through_plain -- the device's exact_partials /
                              DERIV_THROUGH_PLAIN_OPS; by default they are left alone
    SPOILER                   dF <- 0 only with through_plain;   RESET / PD-with-reset: the derivative tables are cleared, always
    ADC                       column 0 the probed state, column 1 + v its derivative at coordinate 0
    init=(states, coords)     as nd_recurrence, the partials zero

With no variables the records are those of nd_recurrence bit for bit (the same operations in the same order)."""
import numpy as np

from tests.jacobian_recurrence import _Arith, _normalise, _rotation, _scalar, SCALAR_PARAMS, T_PARAMS
from tests.nd_recurrence import NDState, _Table, _append, _delta, _lead_of, nd_grid

WHOLE_ROWS = True


def strip(ops):
    """the tuples without their trailing {"order1": ..}"""
    return [op[:-1] if isinstance(op[-1], dict) else op for op in ops]


def _order1(op, params):
    return _normalise(op[-1].get("order1") if isinstance(op[-1], dict) else None, params)


def _gather(arr, idx):
    out = np.zeros((len(idx),) + arr.shape[1:], arr.dtype)
    have = idx >= 0
    out[have] = arr[idx[have]]
    return out


def nd_jacobian_recurrence(ops, variables, *, shape=None, kvalue=1.0, max_nstate=None, init=None, through_plain=False,
                           dtype=np.clongdouble, return_state=False):
    """ops: the tuples of nd_recurrence, T / E / P with a trailing {"order1": {variable: {parameter: coefficient}}}"""
    variables = list(variables)
    plain = strip(ops)
    grid = nd_grid(plain, shape)
    ar = _Arith(grid, dtype)
    lead, kdim = (), 1
    for op in plain:
        if op[0] == "S" and not np.isscalar(op[1]):
            lead, kdim = _append(lead, np.shape(op[1])[:-1]), max(kdim, np.shape(op[1])[-1])
        if op[0] == "D":
            if len(op) > 3 and op[3] is not None:
                kdim = max(kdim, len(op[3]))
            if not isinstance(op[2], tuple) and np.ndim(op[2]) >= 2:
                kdim = max(kdim, np.shape(op[2])[-1])
    if init is not None:
        c0 = np.asarray(init[1])
        lead, kdim = _append(lead, c0.shape[:-2]), max(kdim, c0.shape[-1])
    assert len(lead) <= len(grid) and all(a in (1, b) for a, b in zip(lead, grid)), (lead, grid)
    tab = _Table(ar, lead, kdim)
    dens = np.ones(grid, ar.real)
    if init is None:
        tab.equilibrium(dens)
    else:
        st = np.asarray(init[0])
        st = np.broadcast_to(st.reshape(st.shape[:-2] + (1,) * (len(grid) - (st.ndim - 2)) + st.shape[-2:]), grid + st.shape[-2:])
        l0 = _lead_of(c0.shape[:-2])
        cc = np.zeros(l0 + (c0.shape[-2], kdim), np.int64)
        cc[..., : c0.shape[-1]] = c0.reshape(l0 + c0.shape[-2:])
        cc = np.broadcast_to(cc.reshape(l0 + (1,) * (len(lead) - len(l0)) + cc.shape[-2:]), lead + cc.shape[-2:])
        entries = {}
        for r in range(cc.shape[-2]):
            entries[tuple(int(v) for v in cc[..., r, :].reshape(-1))] = [st[..., r, 0].astype(ar.cplx), st[..., r, 2].astype(ar.cplx)]
        tab.build(entries)
    kv = np.broadcast_to(np.asarray(kvalue, float).reshape(-1)[:kdim] if np.ndim(kvalue) else np.asarray(kvalue, float), (kdim,)).astype(ar.real)
    box = int(max_nstate) if max_nstate else None

    def inside(key):
        return box is None or bool(np.all(np.abs(np.array(key).reshape(-1, kdim)) <= box, axis=1).any())

    def cleared():
        return {v: [np.zeros((len(tab.keys),) + grid, ar.cplx), np.zeros((len(tab.keys),) + grid, ar.cplx)] for v in variables}

    dtab = cleared()                # variable -> [dF, dZ] on tab.keys
    zero_key = (0,) * tab.width
    out = []
    for op, base in zip(ops, plain):
        kind = base[0]
        if kind == "T":
            R, dR = _rotation(ar, base[1], base[2])
            mir = tab.mirror()
            F, B, Z = tab.F, tab.F[mir].conj(), tab.Z
            order1 = _order1(op, T_PARAMS)
            for v in variables:
                dF, dB, dZ = dtab[v][0], dtab[v][0][mir].conj(), dtab[v][1]
                nF = R[..., 0, 0] * dF + R[..., 0, 1] * dB + R[..., 0, 2] * dZ
                nZ = R[..., 2, 0] * dF + R[..., 2, 1] * dB + R[..., 2, 2] * dZ
                for p, c in order1.get(v, {}).items():
                    c = ar.g(c)
                    nF = nF + c * (dR[p][..., 0, 0] * F + dR[p][..., 0, 1] * B + dR[p][..., 0, 2] * Z)
                    nZ = nZ + c * (dR[p][..., 2, 0] * F + dR[p][..., 2, 1] * B + dR[p][..., 2, 2] * Z)
                dtab[v] = [nF, nZ]
            tab.F = R[..., 0, 0] * F + R[..., 0, 1] * B + R[..., 0, 2] * Z
            tab.Z = R[..., 2, 0] * F + R[..., 2, 1] * B + R[..., 2, 2] * Z
        elif kind in ("E", "P"):
            diag, rec, parts = _scalar(ar, kind, base[1:])
            order1 = _order1(op, SCALAR_PARAMS[kind])
            i0 = tab.index[zero_key]
            for v in variables:
                nF, nZ = dtab[v][0] * diag[0], dtab[v][1] * diag[2]
                for p, c in order1.get(v, {}).items():
                    c = ar.g(c)
                    nF = nF + c * (parts[p][0][0] * tab.F)
                    nZ = nZ + c * (parts[p][0][2] * tab.Z)
                    nZ = np.broadcast_to(nZ, (len(tab.keys),) + grid).astype(ar.cplx)
                    nZ[i0] += c * parts[p][1] * dens
                dtab[v] = [nF, nZ]
            tab.F, tab.Z = tab.F * diag[0], tab.Z * diag[2]
            if rec is not None:
                tab.Z[i0] += rec * dens
        elif kind == "S":
            d = _delta(tab, base[1])
            old = dict(tab.index)
            entries = {}
            for i, key in enumerate(tab.keys):
                moved = tuple(int(v) for v in np.array(key) + d)
                if inside(moved):
                    entries.setdefault(moved, [None, None])[0] = tab.F[i]
                if inside(key):
                    entries.setdefault(key, [None, None])[1] = tab.Z[i]
            entries.setdefault(zero_key, [None, None])
            tab.build(entries)
            # the derivative tables: onto the new keys from the same sources (F from key - delta, Z from the key itself)
            src_f = np.array([old.get(tuple(int(v) for v in np.array(key) - d), -1) if inside(key) else -1 for key in tab.keys], dtype=np.int64)
            src_z = np.array([old.get(key, -1) if inside(key) else -1 for key in tab.keys], dtype=np.int64)
            for v in variables:
                dtab[v] = [_gather(dtab[v][0], src_f), _gather(dtab[v][1], src_z)]
        elif kind == "D":
            tau = (ar.g(base[1]) / 1000)
            k = tab.coords().astype(ar.real) * kv / 1000                  # rad/mm, [n, *grid-like, kdim]
            sh = np.zeros(kdim, ar.real)
            if len(base) > 3 and base[3] is not None:
                sh[: len(base[3])] = np.asarray(base[3], float).reshape(-1)
            sh = sh * kv / 1000
            k1 = k - sh

            def outer(a, b):
                return a[..., :, None] * b[..., None, :]

            b_l = outer(k, k)
            b_t = outer(k1, k1) + (outer(k1, sh + 0 * k1) + outer(sh + 0 * k1, k1)) / 2 + outer(sh + 0 * k1, sh + 0 * k1) / 3
            Dv = base[2]
            if isinstance(Dv, tuple) or np.ndim(Dv) == 0:
                dval = ar.g(Dv[1] if isinstance(Dv, tuple) else Dv)
                e_l = np.trace(b_l, axis1=-2, axis2=-1) * dval
                e_t = np.trace(b_t, axis1=-2, axis2=-1) * dval
            else:
                Dm = np.asarray(Dv).astype(ar.real)
                Dm = Dm.reshape(Dm.shape[:-2] + (1,) * (len(grid) - (Dm.ndim - 2)) + Dm.shape[-2:])
                e_l, e_t = np.sum(b_l * Dm, axis=(-2, -1)), np.sum(b_t * Dm, axis=(-2, -1))
            a_t, a_l = np.exp(-e_t * tau), np.exp(-e_l * tau)
            tab.F, tab.Z = tab.F * a_t, tab.Z * a_l
            if through_plain:      # (row i holds dF at the signed coordinate of key i: dF(-c) takes bT of -c, the mirror factor)
                for v in variables:
                    dtab[v] = [dtab[v][0] * a_t, dtab[v][1] * a_l]
        elif kind == "ADC":
            what = base[1] if len(base) > 1 else "F0"
            i0 = tab.index[zero_key]
            rec = np.zeros(grid + (1 + len(variables),), ar.cplx)
            rec[..., 0] = tab.at_zero(what)
            for j, v in enumerate(variables):
                rec[..., 1 + j] = dtab[v][0 if what == "F0" else 1][i0]
            if len(base) > 2 and base[2] is not None:
                rec = rec * np.exp(1j * ar.g(base[2], cplx=True) * ar.pi / 180)[..., None]
            out.append(rec)
        elif kind == "SPOILER":
            tab.F = np.zeros_like(tab.F)
            if through_plain:
                for v in variables:
                    dtab[v][0] = np.zeros_like(dtab[v][0])
        elif kind in ("RESET", "PD"):
            if kind == "PD":
                dens = np.broadcast_to(ar.g(np.atleast_1d(base[1])), grid).astype(ar.real)
            if kind == "RESET" or len(base) < 3 or base[2]:
                tab.equilibrium(dens)
                dtab = cleared()
        elif kind not in ("WAIT", "NULL"):
            raise ValueError(f"unsupported operator {kind}")
        full = (len(tab.keys),) + grid
        tab.F, tab.Z = np.broadcast_to(tab.F, full).astype(ar.cplx), np.broadcast_to(tab.Z, full).astype(ar.cplx)
        for v in variables:
            dtab[v] = [np.broadcast_to(x, full).astype(ar.cplx) for x in dtab[v]]
    records = np.stack(out) if out else np.zeros((0,) + grid + (1 + len(variables),), ar.cplx)
    if not return_state:
        return records
    mir = tab.mirror()

    def table_of(F, Z):
        state = NDState()
        state.lead, state.kdim = tab.lead, tab.kdim
        for i, key in enumerate(tab.keys):      # (coordinates at which nothing was ever put are not part of the state)
            if F[i].any() or Z[i].any() or F[mir[i]].any():
                state[key] = (F[i], Z[i])
        return state

    return records, table_of(tab.F, tab.Z), {v: table_of(*dtab[v]) for v in variables}
