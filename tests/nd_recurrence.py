"""Integer n-D shifts and diffusion in extended precision: the checker of tests/test_gpu_nd_paths.py.

    nd_recurrence(ops, shape=, kvalue=, max_nstate=, init=)      -> records [record, *grid]            (np.clongdouble)
    nd_recurrence(..., return_state=True)                        -> (records, {coordinate: (F, Z)})
    layout(state, coords, grid)                                  -> states [*grid, R, 3] on the rows of `sm.coords`

Shares nothing structural with epgpy_amd/kspace.py or oracle.shift_nd: no sorted rows, no gather tables, no mirror column, no
pruning.  The state is a table from an integer coordinate to (F, Z), F stored at EVERY signed coordinate; what the device
calls B at coordinate c is conj(F(-c)) by definition, and is never stored.

    S(delta)   F(c + delta) <- F(c); Z stays.  An int shift k is [k, 0, ..]; 1-D orders n are coordinates [n, 0, ..].
               With max_nstate a coordinate is dropped only if it lies outside the box |c_i| <= max_nstate in EVERY voxel
               (the reference's shift.py:330-341).
    T E P PD   the closed forms of tests/jacobian_recurrence.py on the row (F(c), conj F(-c), Z(c)); recovery at c = 0
    D          Z(c) *= exp(-tr(bL D)), F(c) *= exp(-tr(bT D)) with  bL = tau k k^T,  k = c kvalue,
               bT = tau (k1 k1^T + (k1 kd^T + kd k1^T) / 2 + kd kd^T / 3),  k1 = k - shift, kd = shift  (`k=` names the shift;
               without it bT = bL): the reference's diffusion.py:60-123, tau in s, k in rad/mm, evaluated in `dtype` from the
               float64 parameters.  F(-c) takes bT of -c: that is the device's "mirror" factor.
    ADC        F(0) or Z(0), times a phase;  SPOILER: F <- 0;  RESET: {0: Z = density}

WHOLE_ROWS.  A vectorised shift (one vector per point of the leading grid axes) gives every voxel its own coordinates.  The
reference then still keeps ROWS: a coordinate of the table is the row's coordinate in every voxel class at once, two pathways
merge only where they coincide in all classes, and a probe reads the row that is zero in all of them (shift.py:461-475
`unique` over whole rows).  A pathway that happens to return to k = 0 in one voxel only is therefore NOT part of that voxel's
F0 -- a quirk of the reference that the library reproduces on purpose; it is the meaning of a key here (WHOLE_ROWS = True,
the only setting implemented: the truncation rule above is stated in terms of such rows)."""
import numpy as np

from tests.jacobian_recurrence import _Arith, _rotation, _scalar

WHOLE_ROWS = True


def _lead_of(shape):
    lead = tuple(int(d) for d in shape)
    while lead and lead[-1] == 1:
        lead = lead[:-1]
    return lead


def _append(a, b):
    """broadcast of two leading shapes, missing axes appended"""
    out = [1] * max(len(a), len(b))
    for s in (a, b):
        for i, d in enumerate(s):
            if d != 1:
                assert out[i] in (1, d), (a, b)
                out[i] = d
    return _lead_of(out)


def nd_grid(ops, shape=None):
    """the grid the tuples span: array parameters, ("field", values) diffusivities, tensors [*lead, d, d], vectorised shifts"""
    nparam = {"T": 2, "E": 4, "P": 2, "PD": 1}
    grid = _lead_of(shape or ())
    for op in ops:
        for a in op[1:1 + nparam.get(op[0], 0)]:
            if not isinstance(a, (bool, dict)):
                grid = _append(grid, np.shape(a))
        if op[0] == "S" and not np.isscalar(op[1]):
            grid = _append(grid, np.shape(op[1])[:-1])
        if op[0] == "D":
            grid = _append(grid, np.shape(op[1]))
            grid = _append(grid, np.shape(op[2][1]) if isinstance(op[2], tuple) else np.shape(op[2])[:-2])
    if shape:
        full = tuple(int(d) for d in shape)
        assert len(grid) <= len(full) and all(g in (1, f) for g, f in zip(grid, full)), (grid, full)
        return full
    return tuple(grid) or (1,)


class _Table:
    """{coordinate key: row}, F [n, *grid] and Z [n, *grid].  A key is the coordinate in every voxel class, flattened:
    lead [*lead, kdim] -> tuple of prod(lead) * kdim ints.  The key set is kept symmetric (c and -c)."""

    def __init__(self, ar, lead, kdim):
        self.ar, self.lead, self.kdim = ar, tuple(lead), kdim
        self.width = int(np.prod(self.lead, dtype=np.int64)) * kdim
        self.keys, self.index = [], {}
        self.F = np.zeros((0,) + ar.grid, ar.cplx)
        self.Z = np.zeros((0,) + ar.grid, ar.cplx)

    def build(self, entries):
        """entries: {key: [F or None, Z or None]}; -key is added for every key"""
        for key in list(entries):
            entries.setdefault(tuple(-v for v in key), [None, None])
        self.keys = list(entries)
        self.index = {k: i for i, k in enumerate(self.keys)}
        zero = np.zeros(self.ar.grid, self.ar.cplx)
        self.F = np.stack([zero if entries[k][0] is None else entries[k][0] for k in self.keys]) if self.keys else self.F[:0]
        self.Z = np.stack([zero if entries[k][1] is None else entries[k][1] for k in self.keys]) if self.keys else self.Z[:0]

    def equilibrium(self, dens):
        self.build({(0,) * self.width: [None, dens.astype(self.ar.cplx)]})

    def mirror(self):
        return np.array([self.index[tuple(-v for v in k)] for k in self.keys], dtype=np.int64)

    def coords(self):
        """[n, *lead-on-grid, kdim] as the wavenumber of every row in every voxel (before kvalue)"""
        c = np.array(self.keys, dtype=np.int64).reshape((len(self.keys),) + self.lead + (self.kdim,))
        return c.reshape((len(self.keys),) + self.lead + (1,) * (len(self.ar.grid) - len(self.lead)) + (self.kdim,))

    def at_zero(self, which):
        return (self.F if which == "F0" else self.Z)[self.index[(0,) * self.width]]


def _delta(tab, k):
    """a shift argument (int, [kdim'] or [*lead', kdim']) -> flat key increment over tab.lead"""
    if np.isscalar(k):
        k = [int(k)]
    k = np.asarray(k, dtype=np.int64)
    lead = _lead_of(k.shape[:-1])
    d = np.zeros(lead + (tab.kdim,), np.int64)
    d[..., : k.shape[-1]] = k.reshape(lead + k.shape[-1:])
    d = d.reshape(lead + (1,) * (len(tab.lead) - len(lead)) + (tab.kdim,))
    return np.broadcast_to(d, tab.lead + (tab.kdim,)).reshape(-1)


def nd_recurrence(ops, *, shape=None, kvalue=1.0, max_nstate=None, init=None, dtype=np.clongdouble, return_state=False):
    """ops: oracle tuples (tests/sequences.py nd_cases / nd_vector_cases); init: (states [*grid-like, R, 3], coords
    [*lead-like, R, kdim]) in the layout of StateMatrix.states / .coords; max_nstate: the truncation box"""
    grid = nd_grid(ops, shape)
    ar = _Arith(grid, dtype)
    lead, kdim = (), 1
    for op in ops:
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

    out = []
    for op in ops:
        kind = op[0]
        if kind == "T":
            R, _ = _rotation(ar, op[1], op[2])
            F, B, Z = tab.F, tab.F[tab.mirror()].conj(), tab.Z
            tab.F = R[..., 0, 0] * F + R[..., 0, 1] * B + R[..., 0, 2] * Z
            tab.Z = R[..., 2, 0] * F + R[..., 2, 1] * B + R[..., 2, 2] * Z
        elif kind in ("E", "P"):
            diag, rec, _ = _scalar(ar, kind, op[1:])
            tab.F, tab.Z = tab.F * diag[0], tab.Z * diag[2]
            if rec is not None:
                tab.Z[tab.index[(0,) * tab.width]] += rec * dens
        elif kind == "S":
            d = _delta(tab, op[1])
            entries = {}
            for i, key in enumerate(tab.keys):
                moved = tuple(int(v) for v in np.array(key) + d)
                if inside(moved):
                    entries.setdefault(moved, [None, None])[0] = tab.F[i]
                if inside(key):
                    entries.setdefault(key, [None, None])[1] = tab.Z[i]
            entries.setdefault((0,) * tab.width, [None, None])
            tab.build(entries)
        elif kind == "D":
            tau = (ar.g(op[1]) / 1000)
            k = tab.coords().astype(ar.real) * kv / 1000                  # rad/mm, [n, *grid-like, kdim]
            sh = np.zeros(kdim, ar.real)
            if len(op) > 3 and op[3] is not None:
                sh[: len(op[3])] = np.asarray(op[3], float).reshape(-1)
            sh = sh * kv / 1000
            k1 = k - sh

            def outer(a, b):
                return a[..., :, None] * b[..., None, :]

            b_l = outer(k, k)
            b_t = outer(k1, k1) + (outer(k1, sh + 0 * k1) + outer(sh + 0 * k1, k1)) / 2 + outer(sh + 0 * k1, sh + 0 * k1) / 3
            Dv = op[2]
            if isinstance(Dv, tuple) or np.ndim(Dv) == 0:
                dval = ar.g(Dv[1] if isinstance(Dv, tuple) else Dv)
                e_l = np.trace(b_l, axis1=-2, axis2=-1) * dval
                e_t = np.trace(b_t, axis1=-2, axis2=-1) * dval
            else:
                Dm = np.asarray(Dv).astype(ar.real)
                Dm = Dm.reshape(Dm.shape[:-2] + (1,) * (len(grid) - (Dm.ndim - 2)) + Dm.shape[-2:])
                e_l, e_t = np.sum(b_l * Dm, axis=(-2, -1)), np.sum(b_t * Dm, axis=(-2, -1))
            tab.F, tab.Z = tab.F * np.exp(-e_t * tau), tab.Z * np.exp(-e_l * tau)
        elif kind == "ADC":
            what = op[1] if len(op) > 1 else "F0"
            rec = np.array(tab.at_zero(what))
            if len(op) > 2 and op[2] is not None:
                rec = rec * np.exp(1j * ar.g(op[2], cplx=True) * ar.pi / 180)
            out.append(rec)
        elif kind == "SPOILER":
            tab.F = np.zeros_like(tab.F)
        elif kind in ("RESET", "PD"):
            if kind == "PD":
                dens = np.broadcast_to(ar.g(np.atleast_1d(op[1])), grid).astype(ar.real)
            if kind == "RESET" or len(op) < 3 or op[2]:
                tab.equilibrium(dens)
        elif kind not in ("WAIT", "NULL"):
            raise ValueError(f"unsupported operator {kind}")
        tab.F, tab.Z = np.broadcast_to(tab.F, (len(tab.keys),) + grid).astype(ar.cplx), np.broadcast_to(tab.Z, (len(tab.keys),) + grid).astype(ar.cplx)
    records = np.stack(out) if out else np.zeros((0,) + grid, ar.cplx)
    if not return_state:
        return records
    mir = tab.mirror()
    state = NDState()
    state.lead, state.kdim = tab.lead, tab.kdim
    for i, key in enumerate(tab.keys):      # (coordinates at which nothing was ever put are not part of the state)
        if tab.F[i].any() or tab.Z[i].any() or tab.F[mir[i]].any():
            state[key] = (tab.F[i], tab.Z[i])
    return records, state


class NDState(dict):
    """{coordinate key: (F [*grid], Z [*grid])} and the form of its keys: `lead` voxel classes x `kdim` components"""
    lead, kdim = (), 1


def _canon(key, kdim, nclass, kdim_to, nclass_to):
    """a key over `nclass` classes x `kdim` components as one over nclass_to x kdim_to (zero padded, repeated)"""
    arr = np.zeros((nclass, kdim_to), np.int64)
    arr[:, :kdim] = np.array(key, dtype=np.int64).reshape(nclass, kdim)
    assert nclass in (1, nclass_to), (nclass, nclass_to)
    return tuple(int(v) for v in np.broadcast_to(arr, (nclass_to, kdim_to)).reshape(-1))


def coord_keys(coords):
    """coords [*lead-like, R, kdim] -> R keys: the coordinate of a row in every voxel class, flattened"""
    coords = np.asarray(coords)
    lead = _lead_of(coords.shape[:-2])
    c = coords.reshape(lead + coords.shape[-2:])
    return [tuple(int(v) for v in c[..., r, :].reshape(-1)) for r in range(c.shape[-2])]


def layout(state, coords, grid):
    """the final table on the rows of `coords` (StateMatrix.coords, or KSpace.coords): [*grid, R, 3] with columns F(c),
    conj F(-c), Z(c); a row whose coordinate the table does not hold is zero.  Every coordinate the table holds must be a row
    (the planner's structural pruning may not have dropped it).  Leading axes of `coords` are leading grid axes."""
    coords = np.asarray(coords)
    lead = _lead_of(coords.shape[:-2])
    both = _append(lead, state.lead)
    kd_c, kd = coords.shape[-1], max(coords.shape[-1], state.kdim)
    n_c, n_s, n = (int(np.prod(x, dtype=np.int64)) for x in (lead, state.lead, both))
    c = coords.reshape(lead + coords.shape[-2:])
    c = np.broadcast_to(c.reshape(lead + (1,) * (len(both) - len(lead)) + c.shape[-2:]), both + c.shape[-2:])
    keys = [_canon(tuple(int(v) for v in c[..., r, :].reshape(-1)), kd_c, n, kd, n) for r in range(c.shape[-2])]
    have = {}
    for key, val in state.items():
        arr = np.array(key, dtype=np.int64).reshape(state.lead + (state.kdim,))
        arr = np.broadcast_to(arr.reshape(state.lead + (1,) * (len(both) - len(state.lead)) + (state.kdim,)), both + (state.kdim,))
        have[_canon(tuple(int(v) for v in arr.reshape(-1)), state.kdim, n, kd, n)] = val
    rows = set(keys)
    missing = [k for k in have if k not in rows]
    assert not missing, ("coordinates the reference holds that are not rows of the device state", missing[:4])
    assert len(rows) == len(keys), "coords: rows must be distinct"
    out = np.zeros(tuple(grid) + (len(keys), 3), next(iter(state.values()))[0].dtype if state else np.clongdouble)
    for r, key in enumerate(keys):
        if key in have:
            out[..., r, 0], out[..., r, 2] = have[key]
        neg = tuple(-v for v in key)
        if neg in have:
            out[..., r, 1] = have[neg][0].conj()
    return out
