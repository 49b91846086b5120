"""Plan-level collapse of a run of state-wise operators into ONE operator whose table the device multiplies up.

A sampled RF pulse (rfpulse.RFPulse) flattens into N small rotations with a relaxation / precession between them: 2 N .. 3 N
primitive records, each walked over every order of every voxel, per use of the pulse.  But the run holds no shift and no
probe: it is ONE affine map  x -> M x + o  per voxel, the same at every order (o acts on the k = 0 order only, through the
density), and M keeps the EPG symmetry.  That is exactly an EPGX_OP_MAT0 record.  Unlike the E . T . E fusion (fusion.py) the
members may precess (complex e0) and there is no table per member: the library runs the whole product in registers, one lane
per table entry (include/epgx.h epgx_chain, csrc/epgx_chain.hip), once per distinct pulse object and plan.

Only MultiOperators flagged `collapsible` are considered (RFPulse, and what `modify` / `encode_phase` return for one).  One
stays whole when every member is a MatrixOp or ScalarOp; it is expanded into its members -- the same results to rounding --
when a member carries partials for one of the plan's variables, when the plan would need more than its index spaces, or when
the generated tables would exceed the budget (14 doubles per entry and distinct pulse object).
"""
import numpy as np

from . import common, operator, opmatrix, opscalar, _lib


def eligible(multi):
    """True if every (flattened) member of a MultiOperator is a state-wise matrix / scalar operator of the library"""
    members = multi.operators      # (flat: a MultiOperator dissolves the MultiOperators it takes)
    return bool(members) and all(isinstance(op, (opmatrix.MatrixOp, opscalar.ScalarOp)) and not op._on_host() for op in members)


def _packed(op):
    if op._packed is None:
        op._packed = (opmatrix.pack_matrix(op.mat, op.mat0) if isinstance(op, opmatrix.MatrixOp)
                      else opscalar.pack_scalar(op.arr, op.arr0))
    return op._packed


def _signature(op):
    """what two members must share to be repetitions of one step: the layout and shape of their tables"""
    if isinstance(op, opscalar.ScalarOp):
        return (_lib.OP_E, tuple(op.arr.shape[:-1]))
    opcode, table = _packed(op)
    return (opcode, tuple(table.shape[:-1]))


def group_members(members):
    """[(count, [position 0: its operator in every repetition, position 1: ...])]: the members cut into groups of at most
    CHAIN_GROUP steps that repeat `count` times with tables of the same layout -- a pulse T_0 E T_1 E ... is ONE group
    (T_i, E) with count = N"""
    sig = [_signature(op) for op in members]
    out, i, n = [], 0, len(members)
    while i < n:
        group, count = 1, 1
        for g in range(1, _lib.CHAIN_GROUP + 1):
            c = 1
            while i + (c + 1) * g <= n and sig[i + c * g: i + (c + 1) * g] == sig[i: i + g]:
                c += 1
            if c > 1 and c * g > group * count:
                group, count = g, c
        out.append((count, [[members[i + r * group + j] for r in range(count)] for j in range(group)]))
        i += group * count
    return out


class Collapsed(operator.Operator):
    """a collapsible MultiOperator as ONE operator.  Holds the recipe, not the numbers: the library multiplies the members up
    on the device when the plan is created (epgx_chain)"""

    def __init__(self, source):
        self.source = source
        self.members = tuple(source.operators)
        self._shape = tuple(common.broadcast_shapes(*[op.shape for op in self.members], append=True))
        self.groups = group_members(self.members)
        super().__init__(name=f"[{source.name}]", duration=source.duration)

    @property
    def shape(self):
        return self._shape

    @property
    def n_steps(self):
        return sum(len(positions) for _, positions in self.groups)

    def _entry(self, enc):
        """pool entry (space, offset, 14) of the collapsed table; registers the recipe once per plan"""
        key = ("CHAIN", id(self))
        if key in enc.generated:
            return enc.generated[key]
        steps = []
        for g, (count, positions) in enumerate(self.groups):
            for j, ops in enumerate(positions):
                first = ops[0]
                if all(op is first for op in ops):           # the same table in every repetition
                    if isinstance(first, opscalar.ScalarOp):
                        entry, kind = first._pool_entry(enc), _lib.OP_E      # (uploaded, or assembled on the device)
                    else:
                        kind, table = _packed(first)
                        entry = enc._table(table, ("MAT", id(first)))
                    stride = 0
                else:                                        # one table per repetition, laid out one after the other
                    kind = _packed(first)[0]
                    entry, stride = enc.table_run([_packed(op)[1] for op in ops], ("RUN", id(self), g, j))
                steps.append((entry, stride, kind, count if j == 0 else 0, len(positions) if j == 0 else 0))
        entry, _ = enc._generated(self._shape, 14, key, sources=[st[0][0] for st in steps])
        enc.add_chain(entry, steps)
        return entry

    def _encode(self, enc):
        enc.add(_lib.OP_MAT0, entry=self._entry(enc))
        enc.note("mix")
        enc.note("relax")

    def host_table(self):
        """the same table computed with NumPy, in the order of operations of chain_kernel (tests; the product path never
        calls this): [*shape, 14] in the EPGX_OP_MAT0 layout"""
        nd = len(self._shape)

        def lead(table):
            shape = table.shape[:-1]
            return np.moveaxis(table.reshape(shape + (1,) * (nd - len(shape)) + table.shape[-1:]), -1, 0)

        one, zero = np.ones(self._shape), np.zeros(self._shape)
        ur, ui, pr, pi, qr, qi, tr, ti, c, o0r, o0i, o2 = one, zero, zero, zero, zero, zero, zero, zero, one, zero, zero, zero
        for count, positions in self.groups:
            for r in range(count):
                for ops in positions:
                    opcode, table = _packed(ops[r])
                    t = lead(table)
                    if opcode == _lib.OP_E:
                        er, ei, e2, rec = t
                        ur, ui = er * ur - ei * ui, er * ui + ei * ur
                        pr, pi = er * pr - ei * pi, er * pi + ei * pr
                        qr, qi = er * qr - ei * qi, er * qi + ei * qr
                        o0r, o0i = er * o0r - ei * o0i, er * o0i + ei * o0r
                        tr, ti, c = tr * e2, ti * e2, c * e2
                        o2 = e2 * o2 + rec
                        continue
                    if opcode == _lib.OP_T:
                        aur, apr, api, aqr, aqi, atr, ati, ac = t
                        aui = aar = aai = aa2 = 0.0
                    else:
                        aur, aui, apr, api, aqr, aqi, atr, ati, ac = t[:9]
                        aar, aai, aa2 = (t[10], t[11], t[12]) if opcode == _lib.OP_MAT0 else (0.0, 0.0, 0.0)
                    n_ur = aur * ur - aui * ui + (apr * pr + api * pi) + (aqr * tr - aqi * ti)
                    n_ui = aur * ui + aui * ur + (api * pr - apr * pi) + (aqr * ti + aqi * tr)
                    n_pr = aur * pr - aui * pi + (apr * ur + api * ui) + (aqr * tr + aqi * ti)
                    n_pi = aur * pi + aui * pr + (api * ur - apr * ui) + (aqi * tr - aqr * ti)
                    n_qr = aur * qr - aui * qi + (apr * qr + api * qi) + aqr * c
                    n_qi = aur * qi + aui * qr + (api * qr - apr * qi) + aqi * c
                    n_tr = atr * ur - ati * ui + (atr * pr - ati * pi) + ac * tr
                    n_ti = atr * ui + ati * ur - (atr * pi + ati * pr) + ac * ti
                    n_c = 2.0 * (atr * qr - ati * qi) + ac * c
                    n_o0r = aur * o0r - aui * o0i + (apr * o0r + api * o0i) + aqr * o2 + aar
                    n_o0i = aur * o0i + aui * o0r + (api * o0r - apr * o0i) + aqi * o2 + aai
                    n_o2 = 2.0 * (atr * o0r - ati * o0i) + ac * o2 + aa2
                    ur, ui, pr, pi, qr, qi, tr, ti, c, o0r, o0i, o2 = n_ur, n_ui, n_pr, n_pi, n_qr, n_qi, n_tr, n_ti, n_c, n_o0r, n_o0i, n_o2
        cols = [ur, ui, pr, pi, qr, qi, tr, ti, c, zero, o0r, o0i, o2, zero]
        return np.stack([np.broadcast_to(col, self._shape) for col in cols], axis=-1)


def collapsed_of(multi):
    """the Collapsed operator of a MultiOperator: built once per object and kept on it (a train uses its pulse echo after
    echo, a fitting loop simulate() after simulate()); rebuilt when the operator has grown since (`append`)"""
    members = tuple(multi.operators)
    known = multi.__dict__.get("_collapsed")
    if known is None or len(known.members) != len(members) or any(a is not b for a, b in zip(known.members, members)):
        known = multi.__dict__["_collapsed"] = Collapsed(multi)
    return known


def _varies(shape):
    return tuple(d for d, n in enumerate(shape) if n > 1)


def generated_bytes(sequence):
    """bytes of device-generated tables the Collapsed operators of a sequence ask for: 14 doubles per entry, once per object"""
    seen = {id(op): int(np.prod(op.shape)) * 14 * 8 for op in sequence if isinstance(op, Collapsed)}
    return sum(seen.values())


def resolve(sequence, grid, variables, budget):
    """a flat sequence in which collapsible MultiOperators were kept whole -> one with a Collapsed operator for each, or with
    its members where the plan cannot take the collapsed form (module docstring); other operators pass through"""
    if not any(isinstance(op, operator.MultiOperator) for op in sequence):
        return sequence
    variables = set(variables or ())
    whole = {}
    for op in sequence:
        if isinstance(op, operator.MultiOperator) and id(op) not in whole:
            differentiated = any(variables & set(getattr(part, "order1", None) or {}) for part in op.operators)
            whole[id(op)] = None if differentiated else collapsed_of(op)
    # the broadcast patterns of the plan's tables: a plan has MAX_SPACES index spaces, past them tables are materialised over
    # larger spaces -- the collapsed tables, one entry per voxel of their shape, are the ones that give way
    patterns = {_varies(part.shape) for op in sequence for part in (whole.get(id(op)) and [whole[id(op)]] or op._parts())}
    patterns |= {_varies(part.shape) for col in whole.values() if col is not None for part in col.members}
    patterns.discard(())
    nbytes = sum({id(col): int(np.prod(col.shape)) * 14 * 8 for col in whole.values() if col is not None}.values())
    if len(patterns) > _lib.MAX_SPACES or nbytes > budget:
        whole = dict.fromkeys(whole)
    out = []
    for op in sequence:
        if isinstance(op, operator.MultiOperator):
            out.extend([whole[id(op)]] if whole[id(op)] is not None else op._parts())
        else:
            out.append(op)
    return out
