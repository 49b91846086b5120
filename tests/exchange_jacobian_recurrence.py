"""The EPG-X recurrence of tests/exchange_recurrence.py with first-order derivative states (include/epgx.h, EPGX_OP_X):

    dS_v <- Op(dS_v, no equilibrium term) + (dOp/dv)(S)      S <- Op(S)

per operator, the partial acting on the state BEFORE the update.  X always acts on the derivative states; SPOILER only with
`through_plain` (simulate(exact_partials=True)); RESET and PD-with-reset always clear them.  The partial of a constant term
(the recovery of E, the densities X relaxes to) goes to order 0 only, and the densities depend on no variable.

Like the plain recurrence it works on the operators' own float64 tables (`_variable_tables()` for the partials), so that
`dtype=np.clongdouble` measures the kernels' arithmetic.  That the tables and both sign conventions are right is pinned
separately: central differences of the PLAIN recurrence (tests/test_exchange_partials_host.py).

CASES are the sequences of tests/test_gpu_exchange_jacobian.py, one per dxrun_kernel<NC, M, V> instantiation; FLOORS what
the float64 recurrence achieves on them against the extended one, per column (the project's 16 x floor convention)."""
import numpy as np

from epgpy_amd import epg, exchange
from tests.exchange_recurrence import _bcast, _grid_array, _truncate


def _x_matrices(tab, n, ax, grid, dtype):
    """device table [*lead (1 at ax), 3 n^2] -> (mT, mL) [*grid without ax, n, n]"""
    lead = tab.shape[:-1]
    mT = tab[..., : 2 * n * n].reshape(lead + (n, n, 2))
    mT = mT[..., 0].astype(dtype) + 1j * mT[..., 1].astype(dtype)
    mL = tab[..., 2 * n * n:].reshape(lead + (n, n)).astype(dtype)
    take = lambda m: np.moveaxis(_bcast(m, lead, grid), ax, -3)[..., 0, :, :]
    return take(mT), take(mL)


def _x_mix(st, mT, mL, ax):
    """every order of [*grid, rows, 3] mixed over the compartments along `ax`"""
    sub = np.moveaxis(st, ax, -1)                    # [..., rows, 3, N]
    new = np.empty_like(sub)
    new[..., 0, :] = np.einsum("...ij,...rj->...ri", mT, sub[..., 0, :])
    new[..., 1, :] = np.einsum("...ij,...rj->...ri", mT.conj(), sub[..., 1, :])
    new[..., 2, :] = np.einsum("...ij,...rj->...ri", mL, sub[..., 2, :])
    return np.moveaxis(new, -1, ax)


def _matrix_partial(tab, dtype):
    """10-coefficient table of d(mat)/dv -> [*lead, 3, 3] (the layout of EPGX_OP_MAT)"""
    tab = tab.astype(np.finfo(dtype).dtype)
    u, p, q, t = (tab[..., 2 * i] + 1j * tab[..., 2 * i + 1] for i in range(4))
    mat = np.empty(tab.shape[:-1] + (3, 3), dtype=dtype)
    mat[..., 0, 0], mat[..., 0, 1], mat[..., 0, 2] = u, p, q
    mat[..., 1, 0], mat[..., 1, 1], mat[..., 1, 2] = p.conj(), u.conj(), q.conj()
    mat[..., 2, 0], mat[..., 2, 1], mat[..., 2, 2] = t, t.conj(), tab[..., 8]
    return mat


def exchange_jacobian_recurrence(seq, variables, grid, density, nmax, *, dtype=np.complex128, max_nstate=None, through_plain=False):
    """probe records [n_probe, *grid, 1 + V] (the state's, then d/d variables[v]) of `seq`: T / E / P / R with order1, X with
    order1, S, SPOILER, RESET, PD, probes (F0, or Z0 for Adc("Z0"))"""
    grid = tuple(grid)
    real = np.finfo(dtype).dtype
    dens = _grid_array(density, grid, real)
    st = np.zeros(grid + (2 * nmax + 1, 3), dtype=dtype)
    st[..., nmax, 2] = dens
    dst = [np.zeros_like(st) for _ in variables]
    out = []
    for op in seq:
        tables = op._variable_tables() if getattr(op, "order1", None) else {}
        if isinstance(op, epg.X):
            ax, n = op.axis, op.ncomp
            mT, mL = _x_matrices(op._table(), n, ax, grid, dtype)
            sub = st.copy()
            sub[..., nmax, 2] -= dens                 # Z_0 - rho is what exchanges
            for v, var in enumerate(variables):
                dst[v] = _x_mix(dst[v], mT, mL, ax)
                if var in tables:
                    dst[v] = dst[v] + _x_mix(sub, *_x_matrices(tables[var], n, ax, grid, dtype), ax)
            st = _x_mix(sub, mT, mL, ax)
            st[..., nmax, 2] += dens
        elif isinstance(op, epg.MatrixOp):
            mat = _bcast(op.mat, op.mat.shape[:-2], grid).astype(dtype)
            for v, var in enumerate(variables):
                dst[v] = np.einsum("...ij,...rj->...ri", mat, dst[v])
                if var in tables:
                    dmat = _matrix_partial(tables[var], dtype)
                    dst[v] = dst[v] + np.einsum("...ij,...rj->...ri", _bcast(dmat, dmat.shape[:-2], grid), st)
            st = np.einsum("...ij,...rj->...ri", mat, st)
            if op.mat0 is not None:
                st[..., nmax, :] += _bcast(op.mat0, op.mat0.shape[:-2], grid)[..., :, 2].astype(dtype) * dens[..., None]
        elif isinstance(op, epg.ScalarOp):
            arr = _bcast(op.arr, op.arr.shape[:-1], grid).astype(dtype)
            for v, var in enumerate(variables):
                dst[v] = dst[v] * arr[..., None, :]
                if var in tables:
                    tab = _bcast(tables[var], tables[var].shape[:-1], grid).astype(real)
                    e0 = tab[..., 0] + 1j * tab[..., 1]
                    darr = np.stack([e0, e0.conj(), tab[..., 2] + 0j], axis=-1).astype(dtype)
                    dst[v] = dst[v] + st * darr[..., None, :]
                    dst[v][..., nmax, 2] += tab[..., 3] * dens
            st = st * arr[..., None, :]
            if op.arr0 is not None:
                st[..., nmax, 2] += _bcast(op.arr0, op.arr0.shape[:-1], grid)[..., 2].astype(dtype) * dens
        elif isinstance(op, epg.S):
            st, dst = _shift(st, op, nmax, max_nstate), [_shift(d, op, nmax, max_nstate) for d in dst]
        elif op is epg.SPOILER:
            st = st.copy()
            st[..., :2] = 0
            if through_plain:
                for d in dst:
                    d[..., :2] = 0
        elif op is epg.RESET or isinstance(op, epg.PD):
            if isinstance(op, epg.PD):
                dens = _grid_array(op.pd, grid, real)
            if op is epg.RESET or op.reset:
                st = np.zeros_like(st)
                st[..., nmax, 2] = dens
                dst = [np.zeros_like(st) for _ in variables]
        elif isinstance(op, epg.Probe):
            col = 2 if op._device_kind() == 1 else 0
            out.append(np.stack([st[..., nmax, col]] + [d[..., nmax, col] for d in dst], axis=-1))
        else:
            raise TypeError(op)
    return np.stack(out)


def _shift(st, op, nmax, max_nstate):
    k = int(op.k)
    new = np.zeros_like(st)
    rows = st.shape[-2]
    if k > 0:
        new[..., k:, 0] = st[..., : rows - k, 0]
        new[..., : rows - k, 1] = st[..., k:, 1]
    else:
        new[..., : rows + k, 0] = st[..., -k:, 0]
        new[..., -k:, 1] = st[..., : rows + k, 1]
    new[..., 2] = st[..., 2]
    return _truncate(new, nmax, max_nstate or op.nmax or None)


def column_errors(got, want):
    """per column v: max|got[..., v] - want[..., v]| / max|want[..., v]|"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = []
    for v in range(want.shape[-1]):
        scale = float(np.max(np.abs(want[..., v])))
        assert scale > 0, f"column {v} of the reference is zero: the case does not exercise it"
        out.append(float(np.max(np.abs(got[..., v] - want[..., v]))) / scale)
    return out


# ------------------------------------------------------------------------------------------------------------- cases
def _spgr(x, alpha, ntr, *, relax=None, spoil=None, alpha_o1=None):
    """RF-spoiled gradient echo: quadratic phase, exchange during TR; `relax`: an E next to the rotation (foldable)"""
    seq = []
    for j in range(ntr):
        seq += [epg.T(alpha, 58.5 * j * (j + 1), **({"order1": alpha_o1} if alpha_o1 else {}))]
        seq += [relax] if relax is not None else []
        seq += [epg.ADC, x, epg.S(1)]
        seq += [spoil] if (spoil is not None and j % 4 == 3) else []
    return seq


def case_2_1_1():
    """compartments FIRST on a 2 x 3 x 2 grid (stride 6), T1 varies along axis 1, the flip angle along axis 2; variable: the
    exchange rate (X only).  PD with reset sets the pool fractions"""
    dens = np.array([0.8, 0.2])
    T1 = np.array([[900.0, 1100.0, 1300.0], [250.0, 300.0, 350.0]])
    x = epg.X(6.0, 0.04 * exchange.exchange_matrix(1.0, densities=dens), T1=T1, T2=[70.0, 12.0], g=[0.0, 0.02],
              dkhi=exchange.exchange_matrix(1.0, densities=dens), order1={"k": {"khi": 1}})
    alpha = np.array([[[12.0, 35.0]]])
    seq = [epg.PD(dens)] + _spgr(x, alpha, 12)
    return dict(seq=seq, variables=["k"], grid=(2, 3, 2), nmax=12, kernel="dxrun_kernel<2, 1, 1>")


def case_2_1_2():
    """bSSFP-like train with a foldable E on either side of T; variables: B1 (T only: X carries no partial) and T1, declared
    by E AND X (array-valued T1 per compartment).  S(1) / S(-1)"""
    T1, T2 = np.array([1000.0, 400.0]), np.array([80.0, 20.0])
    x = epg.X(2.0, 0.03, T1=T1, T2=T2, order1={"T1": {"T1": 1}})
    e = epg.E(1.5, T1, T2, order1={"T1": {"T1": 1}})
    alpha = np.array([[20.0, 45.0, 70.0]])
    seq = [epg.T(alpha / 2, 0, order1={"B1": {"alpha": alpha / 2}}), e]
    for j in range(12):
        seq += [e, epg.T(alpha, 180.0 * (j % 2), order1={"B1": {"alpha": alpha}}), e, epg.ADC, x, epg.S(1), epg.S(-1) if j % 3 == 2 else x]
    return dict(seq=seq, variables=["B1", "T1"], grid=(2, 3), nmax=12, kernel="dxrun_kernel<2, 1, 2>")


def _case_2_1_3(exact):
    """compartments LAST (stride 1) on a 3 x 2 grid, khi varies along axis 0; variables of X only: tau, the second pool's T2
    (a coefficient array along the compartment axis) and g; S(2) (LDS path), S(-1), truncation at max_nstate = 9, SPOILER, RESET,
    PD with and without reset, F0 and Z0 probes"""
    khi = exchange.exchange_matrix([0.01, 0.03, 0.08], axis=1)
    x = epg.X(4.0, khi, axis=1, T1=[[900.0, 300.0]], T2=[[60.0, 15.0]], g=[[0.01, -0.03]],
              order1={"tau": {"tau": 1}, "T2b": {"T2": [[0.0, 1.0]]}, "g": {"g": 1}})
    seq = []
    for j in range(12):
        seq += [epg.T(30.0 + 5 * j, 20.0 * j), x, epg.ADC, epg.Adc("Z0"), epg.S(2) if j % 2 else epg.S(1)]
        if j == 3:
            seq += [epg.SPOILER, x]
        if j == 5:
            seq += [epg.S(-1), epg.PD([[0.7, 0.3]], reset=False), x]
        if j == 8:
            seq += [epg.RESET]
        if j == 9:
            seq += [epg.PD([[0.6, 0.4]]), x]
    return dict(seq=seq, variables=["tau", "T2b", "g"], grid=(3, 2), nmax=20, max_nstate=9, exact=exact, kernel="dxrun_kernel<2, 1, 3>")


def case_2_1_3():
    return _case_2_1_3(False)


def case_2_1_3_exact():
    return _case_2_1_3(True)


def case_3_1_1():
    """three compartments, a kinetic matrix with detailed balance; variable: its scale (dkhi = khi / scale); spoiled train"""
    dens = np.array([0.6, 0.3, 0.1])
    rng = np.random.default_rng(5)
    from tests.exchange_recurrence import conserving_khi
    khi = conserving_khi(rng, dens, 0.02)
    x = epg.X(5.0, khi, T1=[1000.0, 600.0, 300.0], T2=[[90.0, 85.0], [40.0, 35.0], [12.0, 10.0]], g=[0.0, 0.01, -0.02],
              dkhi=khi / 0.02, order1={"k": {"khi": 1}})
    seq = [epg.PD(dens)] + _spgr(x, 25.0, 12, spoil=epg.SPOILER)
    return dict(seq=seq, variables=["k"], grid=(3, 2), nmax=12, kernel="dxrun_kernel<3, 1, 1>")


def case_4_1_1():
    """four compartments; variable: T2 of all compartments together (scalar coefficient), declared by X and by the E next to T"""
    T2 = np.array([100.0, 60.0, 30.0, 10.0])
    x = epg.X(5.0, exchange.exchange_matrix(0.05, ncomp=4), T1=[1200.0, 900.0, 600.0, 300.0], T2=T2, order1={"T2": {"T2": 1}})
    e = epg.E(1.0, [1200.0, 900.0, 600.0, 300.0], T2, order1={"T2": {"T2": 1}})
    seq = _spgr(x, np.array([[15.0, 40.0, 65.0]]), 12, relax=e)
    return dict(seq=seq, variables=["T2"], grid=(4, 3), nmax=12, kernel="dxrun_kernel<4, 1, 1>")


def case_2_2_1():
    """the smallest train past 64 orders: S(3) x 24 = 72 orders, K = 128; variable: T1 of the first pool (X only)"""
    x = epg.X(3.0, 0.05, T1=[800.0, 300.0], T2=[[60.0, 50.0, 40.0], [15.0, 12.0, 10.0]], order1={"T1a": {"T1": [1.0, 0.0]}})
    seq = []
    for j in range(24):
        seq += [epg.T(20.0 + j, 90.0), x, epg.ADC, epg.S(3)]
    seq += [epg.S(-3), epg.ADC]
    return dict(seq=seq, variables=["T1a"], grid=(2, 3), nmax=72, kernel="dxrun_kernel<2, 2, 1>")


CASES = {"x_2_1_1": case_2_1_1, "x_2_1_2": case_2_1_2, "x_2_1_3": case_2_1_3, "x_2_1_3_exact": case_2_1_3_exact,
         "x_3_1_1": case_3_1_1, "x_4_1_1": case_4_1_1, "x_2_2_1": case_2_2_1}

# float64 recurrence against the extended one, largest column (tests/test_exchange_partials_host.py measures and prints them;
# the values here are those measurements rounded up)
FLOORS = {"x_2_1_1": 3e-15, "x_2_1_2": 4e-16, "x_2_1_3": 4e-16, "x_2_1_3_exact": 4e-16, "x_3_1_1": 6e-15, "x_4_1_1": 2e-16,
          "x_2_2_1": 4e-16, "khi0_x": 7e-16, "khi0_e": 9e-16}

def run_case(c, dtype=np.complex128):
    return exchange_jacobian_recurrence(c["seq"], c["variables"], c["grid"], 1.0, c["nmax"], dtype=dtype,
                                        max_nstate=c.get("max_nstate"), through_plain=c.get("exact", False))


# ------------------------------------------------------------- finite differences of the PLAIN recurrence (and of the kernel)
FD_POINT = {"alpha": 30.0, "k": 0.04, "T1": 900.0, "T2b": 14.0, "g": 0.015, "tau": 5.0}


def fd_sequence(p, order1=True):
    """a two-pool spoiled train as a function of the parameter vector p; every X parameter and a T parameter once.
    order1=False: the plain operators (what central differences run)"""
    dens = np.array([0.85, 0.15])
    o1 = (lambda d: {"order1": d}) if order1 else (lambda d: {})
    x = epg.X(p["tau"], p["k"] * exchange.exchange_matrix(1.0, densities=dens), T1=[p["T1"], 0.4 * p["T1"]], T2=[70.0, p["T2b"]],
              g=[0.0, p["g"]], dkhi=exchange.exchange_matrix(1.0, densities=dens),
              **o1({"k": {"khi": 1}, "T1": {"T1": [1.0, 0.4]}, "T2b": {"T2": [0.0, 1.0]}, "g": {"g": [0.0, 1.0]}, "tau": {"tau": 1}}))
    e = epg.E(1.0, [p["T1"], 0.4 * p["T1"]], [70.0, p["T2b"]], **o1({"T1": {"T1": [1.0, 0.4]}, "T2b": {"T2": [0.0, 1.0]}}))
    seq = [epg.PD(dens)]
    for j in range(8):
        seq += [epg.T(p["alpha"], 58.5 * j * (j + 1), **o1({"alpha": {"alpha": 1}})), e, epg.ADC, epg.Adc("Z0"), x, epg.S(1)]
    return seq


FD_VARIABLES = ["alpha", "k", "T1", "T2b", "g", "tau"]


def richardson(f, x, h):
    """central differences with steps h and h / 2, combined (error O(h^4))"""
    d1 = (f(x + h) - f(x - h)) / (2 * h)
    d2 = (f(x + h / 2) - f(x - h / 2)) / h
    return (4 * d2 - d1) / 3


FD_STEP = 1e-3      # relative step of the central differences (with h and h / 2: error O(h^4) + rounding / h)


def fd_jacobian(run, variables=FD_VARIABLES):
    """[n_probe, *grid, V]: Richardson central differences of run(sequence without order1) -> [n_probe, *grid]"""
    cols = []
    for var in variables:
        f = lambda val, var=var: run(fd_sequence({**FD_POINT, var: float(val)}, order1=False))
        cols.append(richardson(f, FD_POINT[var], FD_STEP * FD_POINT[var]))
    return np.stack(cols, axis=-1)


def fd_reference():
    """the extended-precision Jacobian of fd_sequence at FD_POINT: [n_probe, 2, 1 + V]"""
    return exchange_jacobian_recurrence(fd_sequence(FD_POINT), FD_VARIABLES, (2,), 1.0, 9, dtype=np.clongdouble)


def fd_host_errors():
    """per variable: error of the float64 HOST recurrence's finite differences against the extended derivative, relative to
    the column's largest entry -- what a float64 finite difference of this train and step can achieve"""
    from tests.exchange_recurrence import recurrence
    ref = fd_reference()[..., 1:]
    fd = fd_jacobian(lambda seq: recurrence(seq, (2,), 1.0, 9))
    return column_errors(fd, ref)


# khi = 0: X is a relaxation per compartment -- the same train with E runs on the existing derivative kernels
def khi0_sequences():
    T1, T2 = np.array([900.0, 300.0]), np.array([70.0, 15.0])
    o1 = {"T1": {"T1": 1}, "T2": {"T2": 1}}
    x = epg.X(5.0, 0.0, T1=T1, T2=T2, order1=o1)
    e = epg.E(5.0, T1, T2, order1=o1)
    train = lambda op: [part for j in range(12) for part in (epg.T(35.0, 58.5 * j * (j + 1)), op, epg.S(1), epg.ADC)]
    return train(x), train(e)


def case_khi0_x():
    return dict(seq=khi0_sequences()[0], variables=["T1", "T2"], grid=(2,), nmax=12, kernel="dxrun_kernel<2, 1, 2>")


def case_khi0_e():
    return dict(seq=khi0_sequences()[1], variables=["T1", "T2"], grid=(2,), nmax=12, kernel=None)


CASES.update({"khi0_x": case_khi0_x, "khi0_e": case_khi0_e})
