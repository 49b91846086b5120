"""GPU: the reference's recorded per-voxel float shifts (tests/golden/g23_prune.npz) through simulate(..., voxel_coords=True)
and through op(sm), shift by shift; and the errors of the option that need a state matrix.

Bounds.  One shift changes a component by at most 4 (m + 4) 2^-53 sum|sources| (m sources per destination, here m <= M = 8:
the generator records at most a handful per cell); a row-local operator (T, E) by a few 2^-53 of the row.  After j operators
the bound is  j * 4 (M + 4) 2^-53 * A  (make_golden_prune.py asserts m <= M on the reference's numbers),  A the largest sum over the rows of one voxel of |F| + |col1| + |Z| in the reference's
recorded states: a bound from the number formats and the reference's own numbers, not from what the device gives."""
import os

import numpy as np
import pytest

from epgpy_amd import epg
from tests import prune_cases, prune_oracle

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "g23_prune.npz"))
EPS, M = 2.0 ** -53, 8


def amplitude(case):
    return max(np.abs(GOLD[f"{case}_s{i}_states_out"]).sum(axis=(-2, -1)).max() for i in range(int(GOLD[case + "_nshift"])))


@pytest.mark.parametrize("case", prune_cases.CASES)
def test_simulate_against_the_reference(case):
    ops, opts = prune_cases.build(epg, case)
    want = GOLD[case + "_signal"]
    got = np.asarray(epg.simulate(ops, voxel_coords=True, **opts))
    assert got.shape == want.shape
    A = amplitude(case)
    nop = 0
    for r, op in enumerate(o for o in ops if o is epg.ADC):
        nop = [i for i, o in enumerate(ops) if o is epg.ADC][r]
        err, bound = np.abs(got[r] - want[r]).max(), (nop + 1) * 4 * (M + 4) * EPS * A
        print(f"{case} record {r}: err {err:.2e} bound {bound:.2e}")
        assert err <= bound, (case, r, err, bound)


@pytest.mark.parametrize("case", prune_cases.CASES)
def test_operator_by_operator_against_the_reference(case):
    ops, opts = prune_cases.build(epg, case)
    shape = GOLD[case + "_signal"].shape[1:]
    sm = epg.StateMatrix(shape=shape, voxel_coords=True, **opts)
    A, ktv = amplitude(case), GOLD[case + "_ktvalue"]
    i = 0
    for j, op in enumerate(ops):
        if op is epg.ADC:
            continue
        sm = op(sm, inplace=True)
        if not isinstance(op, epg.S):
            continue
        st_ref, k_ref = GOLD[f"{case}_s{i}_states_out"], GOLD[f"{case}_s{i}_k_out"]
        grid = float(GOLD[f"{case}_s{i}_grid"])
        states, k = sm.states, sm.coords * ktv[: sm.kdim]
        assert states.shape[:-2] == st_ref.shape[:-2] == tuple(shape)
        bound = (j + 1) * 4 * (M + 4) * EPS * A
        kbound = (j + 1) * 4 * (M + 4) * EPS * max(np.abs(k_ref).max(), grid)
        nvox = int(np.prod(shape))
        for v in range(nvox):
            idx = np.unravel_index(v, shape)
            mine = prune_oracle.rows_by_cell(states[idx], k[idx], grid)
            ref = prune_oracle.rows_by_cell(st_ref[idx], k_ref[idx], grid)
            assert set(mine) == set(ref), (case, i, v, sorted(set(mine) ^ set(ref)))
            for cell in ref:
                assert np.abs(mine[cell][0] - ref[cell][0]).max() <= bound, (case, i, v, cell)
                assert np.abs(mine[cell][1] - ref[cell][1]).max() <= kbound, (case, i, v, cell)
        i += 1
    assert i == int(GOLD[case + "_nshift"])
    assert sm.options["voxel_coords"] is True and sm.copy().options["voxel_coords"] is True


def test_errors_on_a_state_matrix_with_per_voxel_coordinates():
    sm = epg.StateMatrix(shape=(3, 1), kgrid=0.25, voxel_coords=True)
    sm = epg.T(30, 90)(sm, inplace=True)
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.S([[[1.5]], [[0.5]], [[0.7]]])(epg.StateMatrix(shape=(3, 1), voxel_coords=True))
    sm = epg.S([[[1.5]], [[0.5]], [[0.7]]])(sm, inplace=True)
    before, kbefore = sm.states.copy(), sm.coords.copy()
    with pytest.raises(NotImplementedError, match="D \\(diffusion\\)"):
        epg.D(1.0, 1e-3)(sm)
    with pytest.raises(NotImplementedError, match="per-voxel coordinates"):
        epg.DFT([[0.0, 0.0, 0.0]])._acquire(sm)
    # a scalar float shift and an int shift are broadcast onto the per-voxel coordinates
    assert epg.S(0.5)(sm).coords.shape[:2] == (3, 1) and epg.S(1)(sm).coords.shape[:2] == (3, 1)
    # an operator that widens the grid, then a shift: a named error, the state as it was
    wide = epg.E(2.0, 1000.0, np.array([[40.0, 80.0]]))(sm)
    with pytest.raises(NotImplementedError, match="widening the grid"):
        epg.S(0.5)(wide)
    assert np.array_equal(sm.states, before) and np.array_equal(sm.coords, kbefore)


def test_a_general_equilibrium_with_the_option():
    init = epg.StateMatrix([[0, 0, 1.0]], equilibrium=[[0.1j, -0.1j, 0.5]], shape=(2,), kgrid=1.0, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="general equilibrium"):
        epg.simulate([epg.T(30, 90), epg.S([[1.5], [0.5]]), epg.ADC], init=init, kgrid=1.0, voxel_coords=True)
    with pytest.raises(NotImplementedError, match="general equilibrium"):
        epg.S([[1.5], [0.5]])(init)
