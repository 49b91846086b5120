"""The host oracle (tests/prune_oracle.py) against the reference's recorded calls of `shiftprune`
(tests/golden/g23_prune.npz, from make_golden_prune.py): every case, every shift, every voxel and every cell.  States bit for
bit (the sign of a zero aside: the reference's add.at starts from +0, its conjugate of a zero is -0), coordinates within
4 (m + 4) 2^-53 max|k_source| for a cell of m sources."""
import os

import numpy as np
import pytest

from tests import prune_cases, prune_oracle

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "g23_prune.npz"))
EPS = 2.0 ** -53


def bits(a):
    return (np.ascontiguousarray(a, dtype=np.complex128) + 0.0).view(np.uint64)


def shifts_of(case):
    for i in range(int(GOLD[case + "_nshift"])):
        g = lambda key: GOLD[f"{case}_s{i}_{key}"]
        yield i, {key: g(key) for key in ("states_in", "k_in", "shift", "grid", "nmax", "prune", "tol", "states_out", "k_out")}


@pytest.mark.parametrize("case", prune_cases.CASES)
def test_oracle_matches_the_reference_per_voxel_and_per_cell(case):
    ncell = 0
    for i, c in shifts_of(case):
        vgrid, kdim = c["states_out"].shape[:-2], c["k_in"].shape[-1]
        nvox = int(np.prod(vgrid))
        st_in = np.broadcast_to(c["states_in"], vgrid + c["states_in"].shape[-2:]).reshape((nvox,) + c["states_in"].shape[-2:])
        k_in = np.broadcast_to(c["k_in"], vgrid + c["k_in"].shape[-2:]).reshape((nvox,) + c["k_in"].shape[-2:])
        shift = c["shift"].reshape(nvox, kdim)
        st_out, k_out = c["states_out"].reshape((nvox,) + c["states_out"].shape[-2:]), c["k_out"].reshape((nvox,) + c["k_out"].shape[-2:])
        nmax = None if int(c["nmax"]) < 0 else int(c["nmax"])
        for v in range(nvox):
            st, co = prune_oracle.live_rows(st_in[v], k_in[v])
            details = {}
            rows = prune_oracle.shift_voxel(st, co, shift[v], float(c["grid"]), nmax, bool(c["prune"]), float(c["tol"]), details)
            mine = {cell: r for cell, r in rows.items() if cell == (0,) * kdim or any(x != 0 for x in r[:3]) or np.any(r[3] != 0)}
            ref = prune_oracle.rows_by_cell(st_out[v], k_out[v], float(c["grid"]))
            assert set(mine) == set(ref), (case, i, v)
            kmax = np.abs(co).max() + np.abs(shift[v]).max()
            for cell, (s_ref, k_ref) in ref.items():
                assert np.array_equal(bits(np.array(mine[cell][:3])), bits(s_ref)), (case, i, v, cell)
                assert np.abs(mine[cell][3] - k_ref).max() <= 4 * (details["sources"][cell] + 4) * EPS * kmax, (case, i, v, cell)
                ncell += 1
    assert ncell > 50


def test_golden_covers_what_the_cases_are_for():
    kdims = {GOLD[f"{case}_s0_k_in"].shape[-1] for case in prune_cases.CASES}
    assert {1, 3, 4} <= kdims
    assert any(int(GOLD[f"{case}_s0_nmax"]) > 0 for case in prune_cases.CASES)
    for case in prune_cases.CASES:
        last = np.abs(GOLD[case + "_signal"][-1]).reshape(-1)
        assert np.ptp(last) > 1e-3 * last.max()           # (a broadcast result cannot pass)
