#!/usr/bin/env python3
"""Generate tests/golden/g22_merge.npz from the reference: float wavenumbers (shift-merge, epgpy/shift.py:367-449), the
gradient operator G and the time accumulation C.

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_merge.py

As make_golden.py: the reference is imported as a black box and driven through its public API; only the resulting data are
written.  The cases are those of tests/merge_cases.py.  Per case: the signal of simulate(); the final states and coords of
the operator-by-operator run; for the cases of merge_cases.PER_SHIFT also states and coords before and after every float
shift (`<case>_s<i>_{states,coords}_{in,out}`, plus `_shift`, `_grid`, `_tol`, `_prune`: the arguments the reference handed
to shiftmerge, wavenumbers in rad/m).

A comparison at rounding level needs inputs that do not sit on a decision boundary.  This script ASSERTS, on the reference's
own numbers, for every float shift of every case:
  * no near-tolerance row: no row of the merged (unpruned) matrix whose all-voxel maximum modulus lies within a factor 10 of
    the pruning tolerance, on either side;
  * no cell-boundary coordinate: no quantised coordinate closer than 1e-3 of a grid cell to a cell boundary;
  * in the cases recorded shift by shift, the reference's input and output are exactly mirror-symmetric (row -j the
    conjugate of row j with the F columns swapped), so that a half representation loses nothing (the reference's rotation of
    a single voxel is not: its rows -j and +j may differ in the last bit);
and over all cases: at least one destination component with more than one source of DISTINCT wavenumbers (a real merge), at
least one shift whose pruning removes rows, and a state matrix beyond 64 stored orders.
"""
import os
import sys

sys.dont_write_bytecode = True
REFERENCE = os.environ.get("EPGPY_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

if not hasattr(np, "asfarray"):      # (NumPy 2 removed it; the reference's spline helper still calls it)
    np.asfarray = lambda a: np.asarray(a, dtype=np.float64)

import epgpy as epg  # noqa: E402  (the reference)
from epgpy import shift as ref_shift  # noqa: E402
import merge_cases  # noqa: E402
import merge_oracle  # noqa: E402

OUT = {}
SEEN = {"multi_source": 0, "pruned": 0, "max_stored": 0, "shifts": 0, "min_margin": 1.0, "rows_max": 0}


def put(name, value):
    OUT[name] = np.asarray(value)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_shift(name, states, wavenums, shift, grid, tol, prune, out_states, out_wavenums):
    """the conditions of the module docstring for one call of the reference's shiftmerge"""
    new, k_new, full, alive = merge_oracle.shiftmerge(states, wavenums, shift, grid=grid, prune=prune, tol=tol, details=True)
    assert same_bits(new, out_states), name
    rowmax = np.max(np.abs(full), axis=tuple(range(full.ndim - 2)) + (full.ndim - 1,))
    near = (rowmax > tol / 10) & (rowmax < tol * 10)
    assert not near.any(), f"{name}: rows near the tolerance: {rowmax[near]}"
    k = np.asarray(wavenums).reshape(-1, np.shape(wavenums)[-1])
    cell = grid * np.ones(k.shape[1])
    kz = np.around(k, 8)
    for arg in (0.5 * (kz - kz[::-1]) / cell, (kz + np.reshape(shift, (1, -1))) / cell):
        margin = np.min(0.5 - np.abs(arg - np.around(arg)))
        SEEN["min_margin"] = min(SEEN["min_margin"], float(margin))
        assert margin > 1e-3, f"{name}: coordinate {margin} of a cell from a boundary"
    if name.split("[")[0] in merge_cases.PER_SHIFT:      # (compared bit for bit through the half representation)
        for arr in (np.asarray(states), np.asarray(out_states)):
            assert same_bits(arr[..., ::-1, [1, 0, 2]].conj() + 0.0, arr + 0.0), f"{name}: not mirror-symmetric"
    # a real merge: one destination component fed by sources of distinct wavenumbers
    kp = kz + np.reshape(shift, (1, -1))
    qp = np.around(kp / cell).astype(int)
    _, inv = merge_oracle.lex_unique(qp)
    for dest in np.flatnonzero(np.bincount(inv) > 1):
        members = kp[inv == dest]
        if np.ptp(members, axis=0).max() > 1e-6 * cell.min():
            SEEN["multi_source"] += 1
    if prune and full.shape[-2] > new.shape[-2]:
        SEEN["pruned"] += 1
    SEEN["max_stored"] = max(SEEN["max_stored"], (new.shape[-2] + 1) // 2)
    SEEN["rows_max"] = max(SEEN["rows_max"], new.shape[-2])
    SEEN["shifts"] += 1


def run_case(name):
    ops, opts = merge_cases.build(epg, name)
    put(name + "_signal", epg.simulate(ops, **opts))
    shape = epg.getshape(ops)
    sm = epg.StateMatrix(shape=shape, **opts)
    index = 0
    for op in epg.functions.flatten_sequence(ops):
        if isinstance(op, epg.operators.Probe):
            continue
        if merge_cases.is_merge_shift(epg, op, sm.coords):
            before = sm
            sm = op(sm)
            # the arguments S._apply hands to shiftmerge (shift.py:120-148), from the public attributes
            kdim = sm.kdim
            ktv = np.asarray(sm.ktvalue)
            coords_in = before.coords
            if coords_in is None or coords_in.shape[-1] < kdim:
                tmp = before.copy()
                tmp.setup_coords(kdim)
                coords_in = tmp.coords
            k_in = (coords_in * ktv).reshape(coords_in.shape[-2:])
            k = op.k if not isinstance(op.k, int) else np.array([[op.k] + [0] * (kdim - 1)])
            d = np.zeros(kdim)
            d[: np.shape(k)[-1]] = np.asarray(k).reshape(-1)
            d = d * ktv
            prune = sm.options.get("prune") or op.prune
            tol = 1e-8 if prune in {True, False} else float(prune)
            grid = sm.options.get("kgrid") or op.kgrid
            k_out = (sm.coords * ktv).reshape(sm.coords.shape[-2:])
            ref_states, ref_k = ref_shift.shiftmerge(before.states, coords_in * ktv, d, grid=grid, prune=bool(prune), tol=tol)
            assert np.array_equal(ref_states, sm.states) and np.array_equal(ref_k.reshape(k_out.shape) / ktv * ktv, k_out)
            check_shift(f"{name}[{index}]", before.states, k_in, d, grid, tol, bool(prune), sm.states, k_out)
            if name in merge_cases.PER_SHIFT and merge_cases.recorded(name, index):
                base = f"{name}_s{index}"
                put(base + "_states_in", before.states)
                put(base + "_coords_in", k_in)
                put(base + "_states_out", sm.states)
                put(base + "_coords_out", k_out)
                put(base + "_shift", d)
                put(base + "_grid", grid)
                put(base + "_tol", tol)
                put(base + "_prune", bool(prune))
            index += 1
        else:
            sm = op(sm)
    put(name + "_nshift", index)
    put(name + "_states", sm.states)
    put(name + "_coords", sm.coords)


def record_attributes():
    for i, (cls, args, kwargs) in enumerate(merge_cases.ATTRIBUTES):
        op = getattr(epg.operators, cls)(*args, **kwargs)
        put(f"attr{i}_k", op.k)
        put(f"attr{i}_shape", op.shape)
        put(f"attr{i}_nshift", op.nshift)
        put(f"attr{i}_kdim", op.kdim)
        put(f"attr{i}_duration", op.duration)
    for cls, args in (("G", (-1.0, [1, 0, 0])), ("G", (1.0, [1, 0, 0, 0])), ("C", (-0.5, 1.0))):
        try:
            getattr(epg.operators, cls)(*args)
        except ValueError:
            continue
        raise AssertionError(f"{cls}{args}: the reference raised no ValueError")


if __name__ == "__main__":
    for case in merge_cases.CASES:
        run_case(case)
        print(case, {k: v for k, v in SEEN.items()}, flush=True)
    record_attributes()
    assert SEEN["multi_source"] > 0, "no destination with sources of distinct wavenumbers"
    assert SEEN["pruned"] > 0, "no shift whose pruning removes rows"
    assert SEEN["max_stored"] > 64, f"no state matrix beyond 64 stored orders ({SEEN['max_stored']})"
    path = os.path.join(HERE, "g22_merge.npz")
    np.savez_compressed(path, **OUT)
    print(f"{path}: {len(OUT)} arrays, {os.path.getsize(path) / 1024:.0f} kB")
