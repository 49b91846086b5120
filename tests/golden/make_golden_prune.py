#!/usr/bin/env python3
"""Generate tests/golden/g23_prune.npz from the reference: float wavenumbers that differ between voxels (shift-prune,
epgpy/shift.py:478-629).

Run ONLY in the build container, where the upstream reference (py-baudin/epgpy) is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prune.py

As make_golden_merge.py: the reference is imported as a black box and driven through its public API; only the resulting data
are written.  The cases are those of tests/prune_cases.py.  Per case: the signal of simulate(); the final states and coords of
the operator-by-operator run; for every call of the reference's `shiftprune` its inputs, arguments and outputs
(`<case>_s<i>_{states,k}_{in,out}`, `_shift` [*grid, kdim], `_grid`, `_nmax` (-1: none), `_prune`, `_tol`; wavenumbers = coords
times ktvalue).

A comparison at rounding level needs inputs that do not sit on a decision boundary.  This script ASSERTS, on the reference's
own numbers, for every shift of every case and every voxel:
  * no quantised coordinate within 1e-3 of a cell from a cell boundary;
  * no row norm within a factor 10 of the pruning tolerance;
  * no two rows around a trim cut whose energies lie within a factor 1 + 1e-6 of each other;
  * no two distinct cells with one flat key (shift.py:603-607);
  * every shift that follows a per-voxel one is itself per voxel (all of them go through `shiftprune`);
  * inputs and outputs are exactly mirror-symmetric;
  * no cell has more than 8 sources (the M of the GPU tests' accumulated bound);
  * the host oracle (tests/prune_oracle.py) gives the reference's rows: states bit for bit, per voxel and per cell, once the
    all-zero rows are left out (the reference pads with them, and keeps them in place where one voxel has nothing to prune);
and over all cases: a cell where distinct wavenumbers merge, a voxel with zero shift next to moving ones, voxels with
different live counts after one shift, a shift whose prune removes rows in some voxels only, an active trim, a negative shift,
kdim 1, 3 and 4, and signals that differ between voxels.
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
import prune_cases  # noqa: E402
import prune_oracle  # noqa: E402

OUT = {}
SEEN = {"distinct_merge": 0, "zero_shift": 0, "live_differ": 0, "prune_some": 0, "trim": 0, "negative": 0, "kdim": set(),
        "min_margin": 1.0, "max_stored": 0, "shifts": 0}
CALLS = []
_shiftprune = ref_shift.shiftprune


def recording_shiftprune(states, wavenums, shift, *, grid=1e-5, nmax=None, prune=True, tol=1e-8):
    out = _shiftprune(states, wavenums, shift, grid=grid, nmax=nmax, prune=prune, tol=tol)
    CALLS.append(dict(states=np.array(states), k=np.array(wavenums), shift=np.array(shift), grid=grid, nmax=nmax, prune=prune,
                      tol=tol, states_out=np.array(out[0]), k_out=np.array(out[1])))
    return out


ref_shift.shiftprune = recording_shiftprune


def put(name, value):
    OUT[name] = np.asarray(value)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_call(name, call):
    """the conditions of the module docstring for one call of the reference's shiftprune"""
    states, k = call["states"], call["k"]
    kdim = k.shape[-1]
    vgrid = call["states_out"].shape[:-2]
    nvox = int(np.prod(vgrid))
    grid = call["grid"] * np.ones(kdim)
    shift = np.broadcast_to(call["shift"], vgrid + (kdim,)).reshape(nvox, kdim)
    st_in = np.broadcast_to(states, vgrid + states.shape[-2:]).reshape((nvox,) + states.shape[-2:])
    k_in = np.broadcast_to(k, vgrid + k.shape[-2:]).reshape((nvox,) + k.shape[-2:])
    st_out = call["states_out"].reshape((nvox,) + call["states_out"].shape[-2:])
    k_out = call["k_out"].reshape((nvox,) + call["k_out"].shape[-2:])
    for arr in (st_in, st_out):
        assert same_bits(arr[..., ::-1, [1, 0, 2]].conj() + 0.0, arr + 0.0), f"{name}: not mirror-symmetric"
    # flat keys of the reference (shift.py:603-607) over the candidates of all voxels
    q = np.concatenate([prune_oracle.rnd(0.5 * (k_in - k_in[:, ::-1]) / grid), prune_oracle.rnd((k_in + shift[:, None]) / grid),
                        -prune_oracle.rnd((k_in + shift[:, None]) / grid)[:, ::-1]], axis=1).astype(int)
    mult = np.cumsum(np.r_[1, q.max(axis=(0, 1))[::-1]])[-2::-1]
    for v in range(nvox):
        assert len(np.unique(q[v] @ mult)) == len(np.unique(q[v], axis=0)), f"{name} voxel {v}: flat-key collision"
    live, pruned = [], []
    for v in range(nvox):
        st, co = prune_oracle.live_rows(st_in[v], k_in[v])
        details = {}
        rows = prune_oracle.shift_voxel(st, co, shift[v], grid, call["nmax"], call["prune"], call["tol"], details)
        margin = min(details["margin"])
        SEEN["min_margin"] = min(SEEN["min_margin"], float(margin))
        assert margin > 1e-3, f"{name} voxel {v}: coordinate {margin} of a cell from a boundary"
        norms = np.array([x for x in details["norms"] if x > 0])
        near = (norms > call["tol"] / 10) & (norms < call["tol"] * 10)
        assert not near.any(), f"{name} voxel {v}: row norms near the tolerance: {norms[near]}"
        for below, above in details.get("trim_cut", []):
            assert above > below * (1 + 1e-6), f"{name} voxel {v}: a tie at the trim cut ({below}, {above})"
        # the reference's rows of this voxel, by cell, without the all-zero rows
        used = np.any(st_out[v] != 0, axis=-1) | np.any(k_out[v] != 0, axis=-1)
        used[(len(used) - 1) // 2] = True
        cells = [tuple(int(c) for c in prune_oracle.rnd(kk / grid)) for kk in k_out[v][used]]
        assert len(set(cells)) == len(cells), f"{name} voxel {v}: two rows of the reference in one cell"
        mine = {c: r for c, r in rows.items() if c == (0,) * kdim or any(x != 0 for x in r[:3]) or np.any(r[3] != 0)}
        assert set(cells) == set(mine), f"{name} voxel {v}: cells {sorted(set(cells) ^ set(mine))} differ"
        for c, s_ref, k_ref in zip(cells, st_out[v][used], k_out[v][used]):
            assert same_bits(np.array(mine[c][:3]) + 0.0, s_ref + 0.0), f"{name} voxel {v} cell {c}: states differ {mine[c][:3]} {s_ref}"
            m = details["sources"][c]
            bound = 4 * (m + 4) * 2.0 ** -53 * (np.abs(co).max() + np.abs(shift[v]).max())
            assert np.abs(mine[c][3] - k_ref).max() <= bound, f"{name} voxel {v} cell {c}: coordinates differ"
        assert max(details["sources"].values()) <= 8, f"{name} voxel {v}: a cell of {max(details['sources'].values())} sources"
        live.append((len(mine) + 1) // 2)
        pruned.append(details["pruned"][0])
        SEEN["trim"] += bool(details["trimmed"][0])
        # a real merge: F candidates of distinct wavenumbers (and non-zero weight) in one cell
        k1 = co + shift[v]
        q1 = prune_oracle.rnd(k1 / grid)
        for c in np.unique(q1, axis=0):
            members = k1[np.all(q1 == c, axis=1) & (np.abs(st[:, 0]) > call["tol"])]
            if len(members) > 1 and np.ptp(members, axis=0).max() > 1e-6 * grid.min():
                SEEN["distinct_merge"] += 1
    moving = np.any(shift != 0, axis=1)
    SEEN["zero_shift"] += bool(moving.any() and not moving.all())
    SEEN["live_differ"] += len(set(live)) > 1
    SEEN["prune_some"] += bool(call["prune"] and max(pruned) > 0 and min(pruned) == 0)
    SEEN["negative"] += bool(np.any(shift < 0))
    SEEN["kdim"].add(kdim)
    SEEN["max_stored"] = max(SEEN["max_stored"], max(live))
    SEEN["shifts"] += 1


def run_case(name):
    ops, opts = prune_cases.build(epg, name)
    del CALLS[:]
    signal = np.asarray(epg.simulate(ops, **opts))
    ncall = len(CALLS)
    nshift = sum(isinstance(op, epg.operators.S) for op in epg.functions.flatten_sequence(ops))
    assert ncall == nshift, f"{name}: {ncall} of {nshift} shifts are per voxel"
    flat = signal.reshape(signal.shape[0], -1)
    assert np.abs(flat[-1]).max() > 1e-3 and np.ptp(np.abs(flat[-1])) > 1e-3 * np.abs(flat[-1]).max(), f"{name}: one signal for all voxels"
    put(name + "_signal", signal)
    del CALLS[:]
    sm = epg.StateMatrix(shape=epg.getshape(ops), **opts)
    for op in epg.functions.flatten_sequence(ops):
        if not isinstance(op, epg.operators.Probe):
            sm = op(sm)
    assert len(CALLS) == nshift
    for i, call in enumerate(CALLS):
        check_call(f"{name}[{i}]", call)
        base = f"{name}_s{i}"
        vgrid = call["states_out"].shape[:-2]
        put(base + "_states_in", call["states"])
        put(base + "_k_in", call["k"])
        put(base + "_shift", np.broadcast_to(call["shift"], vgrid + call["k"].shape[-1:]))
        put(base + "_grid", call["grid"])
        put(base + "_nmax", -1 if call["nmax"] is None else call["nmax"])
        put(base + "_prune", bool(call["prune"]))
        put(base + "_tol", call["tol"])
        put(base + "_states_out", call["states_out"])
        put(base + "_k_out", call["k_out"])
    put(name + "_nshift", nshift)
    put(name + "_states", sm.states)
    put(name + "_coords", sm.coords)
    put(name + "_ktvalue", np.asarray(sm.ktvalue, dtype=np.float64) * np.ones(sm.kdim))


if __name__ == "__main__":
    for case in prune_cases.CASES:
        run_case(case)
        print(case, SEEN, flush=True)
    for key in ("distinct_merge", "zero_shift", "live_differ", "prune_some", "trim", "negative"):
        assert SEEN[key] > 0, f"no coverage of: {key}"
    assert {1, 3, 4} <= SEEN["kdim"], SEEN["kdim"]
    assert SEEN["max_stored"] <= 64, SEEN["max_stored"]
    path = os.path.join(HERE, "g23_prune.npz")
    np.savez_compressed(path, **OUT)
    print(f"{path}: {len(OUT)} arrays, {os.path.getsize(path) / 1024:.0f} kB")
