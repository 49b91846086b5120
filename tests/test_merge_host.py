"""Host side of the float-wavenumber shift (shift-merge): the NumPy restatement against the reference's recorded results, the
planner's gather table and its state-dependent half against the same, the public interface of G / C, and the C ABI."""
import os
import re

import numpy as np
import pytest

from epgpy_amd import epg, kmerge, _lib

from tests import merge_cases
from tests import merge_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.uint64)


def shifts(g):
    """every recorded float shift: (label, states_in, coords_in, shift, grid, tol, prune, states_out, coords_out)"""
    for name in merge_cases.PER_SHIFT:
        for i in range(int(g[name + "_nshift"])):
            base = f"{name}_s{i}"
            if base + "_shift" in g:
                yield (base, g[base + "_states_in"], g[base + "_coords_in"], g[base + "_shift"], g[base + "_grid"][()],
                       float(g[base + "_tol"]), bool(g[base + "_prune"]), g[base + "_states_out"], g[base + "_coords_out"])


def close_coords(got, want):
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1e-300) + 1e-300), np.abs(got - want).max()


def test_oracle_equals_every_golden_pair(golden):
    g = golden("g22_merge")
    count = 0
    for base, sin, kin, d, grid, tol, prune, sout, kout in shifts(g):
        new, k_new = merge_oracle.shiftmerge(sin, kin, d, grid=grid, prune=prune, tol=tol)
        assert new.shape == sout.shape and np.array_equal(bits(new), bits(sout)), base
        close_coords(k_new, kout)
        count += 1
    assert count > 40


def test_planner_table_reproduces_the_golden_output_bit_for_bit(golden):
    """the CSR table of epgx_state_merge, applied in NumPy to the half representation of the golden input: every row the
    reference keeps has the reference's bits, and the whole matrix those of the unpruned restatement"""
    g = golden("g22_merge")
    multi = 0
    for base, sin, kin, d, grid, tol, prune, sout, kout in shifts(g):
        plan = kmerge.MergePlan(kin, d, grid)
        n_in = (sin.shape[-2] - 1) // 2
        half = merge_oracle.fold(sin, 64 * (n_in // 64 + 1))
        Kd = 64 * ((plan.nhalf - 1) // 64 + 1)
        out = merge_oracle.apply_table(half, plan.offsets, plan.sources, Kd)
        assert not np.any(out[:, :, plan.nhalf:])
        full = merge_oracle.unfold(out, sin.shape[:-2], plan.nhalf - 1)
        _, _, ref_full, alive = merge_oracle.shiftmerge(sin, kin, d, grid=grid, prune=prune, tol=tol, details=True)
        assert np.array_equal(bits(full + 0.0), bits(ref_full + 0.0)), base
        assert np.array_equal(bits(full[..., alive, :] + 0.0), bits(sout + 0.0)), base
        multi += int(np.any(np.diff(plan.offsets, axis=1) > 1))
        assert plan.offsets[0, 0] == 0 and plan.offsets[-1, -1] == len(plan.sources)
    assert multi > 0          # (some destination component has more than one source)


def test_finish_gives_the_golden_coordinates_and_row_set(golden):
    g = golden("g22_merge")
    pruned = 0
    for base, sin, kin, d, grid, tol, prune, sout, kout in shifts(g):
        plan = kmerge.MergePlan(kin, d, grid)
        n_in = (sin.shape[-2] - 1) // 2
        half = merge_oracle.fold(sin, n_in + 1)
        sums, _ = merge_oracle.row_stats(half, n_in + 1)
        out = merge_oracle.apply_table(half, plan.offsets, plan.sources, plan.nhalf)
        _, maxabs = merge_oracle.row_stats(out, plan.nhalf)
        k_new, keep = plan.finish(sums, maxabs, tol, prune)
        close_coords(k_new, kout)
        _, _, _, alive = merge_oracle.shiftmerge(sin, kin, d, grid=grid, prune=prune, tol=tol, details=True)
        cn = (len(alive) - 1) // 2
        assert np.array_equal(keep, np.flatnonzero(alive[cn:])), base
        assert 2 * len(keep) - 1 == sout.shape[-2]
        pruned += int(len(keep) < plan.nhalf)
    assert pruned > 0


def test_row_stats_restatement_is_the_modulus():
    rng = np.random.default_rng(0)
    half = rng.normal(size=(7, 3, 64)) + 1j * rng.normal(size=(7, 3, 64))
    sums, maxabs = merge_oracle.row_stats(half, 40)
    assert np.allclose(sums, np.abs(half[:, :, :40]).sum(axis=0), rtol=1e-14)
    assert np.allclose(maxabs, np.abs(half[:, :, :40]).max(axis=(0, 1)), rtol=4e-16)


def test_g_and_c_attributes_match_the_reference(golden):
    g = golden("g22_merge")
    for i, (cls, args, kwargs) in enumerate(merge_cases.ATTRIBUTES):
        op = getattr(epg, cls)(*args, **kwargs)
        assert isinstance(op, epg.S)
        assert np.array_equal(op.k, g[f"attr{i}_k"]) and op.k.dtype == g[f"attr{i}_k"].dtype
        assert tuple(op.shape) == tuple(g[f"attr{i}_shape"])
        assert op.nshift == g[f"attr{i}_nshift"] and op.kdim == g[f"attr{i}_kdim"]
        assert np.array_equal(np.asarray(op.duration), g[f"attr{i}_duration"])
    with pytest.raises(ValueError, match="negative time"):
        epg.G(-1.0, [1, 0, 0])
    with pytest.raises(ValueError, match="3d gradients"):
        epg.G(1.0, [1, 0, 0, 0])
    with pytest.raises(ValueError, match="negative time"):
        epg.C(-0.5, 1.0)
    from epgpy_amd import operators
    assert operators.G is epg.G and operators.C is epg.C


def test_float_shift_errors_without_a_device():
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.compile_sequence([epg.S(1.5), epg.ADC])
    with pytest.raises(AttributeError, match="kgrid not set"):
        epg.compile_sequence([epg.G(1.0, [1, 0, 0]), epg.ADC])
    for op in (epg.S([[1.5, 0.2], [0.5, 0.1]], kgrid=0.1), epg.C(1.0, [0.1, 0.2], kgrid=0.1)):
        with pytest.raises(NotImplementedError, match="shift-prune"):       # a float k that varies along a grid axis
            epg.compile_sequence([op, epg.ADC])
    with pytest.raises(NotImplementedError, match="operator by operator"):   # a float shift cannot be compiled into a plan
        epg.compile_sequence([epg.S(1.5, kgrid=1), epg.ADC])


def test_float_kspace_keeps_the_checks():
    ks = kmerge.FloatKSpace.from_coords(np.array([[[-1.5, 0.2], [0, 0], [1.5, -0.2]]]))
    assert ks.nrow == 3 and ks.kdim == 2 and ks.coords.dtype == np.float64 and ks.with_kdim(4).kdim == 4
    with pytest.raises(ValueError, match="symmetric"):
        kmerge.FloatKSpace.from_coords(np.array([[1.5], [0.0], [1.5]]))
    with pytest.raises(ValueError, match="sorted"):
        kmerge.FloatKSpace.from_coords(np.array([[1.5], [0.0], [-1.5]]), kgrid=1.0)
    with pytest.raises(RuntimeError):
        ks.with_kdim(1)
    b_l, b_t, b_m = ks.with_kdim(4).bmatrices(2.0)
    assert b_l.shape == (2, 3, 3)            # the time coordinate does not diffuse
    assert np.array_equal(kmerge.ktvalue(2.0, 3.0, 4), [2, 2, 2, 3]) and np.array_equal(kmerge.ktvalue([1, 2, 3], 5.0, 2), [1, 2])


def test_new_entry_points_in_header_and_binding():
    header = open(os.path.join(ROOT, "include", "epgx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in (("epgx_state_row_stats", 5), ("epgx_state_merge", 6)):
        proto = re.search(rf"^int\s+{name}\(([^;]*?)\);", text, re.M | re.S)
        assert proto and len(proto.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1])
        assert hasattr(_lib.load(), name)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "epgx_state_row_stats" in doc and "epgx_state_merge" in doc
    assert _lib.MERGE_MAX_ROWS == 1024 and _lib.MERGE_COMP_SHIFT == merge_oracle.COMP_SHIFT and _lib.GS_CONJ == merge_oracle.GS_CONJ
