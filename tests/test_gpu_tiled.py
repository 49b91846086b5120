"""GPU: the tiled path for state matrices of any length (csrc/epgx_tiled.hip, include/epgx.h epgx_run_tiled).

(a) at 512 / 1024 orders the tiled entry computes what the per-timestep kernel computes, bit for bit (both walk the same
    fused records with the same per-order arithmetic; a shift by n >= 2 becomes n shifts by one -- the same moves);
(b) beyond 2048 orders it agrees with the C oracle, which has no size limit;
(c) from a start state; (d) in voxel slabs; (e) in every output form; (f) the kernels it launches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import epgpy_amd as epg
from epgpy_amd import _lib, functions
from oracle import epg_c
from tests import sequences as sq

pytestmark = pytest.mark.gpu
TOL = 1e-11


def close(a, b, tol=TOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    assert err <= tol * max(1.0, float(np.max(np.abs(b))) if b.size else 1.0), err


def device_plan(ops, **options):
    enc, _, _ = functions.compile_sequence(ops, options=options)
    ctx = _lib.get_context()
    return ctx, enc, enc.device_plan(ctx)


def run_tiled(ctx, enc, plan, Kbuf, state_in=None, slab_voxels=0):
    nvox = enc.nvox
    sig = _lib.DeviceBuffer(ctx, 16 * max(enc.n_adc, 1) * nvox)
    _lib.run_tiled(ctx, plan, 0, nvox, state_in, Kbuf, sig.ptr.value, nvox, 0, slab_voxels)
    out = sig.download(np.complex128, (enc.n_adc, nvox))
    sig.free()
    return out


def run_per_timestep(ctx, enc, plan, K):
    nvox = enc.nvox
    sig = _lib.DeviceBuffer(ctx, 16 * max(enc.n_adc, 1) * nvox)
    st = _lib.DeviceState(ctx, nvox, K)
    assert _lib.kernel_for(ctx, plan, K, state_in=st, state_out=st).startswith("run_kernel<")
    _lib.run(ctx, plan, 0, plan.n_ops, 0, nvox, st, st, K, sig.ptr.value, nvox, 0)
    out = sig.download(np.complex128, (enc.n_adc, nvox))
    sig.free()
    return out


def long_random(rng, grid, nops):
    """sequences.random_sequence with the shifts biased upwards and RESET (which empties the state matrix) only in the last
    tenth of the train: the populated orders reach several hundred first"""
    tuples = sq.random_sequence(rng, grid, nops=nops)
    late = 9 * len(tuples) // 10
    tuples = [t for i, t in enumerate(tuples) if t[0] != "RESET" or i >= late]
    return [t if t[0] != "S" else ("S", abs(t[1]) if rng.random() < 0.85 else t[1]) for t in tuples]


# ------------------------------------------------------------------ (a) same arithmetic as the per-timestep kernel
@pytest.mark.parametrize("seed", range(6))
def test_same_bits_as_run_kernel(seed):
    rng = np.random.default_rng(1000 + seed)
    grid = (3, 5) if seed % 2 else (7,)
    tuples = long_random(rng, grid, nops=int(rng.integers(1300, 1700)))
    if seed == 5:     # truncation below the capacity
        tuples = [t if t[0] != "S" else ("S", t[1], 600) for t in tuples]
    ops = sq.to_ops(epg, tuples)
    ctx, enc, plan = device_plan(ops)
    K = enc.capacity()
    assert K in (512, 1024), (K, enc.peak)
    assert enc.peak >= 448, enc.peak     # at least two tiles of 448 orders
    ref = run_per_timestep(ctx, enc, plan, K)
    got = run_tiled(ctx, enc, plan, K)
    assert np.array_equal(got, ref), float(np.max(np.abs(got - ref)))


# ------------------------------------------------------------------ (b) beyond 2048 orders, against the C oracle
def hyper_echo(npulse):
    """the reference's hyper-echo test (test/test_core.py:9-32) with `npulse` pulses per half: F0 = 1, Z0 = 0 at the end"""
    echo1 = [("S", 1), ("T", 10.0, 0.0), ("S", 1), ("ADC",)]
    echo2 = [("S", 1), ("T", -10.0, 0.0), ("S", 1), ("ADC",)]
    return [("T", 90.0, 90.0)] + echo1 * npulse + [("S", 1), ("T", 180.0, 0.0), ("S", 1)] + echo2 * npulse


def test_hyper_echo_beyond_2048_orders():
    tuples = hyper_echo(1201)          # 4806 shifts: orders up to 4806
    ops = sq.to_ops(epg, tuples)
    got = epg.simulate(ops)
    close(got, epg_c.simulate(tuples))
    assert abs(got[-1, 0] - 1.0) < 1e-9 and not np.allclose(got[:-1], 1.0)


def mrf_tuples_long(ntr, T1, T2, rng):
    flips = 10 + 60 * np.abs(np.sin(np.arange(ntr) * np.pi / 500)) + rng.uniform(0, 5, ntr)
    tuples = [("T", 180.0, 0.0), ("E", 20.0, T1, T2, 0.0), ("SPOILER",)]
    for i, fa in enumerate(flips):
        tuples += [("T", float(fa), 90.0 if i % 2 else 0.0), ("E", 2.0, T1, T2, 0.0), ("ADC",), ("E", 8.0, T1, T2, 0.0), ("S", 1)]
    return tuples


def test_unbounded_mrf_3000_tr():
    rng = np.random.default_rng(3)
    T1 = np.array([400.0, 900.0, 1600.0])[:, None]
    T2 = np.array([40.0, 120.0])[None, :]
    tuples = mrf_tuples_long(3000, T1, T2, rng)
    ops = sq.to_ops(epg, tuples)
    got = epg.simulate(ops)
    assert got.shape == (3000, 3, 2)
    close(got, epg_c.simulate(tuples))


def test_mse_1100_echoes():
    T2 = np.array([30.0, 60.0, 100.0, 250.0, 800.0])
    tuples = [("T", 90.0, 90.0)]
    for _ in range(1100):
        tuples += [("E", 2.5, 1000.0, T2, 0.0), ("S", 1), ("T", 150.0, 0.0), ("S", 1), ("E", 2.5, 1000.0, T2, 0.0), ("ADC",)]
    ops = sq.to_ops(epg, tuples)
    got = epg.simulate(ops)
    close(got, epg_c.simulate(tuples))


def test_big_and_negative_shifts_truncation_ragged():
    rng = np.random.default_rng(11)
    T2 = rng.uniform(30, 300, 7)     # seven voxels: not a multiple of the four per workgroup
    tuples = [("T", 90.0, 90.0)]
    for i in range(1500):
        tuples += [("S", 2 if i % 3 else -1), ("T", float(rng.uniform(20, 170)), float(rng.uniform(-90, 90))),
                   ("E", 3.0, 900.0, T2, 0.01), ("ADC",)]
        if i == 400:
            tuples += [("S", 300), ("ADC", "Z0"), ("S", -40), ("ADC",)]
    ops = sq.to_ops(epg, tuples)
    close(epg.simulate(ops), epg_c.simulate(tuples))
    close(epg.simulate(ops, max_nstate=2500), epg_c.simulate(tuples, max_nstate=2500))
    capped = [t if t[0] != "S" else ("S", t[1], 2100) for t in tuples]
    capped_ops = sq.to_ops(epg, capped)
    enc = functions.compile_sequence(capped_ops)[0]
    with pytest.raises(NotImplementedError):      # (above the capacity classes: the tiled path)
        enc.capacity(resident=True)
    assert enc.tiled_capacity() == 2112
    close(epg.simulate(capped_ops), epg_c.simulate(capped))


# ------------------------------------------------------------------ (c) from a start state
def test_init_state_grows_past_1024_orders():
    T2 = np.array([50.0, 90.0, 400.0])
    head = [("T", 90.0, 90.0)] + [("S", 1), ("T", 130.0, 0.0), ("E", 4.0, 1000.0, T2, 0.0)] * 300
    train = []
    for _ in range(1150):
        train += [("S", 1), ("T", 150.0, 30.0), ("S", 1), ("E", 4.0, 1000.0, T2, 0.0), ("ADC",)]
    sm = epg.StateMatrix(shape=(3,))
    for op in epg.flatten_sequence(sq.to_ops(epg, head)):
        sm = op(sm, inplace=True)
    assert sm.nstate == 300
    got = epg.simulate(sq.to_ops(epg, train), init=sm)
    assert sm.nstate == 300      # the caller's start state is left as it was
    close(got, epg_c.simulate(head + train))


# ------------------------------------------------------------------ (d) voxel slabs
_SLAB_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
import epgpy_amd as epg
T2 = np.linspace(30, 300, 30)
ops = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.S(1), epg.E(3, 900, T2), epg.ADC] * 1100
np.save({out!r}, epg.simulate(ops))
"""


def test_slabs_give_the_same_bits(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for name, env in (("one", {}), ("slabs", {"EPGX_SLAB_VOXELS": "8"})):
        out = str(tmp_path / f"{name}.npy")
        code = _SLAB_CHILD.format(root=root, out=out)
        subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env={**os.environ, **env})
        res[name] = np.load(out)
    assert res["one"].shape == (1100, 30)
    assert np.array_equal(res["one"], res["slabs"])


# ------------------------------------------------------------------ (e) output forms
def test_output_forms():
    T2 = np.linspace(30, 300, 12).reshape(3, 4)
    ops = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.S(1), epg.E(3, 900, T2), epg.ADC] * 1100
    ref = epg.simulate(ops)
    c64 = epg.simulate(ops, dtype=np.complex64)
    assert c64.dtype == np.complex64 and np.array_equal(c64, ref.astype(np.complex64))
    dev = epg.simulate(ops, out="device")
    assert np.array_equal(np.asarray(dev), ref)
    w = [[1.0, 2.0, 3.0, 4.0]]
    red = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.S(1), epg.E(3, 900, T2), epg.Adc(reduce=1, weights=w)] * 1100
    close(epg.simulate(red), np.sum(ref * np.asarray(w), axis=-1), 1e-12)


# ------------------------------------------------------------------ (f) kernel names
def test_kernel_names():
    ctx, enc, plan = device_plan([epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.ADC] * 3000)
    info = _lib.tiled_info(ctx, plan, enc.tiled_capacity())
    assert info["names"] == "tiled_kernel<8, 32>"
    assert info["blocks"] == -(-3000 // 32) and info["shifts"] == 0 and info["peak"] == 3000
    ctx, enc, plan = device_plan([epg.T(90, 90), epg.S(300), epg.ADC] + [epg.S(1), epg.ADC] * 2000)
    info = _lib.tiled_info(ctx, plan, enc.tiled_capacity())
    assert info["names"] == "tiled_kernel<8, 32> + tiled_shift" and info["shifts"] == 1 and info["peak"] == 2300
    with pytest.raises(_lib.EpgxError):
        _lib.tiled_info(ctx, plan, 2240)      # too short for the plan
    with pytest.raises(_lib.EpgxError):
        _lib.tiled_info(ctx, plan, 2350)      # not a multiple of 64


def schedule_model(enc, Kbuf):
    """what the operator-level model (Encoder.tiled_blocks) predicts for the library's schedule"""
    blocks = enc.tiled_blocks()
    big = sum(1 for b0, b1, _ in blocks if b1 - b0 == 1 and enc.records[b0][0] == _lib.OP_S and abs(enc.records[b0][2]) > _lib.TILED_H)
    return dict(blocks=len(blocks) - big, shifts=big, tile_launches=sum(t for _, _, t in blocks), peak=enc.tiled_capacity() and
                enc._tiled_walk(None, None, None)[1])


@pytest.mark.parametrize("case", ["mrf", "mse", "big_shift", "capped", "reset"])
def test_library_schedule_matches_the_model(case):
    """epgx_tiled_info (the schedule the library launches, cut on fused records) against Encoder.tiled_blocks (cut on
    operators): the same blocks, tiles and peak on trains whose records hold one shift each"""
    T1, T2 = np.array([[600.0], [1400.0]]), np.array([[40.0, 160.0]])
    if case == "mrf":
        seq = [epg.T(180, 0), epg.SPOILER] + [epg.T(30, 90), epg.E(2, T1, T2), epg.ADC, epg.E(8, T1, T2), epg.S(1)] * 2300
    elif case == "mse":
        seq = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.S(1), epg.E(5, 1000, T2), epg.ADC] * 1100
    elif case == "big_shift":
        seq = [epg.T(90, 90)] + [epg.S(1), epg.T(40, 0), epg.ADC] * 700 + [epg.S(300), epg.ADC] + [epg.S(1), epg.T(40, 0), epg.ADC] * 1300
    elif case == "capped":
        seq = [epg.T(90, 90)] + [epg.S(1), epg.T(40, 0), epg.ADC] * 3000
    else:
        seq = [epg.T(90, 90)] + [epg.S(1), epg.T(40, 0), epg.ADC] * 2500 + [epg.RESET, epg.T(90, 90)] + [epg.S(1), epg.T(40, 0), epg.ADC] * 600
    options = {"max_nstate": 2200} if case == "capped" else {}
    ctx, enc, plan = device_plan(seq, **options)
    Kbuf = enc.tiled_capacity()
    info = _lib.tiled_info(ctx, plan, Kbuf)
    model = schedule_model(enc, Kbuf)
    assert {k: info[k] for k in model} == model, (info, model)


# ------------------------------------------------------------------ (g) the reference's own numbers (tests/golden/make_golden_long.py)
def _golden_long():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_long.py")
    spec = importlib.util.spec_from_file_location("make_golden_long", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)      # (the module imports the reference only when run as a program)
    return mod


@pytest.mark.parametrize("case", ["cpmg", "mrf", "hyper", "capped"])
def test_g18_long_trains(golden, case):
    g = golden("g18_long_trains")
    gen = _golden_long()
    inputs = gen.inputs()
    for key in g.files:                  # the stored parameters are the generator's
        if key in inputs:
            assert np.array_equal(g[key], inputs[key]), key
    seq = gen.sequences(epg, inputs)[case]
    enc = functions.compile_sequence(seq)[0]
    with pytest.raises(NotImplementedError):
        enc.capacity(resident=True)      # every train runs on the tiled path
    close(epg.simulate(seq), g[case])
