"""Run analysis on the device: what tests/host/run_check.cpp cannot reach.

  * the refusals that compare handles -- a NULL context or plan, a plan, `in` or `out` of another context -- of epgx_run,
    epgx_kernel_for and epgx_run_tiled, through raw ctypes, with code and text;
  * epgx_kernel_for agrees with the launch: for one tiny plan per route (records at K = 16, 64 and 128, xrun_kernel, the split
    path, dxrun_kernel) the name it returns is the one the `[epgx] run:` trace line of the real epgx_run of the same range
    carries, and the signal of that run equals the host recurrence's to 1e-12.  EPGX_TRACE is set for a child process of its
    own, started before any GPU call in it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epgpy_amd import epg, _lib
from epgpy_amd import functions as _functions
from tests.exchange_recurrence import recurrence
from tests.exchange_jacobian_recurrence import exchange_jacobian_recurrence

pytestmark = pytest.mark.gpu

ATOL = 1e-12
INVALID = -1


# ------------------------------------------------------------------------------------------------ plans
def _plain_sequence():
    """8 voxels, 7 operators, orders up to 2"""
    alpha, T2 = np.linspace(20.0, 90.0, 8), np.linspace(30.0, 100.0, 8)
    return [epg.T(alpha, 90.0), epg.E(5.0, 1000.0, T2), epg.S(1), epg.ADC, epg.T(150.0, 0.0), epg.S(1), epg.ADC]


def _exchange_sequence(order1=None):
    """2 compartments x 4 groups = 8 voxels, 8 operators"""
    x = epg.X(3.0, 0.05, T1=[800.0, 300.0], T2=[60.0, 15.0], **({"order1": order1} if order1 else {}))
    alpha = np.linspace(20.0, 80.0, 4)
    return [epg.T([alpha], 90.0), epg.ADC, x, epg.S(1), epg.T(120.0, 0.0), epg.ADC, x, epg.S(1)]


def _cases():
    """name -> (sequence, grid, K, variables, the kernel's name where the route alone fixes it)"""
    plain, xseq = _plain_sequence(), _exchange_sequence()
    return {
        "records_16": (plain, (8,), 16, [], None),
        "records_64": (plain, (8,), 64, [], None),
        "records_128": (plain, (8,), 128, [], None),
        "xrun": (xseq, (2, 4), 64, [], "xrun_kernel<2, 1, false>"),
        "split": (xseq, (2, 4), 512, [], "split<exchange_kernel>"),
        "dxrun": (_exchange_sequence({"T1": {"T1": 1}}), (2, 4), 64, ["T1"], "dxrun_kernel<2, 1, 1>"),
    }


def _launch(ctx, seq, grid, K, variables):
    """(name from epgx_kernel_for, signal [n_probe, (1 + V,) *grid] of epgx_run over the same range)"""
    enc, records, _ = _functions.compile_sequence(seq, None, variables=variables)
    assert enc.grid == tuple(grid) and 3 <= len(enc.records) <= 8, (enc.grid, len(enc.records))
    plan = enc.device_plan(ctx, K)
    name = _lib.kernel_for(ctx, plan, K)
    print(f"@@ kernel_for: {name}", file=sys.stderr, flush=True)
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * enc.nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, enc.nvox, None, None, K, sig.ptr.value, enc.nvox, 0)
    rows = (len(records), 1 + len(variables)) if variables else (len(records),)
    assert enc.n_adc == int(np.prod(rows))
    return name, sig.download(np.complex128, rows + tuple(grid))


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_run_check as t
from epgpy_amd import _lib
ctx = _lib.get_context(0)
out = {{}}
for case, (seq, grid, K, variables, _) in t._cases().items():
    print("@@ case", case, file=sys.stderr, flush=True)
    name, out[case] = t._launch(ctx, seq, grid, K, variables)
    out["name_" + case] = np.array(name)
np.savez({path!r}, **out)
"""


def test_kernel_for_agrees_with_the_launch(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "routes.npz")
    env = dict(os.environ, EPGX_TRACE="1")
    proc = subprocess.run([sys.executable, "-c", _CHILD.format(root=root, path=path)], env=env, cwd=root, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    got = np.load(path)
    sections = {part.split("\n", 1)[0].strip(): part for part in proc.stderr.split("@@ case ")[1:]}
    for case, (seq, grid, K, variables, kernel) in _cases().items():
        name = str(got["name_" + case])
        trace = [line for line in sections[case].splitlines() if line.startswith("[epgx] run: ")]
        print(case, "epgx_kernel_for:", name, "| trace:", trace[:1])
        assert f"@@ kernel_for: {name}" in sections[case]
        assert kernel is None or name == kernel, (case, name)
        assert name != "none" and (kernel is not None or "xrun" not in name and "split" not in name), (case, name)
        assert trace and trace[0].startswith(f"[epgx] run: {name} -- "), (case, name, trace[:2])
        if variables:
            want = np.moveaxis(exchange_jacobian_recurrence(seq, variables, grid, 1.0, 3), -1, 1)
            assert float(np.max(np.abs(want[:, 1]))) > 1e-6      # (the derivative reaches the probes)
        else:
            want = recurrence(seq, grid, 1.0, 3)
        err = float(np.max(np.abs(got[case] - want)))
        print(case, "max|gpu - recurrence| =", err)
        assert got[case].shape == want.shape and float(np.max(np.abs(want))) > 0.01 and err <= ATOL, (case, err)


# ------------------------------------------------------------------------------------------------ handles
@pytest.fixture(scope="module")
def two_contexts():
    """a plain plan over 8 voxels and a state at K = 64 on the shared context, and the same on a second context of the device"""
    enc, _, _ = _functions.compile_sequence(_plain_sequence(), None)
    made = []
    for ctx in (_lib.get_context(0), _lib.Context(0)):
        made.append((ctx, enc.device_plan(ctx, 64), _lib.DeviceState(ctx, enc.nvox, 64)))
    return enc, made


def _refused(lib, rc, text):
    message = lib.epgx_last_error().decode()
    print(rc, message)
    assert rc == INVALID and message == text, (rc, message)


def test_epgx_run_handles(two_contexts):
    enc, ((ctx, plan, state), (_, plan2, state2)) = two_contexts
    lib, n, nvox = ctx.lib, plan.n_ops, enc.nvox
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    p = sig.ptr
    _refused(lib, lib.epgx_run(None, plan.handle, 0, n, 0, nvox, None, None, 64, p, nvox, 0), "epgx_run: NULL argument")
    _refused(lib, lib.epgx_run(ctx.handle, None, 0, n, 0, nvox, None, None, 64, p, nvox, 0), "epgx_run: NULL argument")
    _refused(lib, lib.epgx_run(ctx.handle, plan2.handle, 0, n, 0, nvox, None, None, 64, p, nvox, 0), "epgx_run: plan belongs to another context")
    _refused(lib, lib.epgx_run(ctx.handle, plan.handle, 0, n, 0, nvox, state2.handle, state.handle, 64, p, nvox, 0),
             "epgx_run: `in` belongs to another context")
    _refused(lib, lib.epgx_run(ctx.handle, plan.handle, 0, n, 0, nvox, state.handle, state2.handle, 64, p, nvox, 0),
             "epgx_run: `out` belongs to another context")
    # the handles come first, the states after the ranges (tests/host/run_check.cpp has the rest of the order)
    _refused(lib, lib.epgx_run(ctx.handle, plan2.handle, 0, n + 1, 0, nvox, state2.handle, None, 64, p, nvox, 0),
             "epgx_run: plan belongs to another context")
    _refused(lib, lib.epgx_run(ctx.handle, plan.handle, 0, n, 1, nvox, state2.handle, None, 64, p, nvox, 0),
             f"epgx_run: voxel range [1,{nvox + 1}) outside the grid ({nvox} voxels)")
    assert lib.epgx_run(ctx.handle, plan.handle, 0, n, 0, nvox, state.handle, state.handle, 64, p, nvox, 0) == 0   # (nothing else was wrong)
    ctx.synchronize()


def test_epgx_kernel_for_handles(two_contexts):
    import ctypes
    enc, ((ctx, plan, state), (_, plan2, state2)) = two_contexts
    lib, n = ctx.lib, plan.n_ops
    buf = ctypes.create_string_buffer(160)
    _refused(lib, lib.epgx_kernel_for(None, plan.handle, 0, n, 64, None, None, buf, len(buf)), "epgx_kernel_for: NULL argument")
    _refused(lib, lib.epgx_kernel_for(ctx.handle, None, 0, n, 64, None, None, buf, len(buf)), "epgx_kernel_for: NULL argument")
    _refused(lib, lib.epgx_kernel_for(ctx.handle, plan.handle, 0, n, 64, None, None, buf, 1), "epgx_kernel_for: no room for the name")
    _refused(lib, lib.epgx_kernel_for(ctx.handle, plan2.handle, 0, n, 64, None, None, buf, len(buf)), "epgx_run: plan belongs to another context")
    _refused(lib, lib.epgx_kernel_for(ctx.handle, plan.handle, 0, n, 64, state2.handle, None, buf, len(buf)), "epgx_run: `in` belongs to another context")
    _refused(lib, lib.epgx_kernel_for(ctx.handle, plan.handle, 0, n, 64, None, state2.handle, buf, len(buf)), "epgx_run: `out` belongs to another context")
    assert lib.epgx_kernel_for(ctx.handle, plan.handle, 0, n, 64, state.handle, state.handle, buf, len(buf)) == 0 and buf.value


@pytest.mark.parametrize("entry", ["epgx_run_tiled", "epgx_tiled_info"])
def test_tiled_handles(two_contexts, entry):
    import ctypes
    enc, ((ctx, plan, state), (_, plan2, state2)) = two_contexts
    lib, nvox = ctx.lib, enc.nvox
    sig = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    if entry == "epgx_run_tiled":
        def call(c, p, st=None):
            return lib.epgx_run_tiled(c, p, 0, nvox, st, 128, sig.ptr, nvox, 0, 0)
    else:
        buf = ctypes.create_string_buffer(160)

        def call(c, p, st=None):
            return lib.epgx_tiled_info(c, p, 128, 0, None, None, None, None, buf, len(buf))
    _refused(lib, call(None, plan.handle), f"{entry}: NULL argument")
    _refused(lib, call(ctx.handle, None), f"{entry}: NULL argument")
    _refused(lib, call(ctx.handle, plan2.handle), f"{entry}: plan belongs to another context")
    if entry == "epgx_run_tiled":
        _refused(lib, call(ctx.handle, plan.handle, state2.handle), "epgx_run_tiled: `in` belongs to another context")
    assert call(ctx.handle, plan.handle, state.handle) == 0, lib.epgx_last_error().decode()   # (64 orders of `in`, two shifts: Kbuf = 128)
    ctx.synchronize()
