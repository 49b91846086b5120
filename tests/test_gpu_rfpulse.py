"""Shaped RF pulses on the device: the G19 cases of the reference; a collapsed pulse (ONE EPGX_OP_MAT0 record whose table
chain_kernel multiplies up, csrc/epgx_chain.hip) against its members run one by one and against the C oracle on the expanded
tuples, in every mode simulate() has; the table itself against Collapsed.host_table(); what epgx_plan_create_ext rejects.
Tolerance: the project's 1e-12 absolute on O(1) signals, every voxel and every probe."""
import numpy as np
import pytest

from epgpy_amd import epg, exchange, collapse, functions, _lib, EpgxError
from oracle import epg_c
from tests import rfpulse_cases as rc
from tests.rfpulse_cases import mg

pytestmark = pytest.mark.gpu
TOL = 1e-12
MAT0_KERNELS = ("run_kernel", "run_contig", "deriv_kernel", "xrun_kernel", "tiled_kernel")


def close(a, b, what="", tol=TOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.max(np.abs(a - b)))
    print(what, "max |a - b| =", err)
    assert err <= tol, (what, err)


@pytest.fixture(scope="module")
def g19():
    return np.load(rc.GOLDEN)


@pytest.mark.parametrize("collapsed", [True, False])
def test_g19_cases(g19, collapsed):
    for name, (seq, kw) in mg.cases(epg).items():
        F0, Z0 = epg.simulate(seq, probe=("F0", "Z0"), collapse=collapsed, **kw)
        close(F0, g19[name + "_F0"], f"{name} F0 collapse={collapsed}")
        close(Z0, g19[name + "_Z0"], f"{name} Z0 collapse={collapsed}")


def test_collapsed_against_members_and_oracle_in_every_mode():
    """a 20-echo CPMG (64 orders) with shaped excitation and refocusing over (3 T2 x 9 positions)"""
    seq, tuples = rc.cpmg(epg, 20, [30.0, 80.0, 200.0], nsample=32, npoint=9, shaped_excitation=True)
    ref = epg_c.simulate(tuples)
    assert ref.shape == (20, 3, 9)
    plain = epg.simulate(seq, collapse=False)
    close(plain, ref, "members vs oracle")
    for mode in ("resident", "stream", "stepwise"):
        close(epg.simulate(seq, mode=mode), ref, f"collapsed ({mode}) vs oracle")
    close(epg.simulate(seq), plain, "collapsed vs members")
    close(epg.simulate(seq, fuse=False), ref, "collapsed, fuse=False vs oracle")
    enc, _, _ = epg.compile_sequence(seq)
    assert enc.capacity() == 64 and enc.packable() == 0
    ctx = _lib.get_context(0)
    name = _lib.kernel_for(ctx, enc.device_plan(ctx, 64), 64)
    assert name.startswith(MAT0_KERNELS), name


def test_256_orders():
    seq, tuples = rc.cpmg(epg, 100, [60.0, 150.0], nsample=16, npoint=5)
    enc, _, _ = epg.compile_sequence(seq)
    assert enc.capacity() == 256
    ctx = _lib.get_context(0)
    assert _lib.kernel_for(ctx, enc.device_plan(ctx, 256), 256).startswith(MAT0_KERNELS)
    ref = epg_c.simulate(tuples)
    close(epg.simulate(seq), ref, "256 orders, collapsed vs oracle")
    close(epg.simulate(seq, mode="stream"), ref, "256 orders, stream vs oracle")
    close(epg.simulate(seq, collapse=False), ref, "256 orders, members vs oracle")


def test_init_device_output_single_precision():
    seq, tuples = rc.cpmg(epg, 8, [40.0, 120.0], nsample=16, npoint=7)
    ref = epg.simulate(seq, collapse=False)
    dev = epg.simulate(seq, out="device")
    assert isinstance(dev, functions.DeviceSignal)
    close(np.asarray(dev), ref, 'out="device"')
    c64 = epg.simulate(seq, dtype=np.complex64)
    assert c64.dtype == np.complex64
    close(c64, ref, "complex64", tol=2e-7)
    close(c64, epg.simulate(seq).astype(np.complex64), "complex64 = rounded complex128", tol=0.0)
    init = mg.PREPARED
    close(epg.simulate(seq, init=init), epg.simulate(seq, init=init, collapse=False), "init=")
    sm = epg.StateMatrix(init)
    close(epg.simulate(seq, init=sm, mode="stream"), epg.simulate(seq, init=init, collapse=False), "init= StateMatrix, stream")
    # op(sm): a pulse applied to a state matrix runs its members (the per-operator path is unchanged)
    pulse = epg.encode_phase(epg.RFPulse(rc.sinc_pulse(16), 2.0, alpha=90), 8.0, 16.0, npoint=7, rewind=True)
    out = pulse(epg.StateMatrix(init))
    F0, Z0 = epg.simulate([pulse, epg.ADC], probe=("F0", "Z0"), init=init)
    close(out.F0, F0[0], "op(sm) F0")
    close(out.Z0, Z0[0], "op(sm) Z0")


def test_voxel_ranges():
    """the plan run in voxel ranges (what ngpu / sharded runs do with it) gives the bits of the whole grid"""
    seq, _ = rc.cpmg(epg, 6, np.linspace(30, 200, 8), nsample=16, npoint=16)
    enc, _, _ = epg.compile_sequence(seq)
    ctx = _lib.get_context(0)
    K = enc.capacity()
    plan = enc.device_plan(ctx, K)
    nvox = enc.nvox
    assert nvox == 128
    whole = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    _lib.run(ctx, plan, 0, plan.n_ops, 0, nvox, None, None, K, whole.ptr.value, nvox, 0)
    ref = whole.download(np.complex128, (enc.n_adc, nvox))
    parts = _lib.DeviceBuffer(ctx, 16 * enc.n_adc * nvox)
    for v0, cnt in ((0, 40), (40, 3), (43, 85)):
        _lib.run(ctx, plan, 0, plan.n_ops, v0, cnt, None, None, K, parts.ptr.value, nvox, v0)
    assert np.array_equal(parts.download(np.complex128, (enc.n_adc, nvox)), ref)
    close(ref.reshape((enc.n_adc,) + enc.grid), epg.simulate(seq, collapse=False), "whole grid vs members")
    assert np.array_equal(epg.simulate(seq), ref.reshape((enc.n_adc,) + enc.grid))


def test_jacobian_with_the_variable_outside_the_pulse():
    T2 = np.array([40.0, 90.0, 160.0])
    wave = rc.sinc_pulse(16)
    rfc = epg.encode_phase(epg.RFPulse(wave, 2.0, alpha=150), 8.0, 16.0, npoint=5)
    relax = epg.E(4.0, 1000.0, T2, order1=["T2"])
    seq = [epg.T(90, 90)] + [relax, epg.S(1), rfc, epg.S(1), relax, epg.ADC] * 10
    probe = epg.Jacobian(["magnitude", "T2"])
    enc, _, _ = epg.compile_sequence(seq, [probe], variables=["T2"])
    assert enc.plan_arrays(64)["ops"]["opcode"].tolist().count(_lib.OP_MAT0) == 10
    ctx = _lib.get_context(0)
    assert _lib.kernel_for(ctx, enc.device_plan(ctx, 64), 64).startswith(MAT0_KERNELS)
    got = epg.simulate(seq, probe=probe)
    want = epg.simulate(seq, probe=probe, collapse=False)
    assert got.shape == (10, 3, 5, 2)
    close(got, want, "Jacobian collapsed vs members")
    # and against a central difference of the collapsed simulation itself
    h = 1e-3
    def at(t2):
        r = epg.E(4.0, 1000.0, t2)
        return epg.simulate([epg.T(90, 90)] + [r, epg.S(1), rfc, epg.S(1), r, epg.ADC] * 10)
    fd = (at(T2 + h) - at(T2 - h)) / (2 * h)
    close(got[..., 1], fd, "dS/dT2 vs central difference", tol=1e-8)


def test_pulse_inside_an_exchange_sequence():
    wave = rc.sinc_pulse(16)
    pulse = epg.RFPulse(wave, 1.0, alpha=40, T1=[900.0, 300.0], T2=[80.0, 20.0])
    assert pulse.shape == (2,)
    exg = epg.X(5.0, exchange.exchange_matrix(0.05, densities=[0.8, 0.2]), T1=[900, 300], T2=[80, 20])
    seq = [[pulse, epg.ADC, exg, epg.S(1)] for _ in range(12)]
    enc, _, _ = epg.compile_sequence(seq)
    ops = enc.plan_arrays(64)["ops"]["opcode"].tolist()
    assert ops.count(_lib.OP_MAT0) == 12 and ops.count(_lib.OP_X) == 12
    ctx = _lib.get_context(0)
    assert _lib.kernel_for(ctx, enc.device_plan(ctx, 64), 64).startswith("xrun_kernel")
    close(epg.simulate(seq), epg.simulate(seq, collapse=False), "X: collapsed vs members")
    close(epg.simulate(seq, mode="stream"), epg.simulate(seq, collapse=False), "X stream: collapsed vs members")


def test_tiled_path():
    """1100 echoes: 2200 orders, beyond the capacity classes"""
    seq, tuples = rc.cpmg(epg, 1100, [60.0, 180.0], nsample=8, npoint=3)
    enc, _, _ = epg.compile_sequence(seq)
    assert enc.peak == 2200 and enc.tiled_ok()
    with pytest.raises(NotImplementedError):
        enc.capacity(resident=True)
    ref = epg_c.simulate(tuples)
    close(epg.simulate(seq), ref, "tiled, collapsed vs oracle")
    close(epg.simulate(seq, collapse=False), ref, "tiled, members vs oracle")


@pytest.mark.parametrize("case", ["plain", "relax", "phi_profile", "b1", "large"])
def test_device_table_against_host_table(case):
    """the table chain_kernel wrote, read back through a one-order simulate from random states, against
    Collapsed.host_table() -- uniform sources (scalar loads), per-entry sources, assembled sources (large grids)"""
    rng = np.random.default_rng(11)
    wave = mg.waveforms()["quad128"][::2]
    if case == "plain":
        op = epg.RFPulse(wave, 2.0, rf=0.8)
    elif case == "relax":
        op = epg.RFPulse(wave, 3.0, rf=0.8, T1=600.0, T2=np.array([20.0, 60.0, 200.0]), g=np.linspace(-1, 1, 5)[None, :])
    elif case == "phi_profile":
        op = epg.encode_phase(epg.RFPulse(wave, 2.0, rf=0.7, phi=40.0, T1=500.0, T2=35.0), 9.0, 12.0, npoint=11, rewind=0.4)
    elif case == "b1":
        op = epg.encode_phase(epg.RFPulse(wave, 2.0, rf=np.array([[0.5], [0.8], [1.1]]), alpha=90), 9.0, 12.0, npoint=4)
    else:   # 33 x 40 x 24 entries: the relaxation table is assembled on the device from per-axis columns
        op = epg.RFPulse(wave, 2.0, rf=0.8, T1=np.linspace(300, 2000, 40)[None, :, None], T2=np.linspace(20, 200, 24)[None, None, :],
                         g=np.linspace(-2, 2, 33)[:, None, None])
    col = collapse.collapsed_of(op)
    f = rng.normal(size=col.shape) + 1j * rng.normal(size=col.shape)
    z = rng.normal(size=col.shape)
    state = np.stack([f, np.conj(f), z + 0j], axis=-1)
    enc, _, _ = epg.compile_sequence([op, epg.ADC], shape=col.shape)
    arrays = enc.plan_arrays(64)
    assert len(arrays["chain"]) == 1 and (case != "large" or arrays["assemble"] is not None)
    F0, Z0 = epg.simulate([op, epg.ADC], probe=("F0", "Z0"), init=state[..., None, :])
    f_new, z_new = rc.apply_table(col.host_table(), state)
    close(F0[0], f_new, f"{case}: F0 through the device table")
    close(Z0[0], z_new, f"{case}: Z0 through the device table")


def tampered(arrays, **changes):
    """the plan arrays with one chain step / destination changed"""
    out = dict(arrays)
    dst, space, steps = arrays["chain"][0]
    steps = steps.copy()
    for key, val in changes.items():
        if key == "dst":
            dst = val
        elif key == "dst_space":
            space = val
        else:
            index, field = key.split("_", 1)
            steps[int(index[1:])][field] = val
    out["chain"] = [(dst, space, steps)]
    return out


def test_invalid_chains_are_refused():
    T2 = np.array([40.0, 120.0])
    pulse = epg.RFPulse(rc.sinc_pulse(8), 1.0, alpha=60, T1=900.0, T2=T2)
    prof = epg.encode_phase(pulse, 8.0, 16.0, npoint=5)
    enc, _, _ = epg.compile_sequence([prof, epg.ADC])
    arrays = enc.plan_arrays(64)
    ctx = _lib.get_context(0)
    _lib.DevicePlan(ctx, **arrays)                                   # the plan itself is fine
    dst, space, steps = arrays["chain"][0]
    n_host, n_pool = len(arrays["coef"]), len(arrays["coef"]) + arrays["n_coef_generated"]
    assert steps["kind"].tolist() == [_lib.OP_T, _lib.OP_E, _lib.OP_E] and enc.grid == (2, 5)
    narrow = next(s for s, st in enumerate(enc.spaces) if st != enc.spaces[space])      # a space over ONE axis: not the destination's
    cases = {
        "destination outside the generated part": [dict(dst=0), dict(dst=n_host - 14), dict(dst=n_pool - 13)],
        "source neither inside the host part": [dict(s0_off=n_host), dict(s0_stride=n_host), dict(s1_off=n_pool)],
        "negative source offset": [dict(s0_off=-8), dict(s0_stride=-8)],
        "unknown kind": [dict(s0_kind=_lib.OP_S), dict(s1_kind=99), dict(s1_kind=_lib.OP_T0)],
        "malformed group": [dict(s0_group=5), dict(s0_group=4), dict(s0_count=0), dict(s0_group=0)],
        "index space": [dict(s1_space=7), dict(dst_space=-2)],
        "varies along an axis the destination does not": [dict(dst_space=narrow, dst=dst)],
    }
    for text, changes in cases.items():
        for change in changes:
            with pytest.raises(EpgxError) as info:
                _lib.DevicePlan(ctx, **tampered(arrays, **change))
            assert "(-1)" in str(info.value) and text in str(info.value), (change, str(info.value))
    # an operator that points into the generated part without a recipe
    with pytest.raises(EpgxError, match="needs a recipe"):
        _lib.DevicePlan(ctx, **{k: v for k, v in arrays.items() if k != "chain"})
    # a struct of another size
    import ctypes
    desc, keep = _lib.plan_desc(**arrays)
    ext, keep_ext = _lib.plan_ext(arrays["chain"])
    ext.struct_size = 8
    handle = ctypes.c_void_p()
    assert ctx.lib.epgx_plan_create_ext(ctx.handle, ctypes.byref(desc), ctypes.addressof(ext), ctypes.byref(handle)) == -1
    assert b"struct_size" in ctx.lib.epgx_last_error() and not handle.value
