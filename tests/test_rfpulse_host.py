"""RFPulse / encode_phase on the host (no GPU): the reference's values (G19, tests/golden/make_golden_rfpulse.py), exceptions
and operator lists; which operators a plan keeps whole and collapses into one EPGX_OP_MAT0 record with a chain recipe
(collapse.py), and when it falls back to the members; Collapsed.host_table() against the oracle's NumPy port."""
import numpy as np
import pytest

from epgpy_amd import epg, _lib, collapse, functions, rfpulse
from oracle import epg_numpy as onp
from tests import rfpulse_cases as rc
from tests.rfpulse_cases import mg


@pytest.fixture(scope="module")
def g19():
    return np.load(rc.GOLDEN)


# ------------------------------------------------------------------ the reference's numbers
def test_host_functions_match_the_reference(g19):
    """estimate_rf / estimate_alpha / spatial_range / space_to_freq / freq_to_space against G19: 1e-14, except the rf that
    scipy's optimiser finds (the quadratic-phase waveform): 1e-6 relative, its own tolerance"""
    got = mg.host_values(epg)
    assert set(got) <= set(g19.files)
    for name, val in got.items():
        ref = g19[name]
        assert np.shape(val) == ref.shape, name
        rel = float(np.max(np.abs(val - ref) / np.maximum(np.abs(ref), 1e-300)))
        print(name, rel)
        assert rel <= (1e-6 if name.startswith("rf_quad128") else 1e-14), (name, rel)
    for name, wave in mg.waveforms().items():
        assert np.array_equal(g19["wave_" + name], wave)
    # the optimiser really ran for the quadratic-phase waveform: its rf is not the closed form
    quad = mg.waveforms()["quad128"]
    closed = 90 / 180 / abs(quad.sum())
    assert abs(got["rf_quad128_90"] - closed) > 1e-4 * closed


def test_exceptions_of_the_reference(monkeypatch):
    wave = rc.sinc_pulse(8)
    with pytest.raises(ValueError, match="rf"):
        epg.RFPulse(wave, 1.0)
    with pytest.raises(ValueError, match="magnitude"):
        epg.RFPulse(2 * wave, 1.0, rf=1)
    with pytest.raises(ValueError, match="magnitude"):
        rfpulse.estimate_rf(2 * wave, 90)
    with pytest.raises(ValueError, match="1-dimensional"):
        rfpulse.make_pulse_sequence(epg.T, wave.reshape(2, 4), 1.0, 1.0)
    with pytest.raises(ValueError, match="same length"):
        epg.RFPulse(wave, [0.1] * 7, rf=1)
    with pytest.raises(TypeError, match="RFPulse"):
        epg.encode_phase(epg.T(90, 0), 10, 20)
    with pytest.raises(TypeError, match="RFPulse"):
        epg.encode_phase(epg.MultiOperator([epg.T(90, 0)]), 10, 20)
    monkeypatch.setattr(rfpulse, "optimize", None)
    assert rfpulse.estimate_rf(wave, 90) > 0                      # constant phase: closed form, no scipy
    with pytest.raises(RuntimeError, match="Scipy"):
        rfpulse.estimate_rf(mg.waveforms()["quad128"], 90)


def test_operator_lists_shapes_and_durations():
    """test/test_rfpulse.py of the reference: members, attributes, durations; per-sample durations; get_adc_times"""
    pulse = epg.RFPulse([0.5, 1, 0.5], 3.0, rf=1)
    assert isinstance(pulse, epg.MultiOperator) and len(pulse) == 3 and pulse.duration == 3.0 and pulse.shape == (1,)
    assert pulse.rf == 1 and pulse.phi is None and np.isclose(epg.RFPulse([0.5], 1.0, rf=1).alpha, 90)
    assert [type(op) for op in pulse] == [epg.T] * 3 and [op.duration for op in pulse] == [1.0] * 3
    assert np.allclose([op.alpha for op in pulse], [90, 180, 90]) and pulse.name == "RFPulse(3, 3.0ms)"
    assert not hasattr(pulse, "T1")
    relaxed = epg.RFPulse([1, 1j], duration=1, rf=1, T1=1000, T2=100)
    assert [type(op) for op in relaxed] == [epg.T, epg.E, epg.T, epg.E] and (relaxed.T1, relaxed.T2, relaxed.g) == (1000, 100, 0)
    assert relaxed[1] is relaxed[3]                               # equal durations: ONE relaxation object
    assert relaxed[1].tau == 0.5 and relaxed[1].duration == 0 and relaxed.duration == 1
    uneven = epg.RFPulse([1, 1j, 0.5], [0.2, 0.3, 0.2], rf=0.1, T2=50)
    assert uneven[1] is uneven[5] and uneven[1] is not uneven[3] and uneven[3].tau == 0.3
    assert uneven[1].T1 == 1e10 and uneven.duration == [0.2, 0.3, 0.2]
    offset = epg.RFPulse([1, 1], 1.0, rf=0.25, phi=30)
    assert [type(op) for op in offset] == [epg.Phi, epg.T, epg.T, epg.Phi] and (offset[0].phi, offset[3].phi) == (-30, 30)
    # B1 axis: rf with two axes
    b1 = epg.RFPulse([0.5, 1], 1.0, rf=np.array([[0.2], [0.25]]), alpha=45)
    assert b1.shape == (2, 1) and b1[0].alpha.shape == (2, 1)
    profile = epg.encode_phase(relaxed, 10.0, 20.0, npoint=5, rewind=True)
    assert type(profile) is epg.MultiOperator and profile.shape == (1, 5) and len(profile) == 7
    assert [type(op) for op in profile] == [epg.T, epg.P, epg.E, epg.T, epg.P, epg.E, epg.P]
    assert profile[1] is profile[4] and np.array_equal(profile[6].g, -profile[1].g) and profile[6].tau == 0.5
    assert np.allclose(profile[1].g, epg.space_to_freq(10.0, epg.spatial_range(20.0, 5))[None, :])
    flat = epg.encode_phase(pulse, 10.0, np.array([-1.0, 0.0, 1.0]), expand=False, rewind=0.25)
    assert flat.shape == (3,) and flat[-1].tau == 0.75
    times = epg.get_adc_times([pulse, epg.ADC, epg.Wait(2.0), relaxed, epg.ADC])
    assert times == [3.0, 6.0]
    seq, tuples = rc.cpmg(epg, 2, [50.0])
    assert epg.getshape(seq) == (1, 9) and epg.getnshift(seq) == 4


def test_flag_travels_through_modify_and_encode_phase():
    pulse = epg.RFPulse(rc.sinc_pulse(8), 1.0, alpha=30)
    assert pulse.collapsible and not epg.MultiOperator([epg.T(10, 0)]).collapsible
    assert not (epg.T(10, 0) * epg.E(1, 100, 10)).collapsible
    modified = epg.modify(pulse, T1=800.0, T2=[40.0, 60.0])
    assert type(modified) is epg.MultiOperator and modified.collapsible and modified.shape == (2,)
    assert epg.encode_phase(pulse, 5.0, 10.0, npoint=3).collapsible
    assert epg.encode_phase(pulse, 5.0, 10.0, npoint=3, rewind=True).collapsible
    assert not epg.modify(epg.MultiOperator([epg.T(10, 0, duration=1.0)]), T2=30.0).collapsible
    assert isinstance(epg.modify([pulse, epg.ADC], T2=30.0), list)


# ------------------------------------------------------------------ plans
def opcodes(enc, K=64):
    return enc.plan_arrays(K)["ops"]["opcode"].tolist()


def test_a_pulse_used_six_times_is_six_records_and_one_table():
    seq, _ = rc.cpmg(epg, 6, [40.0, 120.0], nsample=32, npoint=9)
    enc, records, _ = epg.compile_sequence(seq, fuse=False)          # (fuse: the E . T . E pass would merge the train's relaxations)
    arrays = enc.plan_arrays(64)
    ops = arrays["ops"]
    assert opcodes(enc).count(_lib.OP_MAT0) == 6 and len(ops) == 1 + 6 * 6 and len(records) == 6
    mat0 = ops[ops["opcode"] == _lib.OP_MAT0]
    assert len(set(mat0["coef_off"].tolist())) == 1 and mat0["ncoef"].tolist() == [14] * 6
    chains = arrays["chain"]
    assert len(chains) == 1
    dst, space, steps = chains[0]
    # ONE group (T_i, P) repeated 32 times: two steps; the rotations lie one table (8 doubles) apart, the precession stays
    assert steps["kind"].tolist() == [_lib.OP_T, _lib.OP_E] and steps["count"].tolist() == [32, 0] and steps["group"].tolist() == [2, 0]
    assert steps["stride"].tolist() == [8, 0] and steps["space"].tolist() == [-1, space]
    assert enc.spaces[space] == (0, 1)                            # the table varies along the position axis only
    assert arrays["n_coef_generated"] == 9 * 14 and dst == mat0["coef_off"][0] == len(arrays["coef"])
    assert len(arrays["coef"]) == 8 + 2 * 4 + 32 * 8 + 9 * 4      # excitation, relaxation (2 T2), 32 rotations, one precession table
    # with relaxation inside the pulse and the rewinder: (T_i, P, E) x N, then P
    pulse = epg.RFPulse(rc.sinc_pulse(16), 1.0, alpha=90, T1=900.0, T2=60.0)
    prof = epg.encode_phase(pulse, 8.0, 16.0, npoint=5, rewind=True)
    enc, _, _ = epg.compile_sequence([prof, epg.ADC])
    (_, _, steps), = enc.plan_arrays(64)["chain"]
    assert steps["count"].tolist() == [16, 0, 0, 1] and steps["group"].tolist() == [3, 0, 0, 1]
    assert collapse.collapsed_of(prof).n_steps == 4 and collapse.collapsed_of(prof) is collapse.collapsed_of(prof)


def test_collapse_false_gives_the_primitives():
    seq, _ = rc.cpmg(epg, 3, [40.0, 120.0], nsample=16, npoint=5)
    enc, _, _ = epg.compile_sequence(seq, collapse=False, fuse=False)
    arrays = enc.plan_arrays(64)
    assert "chain" not in arrays and arrays["n_coef_generated"] == 0 and _lib.OP_MAT0 not in opcodes(enc)
    assert opcodes(enc).count(_lib.OP_T) == 1 + 3 * 16 and opcodes(enc).count(_lib.OP_E) == 3 * (16 + 2)
    flat = functions.flatten_sequence(seq)
    assert len(flat) == 1 + 3 * (5 + 32) and not any(isinstance(op, epg.MultiOperator) for op in flat)
    kept = functions.flatten_sequence(seq, keep_collapsible=True)
    assert sum(isinstance(op, epg.MultiOperator) for op in kept) == 3


def collapsed_count(seq, **kw):
    enc, _, _ = epg.compile_sequence(seq, **kw)
    arrays = enc.plan_arrays(enc.capacity())
    return arrays["ops"]["opcode"].tolist().count(_lib.OP_MAT0), len(arrays.get("chain", ()))


def test_fallbacks(monkeypatch):
    wave = rc.sinc_pulse(8)
    relax = epg.E(5.0, 1000.0, [40.0, 80.0], order1=["T2"])
    # (a) a member carries order1 for one of the plan's variables -- and only then
    diff_t = lambda alpha, phi, duration: epg.T(alpha, phi, duration=duration, order1={"fa": "alpha"})      # noqa: E731
    pulse = epg.RFPulse(wave, 1.0, rf=0.3, transform=diff_t)
    seq = [epg.T(90, 90), relax, epg.S(1), pulse, epg.S(1), relax, epg.ADC]
    assert collapsed_count(seq) == (1, 1)
    assert collapsed_count(seq, variables=["T2"]) == (1, 1)
    assert collapsed_count(seq, variables=["fa"]) == (0, 0)
    assert collapsed_count(seq, variables=["T2", "fa"]) == (0, 0)
    # (b) a member that is no state-wise matrix / scalar operator
    plain = epg.RFPulse(wave, 1.0, rf=0.3)
    assert collapsed_count([plain, epg.ADC]) == (1, 1)
    for extra in (epg.S(1), epg.SPOILER, epg.ADC):
        grown = epg.RFPulse(wave, 1.0, rf=0.3)
        grown.append(extra)
        assert collapsed_count([grown, epg.S(1), epg.ADC]) == (0, 0)
    # (c) more broadcast patterns than the plan has index spaces
    axis = lambda d, vals: np.asarray(vals, dtype=float).reshape((1,) * d + (len(vals),))      # noqa: E731
    spread = [epg.E(1.0, 1000.0, axis(d, [30.0 + d, 60.0 + d])) for d in range(4)]
    fifth = epg.RFPulse(wave, 1.0, rf=0.3, T2=axis(4, [20.0, 50.0]))
    assert collapsed_count(spread[:3] + [fifth, epg.ADC]) == (1, 1)
    assert collapsed_count(spread + [fifth, epg.ADC]) == (0, 0)
    # (d) the budget of device-generated tables: 14 doubles per entry and distinct pulse object
    wide = epg.encode_phase(plain, 5.0, 10.0, npoint=100)
    assert collapsed_count([wide, epg.S(1), wide, epg.ADC]) == (2, 1)
    monkeypatch.setattr(functions, "FUSED_TABLE_BUDGET", 100 * 14 * 8 - 1)
    assert collapsed_count([wide, epg.S(1), wide, epg.ADC]) == (0, 0)
    monkeypatch.setattr(functions, "FUSED_TABLE_BUDGET", 100 * 14 * 8)
    assert collapsed_count([wide, epg.S(1), wide, epg.ADC]) == (2, 1)
    # (e) the caller's choice
    assert collapsed_count([wide, epg.ADC], collapse=False) == (0, 0)


def test_unflagged_sequences_compile_to_the_same_bytes():
    from tests import sequences as sq  # noqa: F401  (the package's own sequences need no pulse)
    T2 = np.linspace(30, 200, 7)
    relax = epg.E(5.0, 1000.0, T2)
    multi = epg.T(120, 0) * epg.P(1.0, 0.01)           # an ordinary MultiOperator: not flagged
    seqs = [[epg.T(90, 90)] + [relax, epg.S(1), epg.T(150, 0), epg.S(1), relax, epg.ADC] * 5,
            [epg.T(90, 90)] + [epg.S(1), relax, multi, epg.S(1), relax, epg.ADC] * 4,
            epg.modify([epg.T(30, 0, duration=2.0), epg.ADC, epg.S(1, duration=5.0)] * 6, T1=900.0, T2=T2)]
    for seq in seqs:
        a = epg.compile_sequence(seq)[0].plan_arrays(64)
        b = epg.compile_sequence(seq, collapse=False)[0].plan_arrays(64)
        assert a.keys() == b.keys() and "chain" not in a
        for key in a:
            if isinstance(a[key], np.ndarray):
                assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
            else:
                assert np.array_equal(a[key], b[key]) if isinstance(a[key], list) else a[key] == b[key], key


# ------------------------------------------------------------------ the table itself
@pytest.mark.parametrize("case", ["plain", "relax", "phi_profile", "b1"])
def test_host_table_against_the_oracle(case):
    """Collapsed.host_table() (the NumPy restatement of chain_kernel) applied to random single-order states == the oracle
    walking the expanded tuples.  Bound: the project's 1e-12 on O(1) values (a few hundred steps of a few roundings each)"""
    rng = np.random.default_rng(7)
    wave = mg.waveforms()["quad128"][::2]
    if case == "plain":
        op = epg.RFPulse(wave, 2.0, rf=0.8)
        tuples = rc.pulse_tuples(wave, 2.0, 0.8)
    elif case == "relax":
        T2, g = np.array([20.0, 60.0, 200.0]), np.linspace(-1, 1, 5)[None, :]
        op = epg.RFPulse(wave, 3.0, rf=0.8, T1=600.0, T2=T2, g=g)
        tuples = rc.pulse_tuples(wave, 3.0, 0.8, T1=600.0, T2=T2, g=g)
    elif case == "phi_profile":
        pulse = epg.RFPulse(wave, 2.0, rf=0.7, phi=40.0, T1=500.0, T2=35.0)
        op = epg.encode_phase(pulse, 9.0, 12.0, npoint=11, rewind=0.4)
        tuples = rc.pulse_tuples(wave, 2.0, 0.7, phi=40.0, T1=500.0, T2=35.0, g=0, slice_freqs=rc.slice_freqs(9.0, 12.0, 11), rewind=0.4)
    else:
        rf = np.array([[0.5], [0.8], [1.1]])
        op = epg.encode_phase(epg.RFPulse(wave, 2.0, rf=rf, alpha=90), 9.0, 12.0, npoint=4)
        tuples = rc.pulse_tuples(wave, 2.0, rf, slice_freqs=rc.slice_freqs(9.0, 12.0, 4, 2))
    col = collapse.collapsed_of(op)
    assert col.shape == tuple(op.shape) and set(map(type, col.members)) <= {epg.T, epg.E, epg.P, epg.Phi}
    table = col.host_table()
    assert table.shape == col.shape + (14,) and not table[..., 9].any() and not table[..., 13].any()
    f = rng.normal(size=col.shape) + 1j * rng.normal(size=col.shape)
    z = rng.normal(size=col.shape)
    state = np.stack([f, np.conj(f), z + 0j], axis=-1)
    ref = onp.simulate(tuples + [("ADC",), ("ADC", "Z0")], init=state[..., None, :], shape=col.shape)
    f_new, z_new = rc.apply_table(table, state)
    err = max(float(np.max(np.abs(f_new - ref[0]))), float(np.max(np.abs(z_new - ref[1]))))
    print(case, "max |host_table - oracle| =", err)
    assert err <= 1e-12
    assert float(np.max(np.abs(z_new.imag))) <= 1e-15
