"""CPU: the case table of tests/lanes_path_cases.py, which tests/test_gpu_lanes_paths.py runs on the device.

  * FLOORS is honest: for every case at least the float64 oracle's largest per-record error against the extended-precision
    recurrence and at most twice it; 16 x floor stays within 2e-12;
  * no bounded record is vacuous: every probed record has max_vox|ref| >= 1e-3, except behind a lone S(+1), where the reference
    is identically zero (and the device must return exact zeros);
  * the table covers what it claims: every (kernel, NSP) pair of the launch tables is named by a case on some side -- with a train
    that crosses the register deck and a grid with a third, ragged workgroup -- or listed as unreachable; the NSP a case claims
    is the number of index spaces its plan has; the sub-ranges start mid-wave and end in a ragged block;
  * the checks bite: the per-record check, the tiling check and the sub-range check reject planted errors that the whole-array
    `close(.., 1e-12)` of tests/test_gpu_parity.py admits."""
import numpy as np
import pytest

from tests import lanes_path_cases as lp
from tests.signal_recurrence import record_errors

_REF = {}


def reference(name):
    if name not in _REF:
        _REF[name] = (lp.reference(name), lp.reference(name, oracle=True))
    return _REF[name]


@pytest.mark.parametrize("name", list(lp.CASES))
def test_floor_table_is_honest(name):
    want, got = reference(name)
    floor = max(record_errors(got, want))
    print(name, "float64 floor", floor, "table", lp.FLOORS[name])
    assert floor <= lp.FLOORS[name] <= 2 * floor, (name, floor, lp.FLOORS[name])
    assert lp.MARGIN * lp.FLOORS[name] <= lp.CAP, name


def test_floor_table_names_every_case():
    assert set(lp.FLOORS) == set(lp.CASES)


@pytest.mark.parametrize("name", list(lp.CASES))
def test_every_bounded_record_is_non_vacuous(name):
    want, _ = reference(name)
    c = lp.CASES[name]
    assert want.shape == (sum(1 for t in c["tuples"] if t[0] == "ADC"),) + lp.grid_of_case(c)
    if name.startswith("odd_lead_"):
        assert not want.any() and lp.FLOORS[name] == 0.0      # every probe reads the parity nothing reaches
        return
    scales = [float(np.max(np.abs(r))) for r in want]
    assert min(scales) >= 1e-3, (name, min(scales))
    T2 = [np.asarray(x) for t in c["tuples"] if t[0] == "E" for x in t[3:4]]
    assert all(x.max() <= 3 * x.min() for x in T2), name      # no single voxel sets the scale of a late record


def nvox_of(c):
    return int(np.prod(lp.grid_of_case(c)))


def test_case_table_covers_every_instantiation():
    named = {}
    for name, c in lp.CASES.items():
        for which in lp.SIDES:
            named.setdefault((lp.kernel_on(c, which), c["nsp"]), []).append(name)
    for kernel in lp.KERNELS:
        for nsp in lp.NSPS:
            if (kernel, nsp) in lp.UNREACHABLE:
                assert (kernel, nsp) not in named and lp.UNREACHABLE[(kernel, nsp)]
                continue
            cases = [lp.CASES[n] for n in named.get((kernel, nsp), [])]
            assert cases, (kernel, nsp)
            # a train past the deck (the odd kernel has none: past the other kernels' decks) on a grid with two full waves and a ragged third
            deck = lp.DECK.get(kernel, 16)
            assert any(c["kernel"] == lp.TRAIN and c["L"] > deck and nvox_of(c) > 128 and nvox_of(c) % 64 for c in cases), (kernel, nsp)
    assert all(("rows", nsp) in named for nsp in lp.NSPS)        # the default side: the rows variant below the threshold
    # the lists the issue names
    L = {c["L"] for c in lp.CASES.values() if c["kernel"] == lp.TRAIN}
    assert {17, 18, 21, 24} | {n + 1 for n in (3, 4, 7, 8, 14, 15)} <= L
    assert {nvox_of(c) for c in lp.CASES.values()} == {131, 128, 1, 143, 133}
    for name in lp.SUB_CASES:
        for vox0, nvox in lp.SUBRANGES:
            assert vox0 + nvox < nvox_of(lp.CASES[name])
    (a0, an), (b0, bn) = lp.SUBRANGES
    assert a0 % 64 and (a0 + an) % 64 and a0 // 64 != (a0 + an) // 64 and b0 == 64 and bn == 64
    for name, (small, big, kernel) in lp.THRESHOLD.items():
        c = lp.CASES[small]
        assert int(np.prod(big)) == lp.LANES_MIN_VOXELS - (kernel == "rows") and len(big) == len(lp.grid_of_case(c))
        assert all(64 % n for n in lp.grid_of_case(c))           # every lane position of every block sees every parameter set
        assert kernel == ("rows" if name == "thr_below" else lp.kernel_on(c, "odd")), name


@pytest.mark.parametrize("name", list(lp.CASES))
def test_claimed_index_spaces_are_the_plan_s(name):
    from epgpy_amd import functions as _functions
    from tests.signal_cases import ops_of, kn
    c = lp.CASES[name]
    enc, _, _ = _functions.compile_sequence(ops_of(c["tuples"]), shape=lp.grid_of_case(c), options={"max_nstate": 63}, fuse=c["fuse"])
    assert kn(len(enc.spaces)) == c["nsp"] and enc.grid == lp.grid_of_case(c), (name, enc.spaces)
    assert 32 < enc.peak + 1 <= 64, (name, enc.peak)              # a launch at 64 orders, above the 32 of the packed layout


def test_tiled_tuples_tile_every_parameter():
    small, big, _ = lp.THRESHOLD["thr_train"]
    tiled = lp.tiled_tuples(small, (22, 39))
    ref_small = lp.reference(small)
    from tests.signal_recurrence import signal_recurrence
    lp.check_tiling(signal_recurrence(tiled, max_nstate=63), ref_small)
    assert sum(1 for a, b in zip(tiled, tiled[1:]) if a is b) == 0 and len({id(t) for t in tiled}) == len({id(t) for t in lp.CASES[small]["tuples"]})


# ------------------------------------------------------------------------------------------------ the checks bite
def test_per_record_check_bites_where_close_does_not():
    """1e-9 of a late record"""
    from tests.test_gpu_parity import close
    name = "train_23_131"
    want, _ = reference(name)
    good = want.astype(np.complex128)
    lp.check_case("host", name, good, want)
    v = int(np.argmin(np.abs(want[-1])))
    size = float(np.abs(want[-1, v]))
    assert 0 < size <= 1e-3 and size >= 1e-3 * float(np.max(np.abs(want[-1]))), size       # a short-T2 voxel of the last echo
    bad = good.copy()
    bad[-1, v] *= 1 + 1e-9
    close(bad, good, 1e-12)
    with pytest.raises(AssertionError):
        lp.check_case("host", name, bad, want)
    lp.RATIO.pop("host", None)


def nearly_equal_columns():
    """the signals of train_20_131 with two pairs of voxels whose parameters differ in the thirteenth digit: 129 ~ 130 (both in
    the ragged last block) and 130 ~ 2 (block 2 and block 0)"""
    small = reference("train_20_131")[0].astype(np.complex128)
    small[:, 130] = small[:, 2] * (1 + 1e-13)
    small[:, 129] = small[:, 130] * (1 - 2e-13)
    return small


def test_tiling_check_bites_where_close_does_not():
    from tests.test_gpu_parity import close
    small = nearly_equal_columns()
    n = 131 * 3 + 7                                               # 400 voxels: six full blocks and a ragged one of 16
    good = small[:, np.arange(n) % 131]
    lp.check_tiling(good, small)
    swapped = good.copy()                                         # two columns of the ragged last block swapped
    a, b = 131 * 2 + 129, 131 * 2 + 130
    assert a // 64 == b // 64 == (n - 1) // 64 and n % 64
    swapped[:, [a, b]] = good[:, [b, a]]
    close(swapped, good, 1e-12)
    with pytest.raises(AssertionError):
        lp.check_tiling(swapped, small)
    slipped = good.copy()                                         # one column of block 2 taken from block 0
    slipped[:, 130] = good[:, 2]
    close(slipped, good, 1e-12)
    with pytest.raises(AssertionError):
        lp.check_tiling(slipped, small)


def test_subrange_check_bites_where_close_does_not():
    from tests.test_gpu_parity import close
    full = nearly_equal_columns()
    vox0, nvox = 64, 67                                           # block 1 and the ragged block 2
    good = np.full(full.shape, lp.PREFILL)
    good[:, vox0:vox0 + nvox] = full[:, vox0:vox0 + nvox]
    lp.check_subrange(good, full, vox0, nvox)
    swapped = good.copy()
    swapped[:, [129, 130]] = good[:, [130, 129]]
    close(swapped, good, 1e-12)
    with pytest.raises(AssertionError):
        lp.check_subrange(swapped, full, vox0, nvox)
    slipped = good.copy()
    slipped[:, 130] = full[:, 2]
    close(slipped, good, 1e-12)
    with pytest.raises(AssertionError):
        lp.check_subrange(slipped, full, vox0, nvox)
    spilled = good.copy()                                         # the store bound of a ragged block one lane too wide
    spilled[:, 0] = full[:, 0]
    with pytest.raises(AssertionError):
        lp.check_subrange(spilled, full, vox0, nvox)
    short = good.copy()                                           # ... and one lane too narrow
    short[:, 130] = lp.PREFILL
    with pytest.raises(AssertionError):
        lp.check_subrange(short, full, vox0, nvox)


def test_zero_records_must_be_exactly_zero():
    want, _ = reference("odd_lead_20_131")
    lp.check_case("host", "odd_lead_20_131", np.zeros(want.shape, dtype=np.complex128), want)
    bad = np.zeros(want.shape, dtype=np.complex128)
    bad[3, 130] = 1e-300
    with pytest.raises(AssertionError):
        lp.check_case("host", "odd_lead_20_131", bad, want)


def test_trace_check_reads_the_launcher_s_lines():
    fam = "[epgx] run: rows_grow_kernel<1> -- 64 orders from equilibrium, a good share of the records while the state matrix is short\n"
    recs = "[epgx] run: 3 records: [0, 1) at 16 orders per voxel, [1, 2) at 32, the rest at 64\n"
    train = "[epgx] run: variant lanes (one voxel per lane): L = 21, kernel train (deck 16), 15360 bytes of LDS per wave, 40 shifts before the last probe, body generic+echo-x/4\n"
    odd = ("[epgx] run: variant lanes-odd (one voxel per lane, odd orders only): L = 21, kernel rows_grow_lanes_kernel_odd (12 cells of 2 orders), "
           "state in 144 VGPRs, 0 bytes of LDS per wave, 40 shifts before the last probe\n")
    lp.check_trace(fam + recs + train, lp.TRAIN, 21, 1)
    lp.check_trace(fam + recs + odd, lp.ODD, 21, 1)
    for trace, kernel, L, nsp in ((fam + recs + train, lp.ANY, 21, 1), (fam + recs + train, lp.TRAIN, 20, 1), (fam + recs + train, lp.TRAIN, 21, 2),
                                  (fam + recs + odd, lp.TRAIN, 21, 1), (fam + recs, lp.TRAIN, 21, 1), (fam + recs + train + fam + recs + train, lp.TRAIN, 21, 1)):
        with pytest.raises(AssertionError):
            lp.check_trace(trace, kernel, L, nsp)
