"""CPU: the tiled path for state matrices above the capacity classes -- its operator-level schedule (blocks of at most
H shift units, shifts by more than H on their own, tiles that follow the populated top), its buffer size, and which
plans simulate() sends there.  No GPU needed."""
import numpy as np
import pytest

import epgpy_amd as epg
from epgpy_amd import _lib, functions

H, W = _lib.TILED_H, _lib.TILED_W


def plan(ops, **options):
    return functions.compile_sequence(ops, options=options)[0]


def shifts_of(enc):
    return [abs(rec[2]) if rec[0] == _lib.OP_S else 0 for rec in enc.records]


def test_tile_geometry():
    assert (_lib.TILED_M, _lib.TILED_H, _lib.TILED_W) == (8, 32, 448)


def test_blocks_bound_the_shift_units():
    enc = plan([epg.T(30, 0)] + [epg.S(1), epg.T(60, 90), epg.ADC] * 3000)
    blocks = enc.tiled_blocks()
    units = shifts_of(enc)
    assert blocks[0][0] == 0 and blocks[-1][1] == len(enc.records)
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))       # contiguous, every operator once
    for b0, b1, _ in blocks:
        assert 0 < sum(units[b0:b1]) <= H
    assert len(blocks) == -(-3000 // H)


def test_tiles_follow_the_populated_top():
    enc = plan([epg.T(90, 90)] + [epg.S(1), epg.T(30, 0), epg.ADC] * 2100)
    blocks = enc.tiled_blocks()
    top = 0
    units = shifts_of(enc)
    for b0, b1, tiles in blocks:
        top += sum(units[b0:b1])
        assert tiles == top // W + 1
    assert blocks[0][2] == 1 and blocks[-1][2] == 2100 // W + 1
    assert enc.tiled_capacity() == 2112


def test_shifts_beyond_the_halo_are_blocks_of_their_own():
    seq = [epg.T(90, 90), epg.S(2), epg.S(-1), epg.T(120, 0), epg.S(300), epg.ADC, epg.S(1), epg.ADC]
    enc = plan(seq)
    blocks = enc.tiled_blocks()
    big = [i for i, rec in enumerate(enc.records) if rec[0] == _lib.OP_S and abs(rec[2]) > H]
    assert len(big) == 1
    assert (big[0], big[0] + 1) in [(b0, b1) for b0, b1, _ in blocks]
    assert blocks[-1][2] == 303 // W + 1
    # the same rule at another halo: a shift by 2 no longer fits a block with one unit left
    small = enc.tiled_blocks(H=2)
    assert all(sum(shifts_of(enc)[b0:b1]) <= 2 or b1 - b0 == 1 for b0, b1, _ in small)


def test_truncation_lowers_the_top():
    seq = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.ADC] * 3000
    assert plan(seq).tiled_capacity() == 3008
    assert plan(seq, max_nstate=2500).tiled_capacity() == 2560
    capped = plan(seq, max_nstate=2500).tiled_blocks()
    assert max(t for _, _, t in capped) == 2500 // W + 1
    nmax = [epg.T(90, 90)] + [epg.S(1, nmax=1500), epg.T(150, 0), epg.ADC] * 2000
    assert plan(nmax).tiled_capacity() == 1536
    # a reset drops the top to 0: the tiles of later blocks shrink to what the buffers still hold
    reset = plan([epg.T(90, 90)] + [epg.S(1), epg.ADC] * 1200 + [epg.RESET] + [epg.T(90, 90), epg.S(1), epg.ADC] * 100)
    tiles = [t for _, _, t in reset.tiled_blocks()]
    assert max(tiles) == 1200 // W + 1 and tiles[-1] >= 1


def test_adc_positions_stay_in_order():
    seq = [epg.T(90, 90)] + [epg.S(1), epg.T(150, 0), epg.ADC] * 1500
    enc = plan(seq)
    adc = [i for i, rec in enumerate(enc.records) if rec[0] == _lib.OP_ADC]
    assert [enc.records[i][2] for i in adc] == list(range(1500))
    owner = [next(j for j, (b0, b1, _) in enumerate(enc.tiled_blocks()) if b0 <= i < b1) for i in adc]
    assert owner == sorted(owner)


def test_start_state_counts_as_populated():
    enc = functions.compile_sequence([epg.S(1)] * 2000 + [epg.ADC], nstate0=700, dense_start=True)[0]
    assert enc.tiled_capacity() == 2752
    assert enc.tiled_capacity(top0=1023) == 3072
    assert enc.tiled_blocks(top0=1023)[0][2] == 1023 // W + 1


# ------------------------------------------------------------------ which plans take the tiled path
def test_capacity_classes_unchanged():
    assert plan([epg.T(90, 90)] + [epg.S(1), epg.ADC] * 1023).capacity() == 1024
    assert plan([epg.T(90, 90)] + [epg.S(1), epg.ADC] * 2047).capacity(resident=True) == 2048
    long = plan([epg.S(1)] * 3000 + [epg.ADC])
    with pytest.raises(NotImplementedError):
        long.capacity()
    with pytest.raises(NotImplementedError):
        long.capacity(resident=True)
    assert long.tiled_ok()
    assert long.tiled_capacity() == 3008
    assert len(long.tiled_blocks()) == -(-3000 // H)


def test_plans_the_tiled_path_does_not_take():
    T1, T2 = np.array([800.0, 1200.0]), np.array([60.0, 90.0])
    jac = [epg.T(90, 90)] + [epg.S(1), epg.E(5, T1, T2, order1=True), epg.ADC] * 1100
    enc = functions.compile_sequence(jac, variables=["T2"])[0]
    assert not enc.tiled_ok()
    nd = plan([epg.T(90, 90)] + [epg.S([1, 1]), epg.ADC] * 1100)
    assert not nd.tiled_ok()
    ex = plan([epg.T(90, 90), epg.X(5, 0.01, T1=[800, 1000], T2=[40, 80], axis=0), epg.ADC] + [epg.S(1)] * 1100 + [epg.ADC])
    assert not ex.tiled_ok()


def _route(monkeypatch, seq, **kw):
    """simulate() up to its choice of path (no device is touched before it): 'tiled', or the exception raised"""
    def tiled(*args, **kwargs):
        raise _Tiled()

    monkeypatch.setattr(functions, "_simulate_tiled", tiled)
    monkeypatch.setattr(_lib, "default_device", lambda: 0)
    try:
        epg.simulate(seq, **kw)
    except _Tiled:
        return "tiled"
    except NotImplementedError:
        return "NotImplementedError"
    except Exception as exc:   # pragma: no cover - reached a device call: not the tiled path
        return type(exc).__name__
    return "ran"


class _Tiled(Exception):
    pass


def test_simulate_routes_long_plans(monkeypatch):
    train = [epg.T(90, 90)] + [epg.S(1), epg.T(30, 0), epg.ADC] * 2100     # (up to 2047 orders: the 2048-order kernel)
    assert _route(monkeypatch, [epg.S(1)] * 3000 + [epg.ADC]) == "tiled"
    assert _route(monkeypatch, train) == "tiled"
    assert _route(monkeypatch, train, mode="resident") == "tiled"
    assert _route(monkeypatch, train, mode="stream") == "NotImplementedError"
    assert _route(monkeypatch, train, ngpu=2) == "NotImplementedError"
    assert _route(monkeypatch, [epg.T(90, 90)] + [epg.S([1, 0]), epg.T(30, 0), epg.ADC] * 1100) == "NotImplementedError"
    T2 = np.array([60.0, 90.0])
    jac = [epg.T(90, 90)] + [epg.S(1), epg.E(5, 1000, T2, order1=True), epg.ADC] * 1100
    assert _route(monkeypatch, jac, probe=epg.Jacobian(["T2"])) == "NotImplementedError"
