"""`simulate(..., probe=Hessian, mode="resident", out="device")`: the DeviceHessian handle on the passes' shared signal buffer.
(The gradient form of stats.crlb on device handles is not part of the library yet: crlb(J_dev, H=...) keeps raising.)"""
import numpy as np
import pytest

from epgpy_amd import epg, stats
from epgpy_amd import functions as _functions
from tests import sequences as sq

pytestmark = pytest.mark.gpu


def grid_case():
    return next(c for c in sq.hessian_cases(epg) if c[0] == "grid")


def test_device_hessian_equals_the_host_result():
    _, seq, probes, opts = grid_case()
    host = epg.simulate(seq, probe=probes, mode="resident", **opts)
    dev = epg.simulate(seq, probe=probes, mode="resident", out="device", **opts)
    assert len(dev) == len(probes) == 2
    for pb, h, want in zip(probes, dev, host):
        assert isinstance(h, _functions.DeviceHessian)
        assert h.shape == want.shape == (3, 2, 3, len(pb.variables1), len(pb.variables2)) and len(h) == 3
        assert h.variables1 == pb.variables1 and h.variables2 == pb.variables2 and h.grid == (2, 3) and h.nrec == 3
        assert h.row_stride == h.nvox == 6 and h.dtype == np.complex128 and h.ptr
        assert h.offsets.shape == h.record_strides.shape == (len(pb.variables1), len(pb.variables2))
        # an entry lives in the pass of its pair: three rows per record for a diagonal pair, four otherwise, per probe position
        for i1, v1 in enumerate(pb.variables1):
            for i2, v2 in enumerate(pb.variables2):
                if "magnitude" not in (v1, v2):
                    assert h.record_strides[i1, i2] == len(probes) * (3 if v1 == v2 else 4) * h.nvox and h.offsets[i1, i2] >= 0
        assert np.array_equal(h.offsets, np.swapaxes(h.offsets, 0, 1)) or pb.variables1 != pb.variables2     # symmetric pairs: one pass
        assert np.array_equal(np.asarray(h), want)                      # bit for bit: the same rows, downloaded


def test_device_hessian_refusals():
    _, seq, probes, opts = grid_case()
    with pytest.raises(NotImplementedError, match="ngpu"):
        epg.simulate(seq, probe=probes, mode="resident", out="device", ngpu=2, **opts)
    with pytest.raises(NotImplementedError, match="init"):
        epg.simulate(seq, probe=probes, mode="resident", out="device", init=[0, 0, 1], **opts)
    with pytest.raises(NotImplementedError, match="complex128"):
        epg.simulate(seq, probe=probes, mode="resident", out="device", dtype=np.complex64, **opts)
    with pytest.raises(NotImplementedError, match="every probe of the list is a Hessian"):
        epg.simulate(seq, probe=[probes[0], epg.Jacobian(["T2"])], mode="resident", out="device", **opts)
    with pytest.raises(ValueError):                                    # the operator-by-operator path has no device records
        epg.simulate(seq, probe=probes, out="device", **opts)


def test_crlb_on_device_handles_still_needs_a_host_hessian():
    """the gradient on the device did not ship: a device Jacobian with any H raises, as before"""
    rf = epg.T(150.0, 0.0, order1={"fa": {"alpha": 1.0}}, order2=[("fa", "fa"), ("T2", "fa")])
    rl = epg.E(5.0, 1000.0, np.linspace(40.0, 90.0, 5), order1="T2", order2=[("T2", "T2"), ("T2", "fa")])
    seq = [epg.T(90.0, 90.0)] + [epg.S(1), rl, rf, epg.S(1), rl, epg.ADC] * 6
    J_dev = epg.simulate(seq, probe=epg.Jacobian(["T2"]), out="device")
    H_dev, = [epg.simulate(seq, probe=epg.Hessian(["T2"], ["fa"]), mode="resident", out="device")]
    assert np.asarray(H_dev).shape == (6, 5, 1, 1)
    with pytest.raises(NotImplementedError):
        stats.crlb(J_dev, H=H_dev)
