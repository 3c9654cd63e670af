"""mifsk_frame_softbits (include/mifsk.h): what it refuses, it refuses before any HIP call, so every
code below comes back on a machine without a device.  The context is a block of zeroed host
memory and the device pointers are numbers: nothing looks into either before the call is refused."""
import ctypes as C

import pytest

import minimodem_amd as M
from _abi import EINVAL, ENOTSUP, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib


def test_the_python_name_is_public():
    assert "frame_softbits" in M.__all__ and callable(M.frame_softbits)


def _io(**kw):
    base = 1 << 20                                  # 16-byte aligned; never dereferenced
    io = _lib.SoftbitsIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = base, 96000, 96000, 2
    io.kind, io.rxnoise = _lib.FEED_F32, 0.0
    io.d_frames, io.d_nframes, io.frames_cap = base + (1 << 24), base + (1 << 25), 64
    io.d_mag, io.d_rawbits = base + (1 << 26), base + (1 << 27)
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx
    cfg = M.rx_config("1200")

    def rc(ctx=ctx, cfg=cfg, io=True, **kw):
        return lib.mifsk_frame_softbits(ctx, C.byref(cfg) if cfg is not None else None,
                                        C.byref(_io(**kw)) if io else None, None)

    assert rc(ctx=None) == EINVAL and rc(cfg=None) == EINVAL and rc(io=False) == EINVAL
    for name in ("d_samples", "d_frames", "d_nframes", "d_mag"):
        assert rc(**{name: None}) == EINVAL, name
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    assert rc(frames_cap=0) == EINVAL
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    assert rc(rxnoise=0.1) == EINVAL                                # float32 rows take no --Xrxnoise term
    assert rc(rxnoise=float("nan")) == EINVAL
    # 16-byte rows: the base, and a stride of whole vectors -- 4 floats, 8 PCM16 samples
    assert rc(d_samples=(1 << 20) + 8) == EINVAL and rc(d_samples=(1 << 20) + 4) == EINVAL
    assert rc(stream_stride=96002) == EINVAL and rc(stream_stride=95999) == EINVAL
    assert rc(kind=_lib.FEED_S16, stream_stride=96004) == EINVAL    # a multiple of 4, not of 8
    assert rc(kind=_lib.FEED_S16, d_samples=(1 << 20) + 8) == EINVAL
    # mifsk_check_cfg's verdict
    for field, v in (("expect_n_bits", 0), ("expect_n_bits", 65), ("bit_nsamples", 0), ("fftsize", 1)):
        bad = M.rx_config("1200")
        setattr(bad, field, v)
        assert rc(cfg=bad) == EINVAL, field
    # --auto-carrier: a frame's bands are its episode's
    assert rc(cfg=M.rx_config("1200", auto_carrier_threshold=0.001)) == ENOTSUP
    assert rc(cfg=M.rx_config("rtty", auto_carrier_threshold=0.5), kind=_lib.FEED_S16, rxnoise=0.1) == ENOTSUP
    # a stream's (frame, bit) cases are counted in 32 bits
    assert rc(frames_cap=(1 << 32) // 11 + 1) == EINVAL
    # the earlier checks win over the later ones
    auto = M.rx_config("1200", auto_carrier_threshold=0.001)
    assert rc(cfg=auto, ctx=None) == EINVAL
    assert rc(cfg=auto, d_mag=None) == EINVAL
    assert rc(cfg=auto, stream_stride=96002) == EINVAL
    assert rc(cfg=auto, kind=7) == EINVAL


def test_python_refuses_what_is_not_a_device_tensor():
    import numpy as np
    cfg = M.rx_config("1200")
    with pytest.raises((AssertionError, AttributeError)):
        M.frame_softbits(None, cfg, np.zeros((2, 64), np.float32), {"frames": None, "nframes": None})
