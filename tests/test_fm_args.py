"""mifsk_fm_demod_batch, mifsk_fm_modulate_batch and their host helpers (include/mifsk.h): what
the entries refuse -- before any HIP call, so every code below comes back on a machine without a device:
the context is a block of zeroed host memory and the device pointers are numbers."""
import ctypes as C

import numpy as np

import minimodem_amd as M
from minimodem_amd import _lib

import _fm as Fm
from _abi import BASE, EINVAL, fake_ctx, ladder, lib  # noqa: F401


def test_the_python_names_are_public_and_the_kinds_are_the_restatements():
    assert (_lib.FEED_F32, _lib.FEED_S16) == (Fm.F32K, Fm.S16K)
    for name in ("FmDemodIO", "FmModIO", "fm_demod", "fm_modulate", "fm_gain", "fm_step"):
        assert name in M.__all__ and hasattr(M, name), name
    assert M.FmDemodIO is _lib.FmDemodIO and M.FmModIO is _lib.FmModIO and hasattr(M.Context, "selftest_turn")


def _demod_io(**kw):
    io = _lib.FmDemodIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = BASE, 96000, 96000, 2
    io.kind, io.flags = _lib.FEED_F32, 0
    io.d_out, io.out_stride = BASE + (1 << 24), 96000
    io.gain = 16.0
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _mod_io(**kw):
    io = _lib.FmModIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = BASE, 96000, 96000, 2
    io.out_kind, io.flags = _lib.FEED_F32, 0
    io.d_out, io.out_stride = BASE + (1 << 24), 96000
    io.deviation, io.centre, io.amplitude = 0.0625, 0.0, 1.0
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_the_discriminators_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx

    def rc(ctx=ctx, io=True, **kw):
        return lib.mifsk_fm_demod_batch(ctx, C.byref(_demod_io(**kw)) if io else None, None)

    # 1: a NULL ctx, io, d_samples or d_out
    assert rc(ctx=None) == EINVAL and rc(io=False) == EINVAL
    assert rc(d_samples=None) == EINVAL and rc(d_out=None) == EINVAL
    # 2: the rows
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    # 3: the kind
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    # 4: flags
    assert rc(flags=1) == EINVAL and rc(flags=0x80000000) == EINVAL
    # 5: the input base
    assert rc(d_samples=BASE + 8) == EINVAL and rc(d_samples=BASE + 4) == EINVAL
    assert rc(kind=_lib.FEED_S16, d_samples=BASE + 8) == EINVAL
    # 6: input rows of whole 16-byte vectors of complex elements: 2 of float32, 4 of PCM16
    assert rc(stream_stride=96001) == EINVAL and rc(stream_stride=95999) == EINVAL
    assert rc(kind=_lib.FEED_S16, stream_stride=96002) == EINVAL    # a multiple of 2, not of 4
    assert rc(kind=_lib.FEED_S16, stream_stride=96001) == EINVAL
    # 7: the output base
    assert rc(d_out=BASE + 8) == EINVAL and rc(d_out=BASE + 2) == EINVAL
    # 8: the output stride
    assert rc(out_stride=0) == EINVAL
    assert rc(out_stride=96002) == EINVAL and rc(out_stride=95999) == EINVAL
    assert rc(out_stride=(1 << 32) - 4) == EINVAL and rc(out_stride=1 << 32) == EINVAL
    assert rc(out_stride=1 << 40) == EINVAL
    ladder(rc, dict(out_stride=96002),
           [dict(d_samples=None), dict(nstreams=0), dict(kind=9), dict(flags=2), dict(d_samples=BASE + 8),
            dict(stream_stride=96001), dict(d_out=BASE + 4)])
    # gain, d_prev and d_last are data and not among the checks
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert rc(out_stride=96002, gain=v) == EINVAL
    assert rc(out_stride=96002, d_prev=BASE + 4, d_last=BASE + 12) == EINVAL


def test_the_modulators_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx

    def rc(ctx=ctx, io=True, **kw):
        return lib.mifsk_fm_modulate_batch(ctx, C.byref(_mod_io(**kw)) if io else None, None)

    # 1: a NULL ctx, io, d_samples or d_out
    assert rc(ctx=None) == EINVAL and rc(io=False) == EINVAL
    assert rc(d_samples=None) == EINVAL and rc(d_out=None) == EINVAL
    # 2: the rows
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    # 3: the output's kind
    assert rc(out_kind=2) == EINVAL and rc(out_kind=0xFFFFFFFF) == EINVAL
    # 4: flags
    assert rc(flags=1) == EINVAL and rc(flags=0x80000000) == EINVAL
    # 5: the input base
    assert rc(d_samples=BASE + 8) == EINVAL and rc(d_samples=BASE + 4) == EINVAL
    # 6: input rows of whole 16-byte vectors: 4 floats
    assert rc(stream_stride=96002) == EINVAL and rc(stream_stride=95999) == EINVAL
    # 7: the output base
    assert rc(d_out=BASE + 8) == EINVAL and rc(d_out=BASE + 2) == EINVAL
    # 8: output rows of whole 16-byte vectors of complex elements: 2 of float32, 4 of PCM16
    assert rc(out_stride=0) == EINVAL
    assert rc(out_stride=96001) == EINVAL and rc(out_kind=_lib.FEED_S16, out_stride=96002) == EINVAL
    assert rc(out_stride=(1 << 32) - 6) == EINVAL and rc(out_stride=1 << 32) == EINVAL
    assert rc(out_stride=1 << 40) == EINVAL
    ladder(rc, dict(out_stride=96001),
           [dict(d_out=None), dict(nstreams=0), dict(out_kind=9), dict(flags=2), dict(d_samples=BASE + 8),
            dict(stream_stride=96002), dict(d_out=BASE + 4)])
    # deviation, centre, amplitude and the phase arrays are data and not among the checks
    for v in (0.0, -1.0, float("inf"), float("nan"), 1e30):
        for name in ("deviation", "centre", "amplitude"):
            assert rc(out_stride=96001, **{name: v}) == EINVAL
    assert rc(out_stride=96001, d_phase0=BASE + 4, d_phase_out=BASE + 4) == EINVAL


def test_selftest_turn_refuses_null_pointers(lib, fake_ctx):
    ctx, _keep = fake_ctx
    y, x, out = (C.c_double * 1)(), (C.c_double * 1)(), (C.c_double * 1)()
    assert lib.mifsk_selftest_turn(None, y, x, 1, out) == EINVAL
    assert lib.mifsk_selftest_turn(ctx, None, x, 1, out) == EINVAL
    assert lib.mifsk_selftest_turn(ctx, y, None, 1, out) == EINVAL
    assert lib.mifsk_selftest_turn(ctx, y, x, 1, None) == EINVAL
    assert lib.mifsk_selftest_turn(ctx, y, x, (1 << 30) + 1, out) == EINVAL


def test_fm_gain_and_fm_step_are_the_quotients(lib):
    assert M.fm_gain(48000.0, 3000.0) == 16.0 and M.fm_step(3000.0, 48000.0) == 0.0625
    assert M.fm_gain(48000.0, 5000.0) == float(np.float32(48000.0 / 5000.0))
    assert M.fm_step(5000.0, 44100.0) == 5000.0 / 44100.0
    assert M.fm_step(-1700.0, 48000.0) == -1700.0 / 48000.0
    assert lib.mifsk_fm_gain(22050.0, 2500.0) == float(np.float32(22050.0 / 2500.0))
    assert lib.mifsk_fm_step(0.0, 48000.0) == 0.0 and M.fm_gain(48000.0, 0.0) == float("inf")
