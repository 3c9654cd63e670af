"""mifsk_impair_batch and its host helper (include/mifsk.h): what the entry refuses --
before any HIP call, so every code below comes back on a machine without a device: the context is a
block of zeroed host memory and the device pointers are numbers."""
import ctypes as C

import numpy as np

import minimodem_amd as M
from minimodem_amd import _lib

import _impair as Im
from _abi import BASE, EINVAL, fake_ctx, ladder, lib  # noqa: F401


def test_the_python_names_are_public_and_the_kinds_are_the_restatements():
    assert (_lib.FEED_F32, _lib.FEED_S16) == (Im.F32K, Im.S16K)
    for name in ("ImpairIO", "impair", "snr_sigma"):
        assert name in M.__all__ and hasattr(M, name), name
    assert M.ImpairIO is _lib.ImpairIO


def _io(**kw):
    io = _lib.ImpairIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = BASE, 96000, 96000, 2
    io.kind = io.out_kind = _lib.FEED_F32
    io.d_out, io.out_stride = BASE + (1 << 24), 96000
    io.seed, io.first_stream, io.first_sample = 1, 0, 0
    io.gain, io.sigma, io.dc, io.flags = 1.0, 0.1, 0.0, 0
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx

    def rc(ctx=ctx, io=True, **kw):
        return lib.mifsk_impair_batch(ctx, C.byref(_io(**kw)) if io else None, None)

    # 1: a NULL ctx, io or d_out
    assert rc(ctx=None) == EINVAL and rc(io=False) == EINVAL and rc(d_out=None) == EINVAL
    # 2: the rows
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    # 3: either kind
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    assert rc(out_kind=2) == EINVAL and rc(out_kind=0xFFFFFFFF) == EINVAL
    # 4: flags
    assert rc(flags=1) == EINVAL and rc(flags=0x80000000) == EINVAL
    # 5: a piece begins at a block of the field
    for n in (1, 2, 3, 5, (1 << 40) + 2, (1 << 64) - 1):
        assert rc(first_sample=n) == EINVAL, n
    # 6: input rows of whole 16-byte vectors -- 4 floats, 8 PCM16 samples -- when there are input rows
    assert rc(d_samples=BASE + 8) == EINVAL and rc(d_samples=BASE + 4) == EINVAL
    assert rc(stream_stride=96002) == EINVAL and rc(stream_stride=95999) == EINVAL
    assert rc(kind=_lib.FEED_S16, stream_stride=96004) == EINVAL    # a multiple of 4, not of 8
    assert rc(kind=_lib.FEED_S16, d_samples=BASE + 8) == EINVAL
    # 7: output rows
    assert rc(d_out=BASE + 8) == EINVAL and rc(d_out=BASE + 2) == EINVAL
    assert rc(out_stride=0) == EINVAL
    assert rc(out_stride=96002) == EINVAL and rc(out_kind=_lib.FEED_S16, out_stride=96004) == EINVAL
    assert rc(out_stride=(1 << 32) - 4) == EINVAL and rc(out_stride=1 << 32) == EINVAL
    assert rc(out_stride=1 << 40) == EINVAL
    # noise rows: the input's base and stride are not looked at, the output's still are
    assert rc(d_samples=None, stream_stride=3, out_stride=96002) == EINVAL
    assert rc(d_samples=None, stream_stride=3, d_out=BASE + 4) == EINVAL
    # the earlier checks win over the later ones: with the output stride as the one late violation,
    # each earlier one alone still refuses, and so does every pair in the stated order
    ladder(rc, dict(out_stride=96002),
           [dict(d_out=None), dict(nstreams=0), dict(out_kind=9), dict(flags=2), dict(first_sample=2),
            dict(stream_stride=96001)])


def test_parameters_are_data_and_not_among_the_checks(lib, fake_ctx):
    """gain, sigma, dc, the seed and the stream index may hold anything: with the output stride as the one
    violation, the call comes back with that violation's code whatever they hold."""
    ctx, _keep = fake_ctx
    for v in (0.0, -1.0, float("inf"), float("nan"), 1e30):
        for name in ("gain", "sigma", "dc"):
            io = _io(out_stride=96002, **{name: v})
            assert lib.mifsk_impair_batch(ctx, C.byref(io), None) == EINVAL
    io = _io(out_stride=96002, seed=(1 << 64) - 1, first_stream=(1 << 64) - 1, first_sample=(1 << 64) - 4)
    assert lib.mifsk_impair_batch(ctx, C.byref(io), None) == EINVAL


def test_selftest_gauss_refuses_null_pointers(lib, fake_ctx):
    ctx, _keep = fake_ctx
    w, z = (C.c_uint32 * 2)(), (C.c_double * 2)()
    assert lib.mifsk_selftest_gauss(None, w, 1, z) == EINVAL
    assert lib.mifsk_selftest_gauss(ctx, None, 1, z) == EINVAL
    assert lib.mifsk_selftest_gauss(ctx, w, 1, None) == EINVAL
    assert lib.mifsk_selftest_gauss(ctx, w, (1 << 30) + 1, z) == EINVAL


def test_impair_sigma_is_the_formula(lib):
    """(float)sqrt((a a / 2) / 10^(snr_db / 10)) in double: numpy's float64 evaluation rounded to float32, one
    float32 step allowed for a pow() that differs in its last place."""
    for a in (0.5, 1.0, 0.3):
        for snr in (20.0, 12.0, 6.0, 0.0):
            a32 = float(np.float32(a))
            want = np.float32(np.sqrt((a32 * a32 / 2.0) / 10.0 ** (snr / 10.0)))
            got = np.float32(lib.mifsk_impair_sigma(a, snr))
            assert abs(int(got.view(np.uint32)) - int(want.view(np.uint32))) <= 1, (a, snr, got, want)
            assert M.snr_sigma(a, snr) == float(got)
    # amplitude 0.5 (bench.py's and tools/same_snr_sweep.py's): p_sig = 0.125
    assert abs(M.snr_sigma(0.5, 0.0) - np.sqrt(0.125)) < 1e-7
    assert abs(M.snr_sigma(0.5, 20.0) - np.sqrt(0.125) / 10.0) < 1e-8
    assert M.snr_sigma(0.5, float("inf")) == 0.0
