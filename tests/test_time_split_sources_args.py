"""The time split's entries for PCM16, host memory and WAV files (mifsk_demod_long_batch_s16,
mifsk_demod_long_batch_host, mifsk_demod_files_long): what they refuse, they refuse before any HIP
call, so every code below comes back on a machine without a device.  Where a check lies behind the
NULL-context check the context is a block of zeroed host memory: nothing looks into it before the
call is refused."""
import ctypes as C

import pytest

import minimodem_amd as M
from _abi import EINVAL, ENOTSUP, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib


def _params(flags=0, chunk=0, warmup=0):
    p = _lib.TimeSplit()
    p.chunk, p.warmup, p.flags = chunk, warmup, flags
    return p


def test_pcm16_entry_argument_checks_in_order(lib, fake_ctx):
    ctx, _keep = fake_ctx
    cfg = M.rx_config("1200")
    io = _lib.DemodIO()
    io.nstreams = 2
    base = 1 << 20                                  # 16-byte aligned; never dereferenced

    def rc(ctx=ctx, cfg=cfg, ptr=base, stride=96000, lens=(5000, 5000), nstreams=2, io=io, params=None):
        arr = (C.c_uint64 * max(1, len(lens)))(*lens) if lens is not None else None
        return lib.mifsk_demod_long_batch_s16(
            ctx, C.byref(cfg) if cfg is not None else None, C.c_void_p(ptr), stride, arr, nstreams,
            C.c_float(0.0), C.byref(params) if params is not None else None,
            C.byref(io) if io is not None else None, None, None)

    assert rc(ctx=None) == EINVAL
    assert rc(cfg=None) == EINVAL
    assert rc(io=None) == EINVAL
    assert rc(lens=None) == EINVAL
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-3) == EINVAL
    assert rc(ptr=base + 8) == EINVAL               # 8-byte aligned is not enough for the base
    assert rc(stride=96004) == EINVAL               # a multiple of 4, not of 8
    assert rc(stride=95999) == EINVAL
    assert rc(lens=(96001, 5000)) == EINVAL         # a stream longer than its row
    assert rc(lens=(5000, 96008)) == EINVAL
    # ... then the planner's codes
    assert rc(params=_params(flags=_lib.IO_RING_EXACT)) == ENOTSUP
    assert rc(params=_params(flags=_lib.IO_ENGINE_WAVE | _lib.IO_ENGINE_WORKGROUP)) == EINVAL
    assert rc(params=_params(warmup=cfg.samplebuf_size)) == EINVAL          # below 2 * samplebuf_size
    assert rc(params=_params(chunk=cfg.samplebuf_size // 2 + 1)) == EINVAL   # off the lattice
    # the earlier checks win over the later ones
    assert rc(ctx=None, params=_params(flags=_lib.IO_RING_EXACT)) == EINVAL
    assert rc(stride=96004, params=_params(flags=_lib.IO_RING_EXACT)) == EINVAL
    assert rc(lens=(96001, 5000), params=_params(flags=_lib.IO_RING_EXACT)) == EINVAL


def test_host_entry_argument_checks(lib, fake_ctx):
    import numpy as np
    ctx, _keep = fake_ctx
    cfg = M.rx_config("1200")
    io = _lib.DemodIO()
    io.nstreams = 1
    x = np.zeros(1000, np.int16)

    def rc(ctx=ctx, rows=(x.ctypes.data,), lens=(1000,), nstreams=1, src_flags=_lib.IO_HOST_S16, params=None,
           io=io):
        r = (C.c_void_p * max(1, len(rows)))(*rows) if rows is not None else None
        arr = (C.c_uint64 * max(1, len(lens)))(*lens) if lens is not None else None
        return lib.mifsk_demod_long_batch_host(ctx, C.byref(cfg), r, arr, nstreams, src_flags, C.c_float(0.0),
                                               C.byref(params) if params is not None else None,
                                               C.byref(io) if io is not None else None, None, None)

    assert rc(ctx=None) == EINVAL
    assert rc(rows=None) == EINVAL and rc(lens=None) == EINVAL and rc(io=None) == EINVAL
    assert rc(nstreams=0) == EINVAL
    assert rc(src_flags=_lib.IO_RING_EXACT) == EINVAL           # only 0 or MIFSK_IO_HOST_S16
    assert rc(rows=(None,)) == EINVAL                           # samples, but no pointer to them
    assert rc(params=_params(flags=_lib.IO_RING_EXACT)) == ENOTSUP
    assert rc(params=_params(warmup=7)) == EINVAL


def test_files_long_argument_checks(lib, fake_ctx, tmp_path):
    ctx, _keep = fake_ctx
    a = _lib.ModemArgs()
    lib.mifsk_modem_args_default(C.byref(a))
    a.baudmode = b"1200"
    missing = str(tmp_path / "never_opened.wav").encode()
    paths = (C.c_char_p * 1)(missing)

    def rc(ctx=ctx, args=a, paths=paths, nfiles=1, flags=0, params=None, out=True):
        h = C.c_void_p()
        r = lib.mifsk_demod_files_long(ctx, C.byref(args) if args is not None else None, paths, nfiles,
                                       C.c_float(0.0), flags, C.byref(params) if params is not None else None,
                                       C.byref(h) if out else None)
        assert not h                               # a refused call makes no object
        return r

    assert rc(flags=_lib.IO_RING_EXACT) == ENOTSUP
    assert rc(params=_params(flags=_lib.IO_RING_EXACT)) == ENOTSUP
    assert rc(ctx=None) == EINVAL and rc(args=None) == EINVAL and rc(out=False) == EINVAL
    assert rc(nfiles=-1) == EINVAL
    assert rc(paths=None, nfiles=1) == EINVAL
    assert rc(ctx=None, flags=_lib.IO_RING_EXACT) == EINVAL
    assert lib.mifsk_files_time_split(None, 0) is None or not lib.mifsk_files_time_split(None, 0)


def test_python_refuses_time_split_with_ring_exact():
    for ts in (True, {"chunk": 48000}):
        with pytest.raises(ValueError):
            M.demod_files(None, ["x.wav"], ring_exact=True, time_split=ts)
