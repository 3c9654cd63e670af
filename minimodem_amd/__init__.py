"""minimodem_amd -- MI355X-native batched FSK demodulator behind minimodem's
fsk.h API.

The signal path lives in libmifsk.so (hand-written HIP for gfx950, C ABI in
include/fsk.h + include/mifsk.h).  This package is the thin host-side mirror
used by the tests, the benchmark and Python callers: it marshals arguments,
uses PyTorch only for device memory / streams / torch.distributed, and raises
if the native library is missing -- there is no fallback implementation.
"""
import collections
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from ._lib import ModemArgs, RxConfig  # noqa: F401
from ._lib import MUX_COMPLEX, MuxIO, MuxParams  # noqa: F401
from ._lib import ImpairIO  # noqa: F401
from ._lib import FmDemodIO, FmModIO  # noqa: F401
from ._lib import FmSquelchIO  # noqa: F401

__all__ = ["build", "rx_config", "Context", "demod_batch", "frame_softbits", "find_frame_batch",
           "LegacyPlan", "synthesize", "FRAME_DTYPE", "EPISODE_DTYPE",
           "gather_bytes", "shard_range", "carrier_survey", "carrier_windows", "carrier_tones",
           "channel_taps", "ChannelPlan", "channelize", "ChannelStream", "channel_stream_outputs",
           "MUX_COMPLEX", "MuxParams", "MuxIO", "MuxPlan", "multiplex", "mux_table",
           "ImpairIO", "impair", "snr_sigma",
           "FmDemodIO", "FmModIO", "fm_demod", "fm_modulate", "fm_gain", "fm_step",
           "FmSquelchIO", "fm_squelch", "squelch_level"]

_HERE = os.path.dirname(os.path.abspath(__file__))

FRAME_DTYPE = np.dtype([("bits", "<u8"), ("start", "<u8"), ("confidence", "<f4"),
                        ("amplitude", "<f4"), ("flags", "<u4"), ("reserved", "<u4")])
EPISODE_DTYPE = np.dtype([("carrier_nsamples", "<u8"), ("first_frame", "<u4"),
                          ("nframes", "<u4"), ("confidence_total", "<f4"),
                          ("amplitude_total", "<f4"), ("end_reason", "<u4"),
                          ("b_mark", "<u4")])
SEARCH_DTYPE = np.dtype([("sample_offset", "<u8"), ("navail", "<u4"), ("try_first", "<u4"),
                         ("try_max", "<u4"), ("try_step", "<u4"), ("search_limit", "<f4"),
                         ("use_sync_string", "<u4")])
RESULT_DTYPE = np.dtype([("bits", "<u8"), ("confidence", "<f4"), ("amplitude", "<f4"),
                         ("frame_start", "<u4"), ("n_positions", "<u4")])
assert SEARCH_DTYPE.itemsize == 32 and RESULT_DTYPE.itemsize == 24
NCOUNTERS = 32
COUNTER_NAMES = {0: "iterations", 1: "batches", 2: "stages", 3: "bulk_frames", 4: "refines",
                 5: "cache_hits", 6: "positions", 7: "lattice_batches", 8: "cyc_total",
                 9: "cyc_scan", 10: "cyc_wait", 11: "cyc_confidence", 12: "cyc_bulk", 13: "w_stage", 14: "w_correlate",
                 15: "w_barrier", 16: "cyc_general", 17: "cyc_restart", 18: "cyc_scan1", 19: "cyc_scan2", 20: "cyc_replay_scan", 21: "cyc_scan_wait",
                 24: "conf_fallbacks", 25: "seg_second_looks"}


def build(force=False):
    """Compile libmifsk.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force and os.path.exists(_lib.LIB_PATH):
        os.unlink(_lib.LIB_PATH)
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True)
    return _lib.LIB_PATH


def rx_config(baudmode="1200", **opts):
    """The --rx command line as a derived configuration
    (mifsk_rx_config_init; reference src/minimodem.c:819-965,1037-1131)."""
    lib = _lib.load()
    a = ModemArgs()
    lib.mifsk_modem_args_default(C.byref(a))
    a.baudmode = str(baudmode).encode()
    if "sync_byte" in opts:
        a.have_sync_byte = 1
    for k, v in opts.items():
        if not hasattr(a, k):
            raise TypeError("unknown modem option %r" % k)
        setattr(a, k, v)
    cfg = RxConfig()
    rc = lib.mifsk_rx_config_init(C.byref(cfg), C.byref(a))
    if rc != 0:
        raise ValueError("mifsk_rx_config_init failed: %d" % rc)
    cfg._keepalive = a
    return cfg


class _Handle:
    """A library handle that is destroyed once: `handle`, close() and __del__.  A subclass names the
    library's destroy function and sets `_lib` and `handle` when it has made one."""
    handle = None
    _destroy = None

    def close(self):
        if self.handle:
            getattr(self._lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """A device context (twiddle tables etc.); one per process/GPU."""
    _destroy = "mifsk_ctx_destroy"

    def __init__(self, device=-1):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.mifsk_ctx_create(C.byref(h), int(device))
        if rc != 0:
            raise RuntimeError("mifsk_ctx_create failed: %d (no gfx950 HIP device? "
                               "this package has no CPU path)" % rc)
        self.handle = h

    @property
    def device_name(self):
        return self._lib.mifsk_ctx_device_name(self.handle).decode()

    def selftest_sqrt(self, nvalues, seed=1):
        """mifsk_selftest_sqrt: the kernels' short square root against the exact sequence on
        `nvalues` sums of squares -> (accepted and differing [must be 0], sent to the exact
        sequence by the guard, differing without the guard, evaluated)."""
        counts = (C.c_uint64 * 4)()
        rc = self._lib.mifsk_selftest_sqrt(self.handle, int(seed), int(nvalues), counts)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_sqrt failed: %d" % rc)
        return tuple(int(c) for c in counts)

    def selftest_rcp(self, c, x):
        """mifsk_selftest_rcp: float arrays c, x -> (the device's double reciprocal of c, the
        quotient x / c it makes with it)."""
        c = np.ascontiguousarray(c, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        assert c.shape == x.shape and c.ndim == 1
        rc_out, q = np.empty(c.shape, np.float64), np.empty(c.shape, np.float32)
        rc = self._lib.mifsk_selftest_rcp(self.handle, c.ctypes.data, x.ctypes.data, c.size,
                                          rc_out.ctypes.data, q.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_rcp failed: %d" % rc)
        return rc_out, q

    def selftest_gauss(self, words):
        """mifsk_selftest_gauss: uint32 words [n, 2] -> float64 [n, 2], the device's R(w[0]) C(w[1]) and
        R(w[0]) S(w[1]) of the channel model's noise field."""
        words = np.ascontiguousarray(words, np.uint32)
        assert words.ndim == 2 and words.shape[1] == 2
        z = np.empty(words.shape, np.float64)
        rc = self._lib.mifsk_selftest_gauss(self.handle, words.ctypes.data, words.shape[0], z.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_gauss failed: %d" % rc)
        return z

    def selftest_turn(self, y, x):
        """mifsk_selftest_turn: float64 arrays y, x [n] -> float64 [n], the device's mifsk_turn(y, x) of the
        FM stage: the angle of x + i y in turns."""
        y = np.ascontiguousarray(y, np.float64)
        x = np.ascontiguousarray(x, np.float64)
        assert y.shape == x.shape and y.ndim == 1
        out = np.empty(y.shape, np.float64)
        rc = self._lib.mifsk_selftest_turn(self.handle, y.ctypes.data, x.ctypes.data, y.size, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_turn failed: %d" % rc)
        return out

    def selftest_mag(self, re, im, scalar=1.0):
        """mifsk_selftest_mag: double arrays re, im -> (sqrt_sumsq(s), sqrt_newton1(s)'s g, its
        `unsafe` flag, band_mag(re, im, scalar)) with s as band_mag builds it."""
        re = np.ascontiguousarray(re, np.float64)
        im = np.ascontiguousarray(im, np.float64)
        assert re.shape == im.shape and re.ndim == 1
        root, g = np.empty(re.shape, np.float64), np.empty(re.shape, np.float64)
        unsafe, mag = np.empty(re.shape, np.uint8), np.empty(re.shape, np.float32)
        rc = self._lib.mifsk_selftest_mag(self.handle, re.ctypes.data, im.ctypes.data, float(scalar),
                                          re.size, root.ctypes.data, g.ctypes.data,
                                          unsafe.ctypes.data, mag.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_mag failed: %d" % rc)
        return root, g, unsafe, mag

    def selftest_confidence(self, variant, mags, req_mask=0, req_val=0):
        """mifsk_selftest_confidence: mags[ncases, n_bits, 2] = (mark, space) magnitudes ->
        (conf, ampl, bits, fell_back) per case; case i runs on lane i % 64 of wave i / 64.
        variant 0: frame_confidence, 1: frame_confidence_any, 2: frame_confidence_any_staged."""
        mags = np.ascontiguousarray(mags, np.float32)
        assert mags.ndim == 3 and mags.shape[2] == 2
        n = mags.shape[0]
        conf, ampl = np.empty(n, np.float32), np.empty(n, np.float32)
        bits, fb = np.empty(n, np.uint64), np.empty(n, np.uint32)
        rc = self._lib.mifsk_selftest_confidence(self.handle, int(variant), mags.shape[1],
                                                 int(req_mask), int(req_val), mags.ctypes.data, n,
                                                 conf.ctypes.data, ampl.ctypes.data,
                                                 bits.ctypes.data, fb.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_confidence failed: %d" % rc)
        return conf, ampl, bits, fb

    def selftest_corr(self, cfg, routine, samples, starts, lens=None, param=0):
        """mifsk_selftest_corr: the windows of cfg.bit_nsamples samples at `starts` of `samples`
        (for "seg_group": segments of `lens` samples) through one correlator of _lib.CORR_ROUTINES
        -> (acc[ncases, 4] doubles, the float energy sums of "seg_group" or None); case i runs on
        lane i % 64 of wave i / 64.  ValueError where the library refuses the cases (-EINVAL: a
        precondition of the routine does not hold; nothing was launched)."""
        samples = np.ascontiguousarray(samples, np.float32)
        starts = np.ascontiguousarray(starts, np.uint32)
        assert samples.ndim == 1 and starts.ndim == 1
        seg = routine == "seg_group"
        if seg:
            lens = np.ascontiguousarray(lens, np.uint32)
            assert lens.shape == starts.shape
        acc = np.empty((starts.size, 4), np.float64)
        esum = np.empty(starts.size, np.float32) if seg else None
        rc = self._lib.mifsk_selftest_corr(self.handle, C.byref(cfg), _lib.CORR_ROUTINES[routine], int(param),
                                           samples.ctypes.data, samples.size, starts.ctypes.data,
                                           lens.ctypes.data if seg else None, starts.size,
                                           acc.ctypes.data, esum.ctypes.data if seg else None)
        if rc == -22:
            raise ValueError("mifsk_selftest_corr refused the cases (-EINVAL)")
        if rc != 0:
            raise RuntimeError("mifsk_selftest_corr failed: %d" % rc)
        return acc, esum

    def selftest_scan(self, routine, state, cv, av, k, totals=True):
        """mifsk_selftest_scan: state[nwaves, 4] = (track, peak, confidence total, amplitude total)
        before frame 0, cv / av[nwaves, 64], k[nwaves] frames -> (x[nwaves, 64, 4], b[nwaves, 64, 4]):
        the state after and before every lane's frame.  routine: "asm", "soft" or "track"."""
        state = np.ascontiguousarray(state, np.float32)
        cv = np.ascontiguousarray(cv, np.float32)
        av = np.ascontiguousarray(av, np.float32)
        k = np.ascontiguousarray(k, np.uint32)
        n = k.size
        assert state.shape == (n, 4) and cv.shape == (n, 64) and av.shape == (n, 64)
        x, b = np.empty((n, 64, 4), np.float32), np.empty((n, 64, 4), np.float32)
        rc = self._lib.mifsk_selftest_scan(self.handle, _lib.SCAN_ROUTINES[routine], int(bool(totals)),
                                           state.ctypes.data, cv.ctypes.data, av.ctypes.data, k.ctypes.data, n,
                                           x.ctypes.data, b.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_scan failed: %d" % rc)
        return x, b

    def selftest_wave_max(self, v):
        """mifsk_selftest_wave_max: v[nwaves, 64] -> wave_max_f32 of every wave"""
        v = np.ascontiguousarray(v, np.float32)
        assert v.ndim == 2 and v.shape[1] == 64
        out = np.empty(v.shape[0], np.float32)
        rc = self._lib.mifsk_selftest_wave_max(self.handle, v.ctypes.data, v.shape[0], out.ctypes.data)
        if rc != 0:
            raise RuntimeError("mifsk_selftest_wave_max failed: %d" % rc)
        return out


def _torch():
    import torch
    return torch


def _on(torch, stream):
    """Allocations and fills that a launch on `stream` depends on are queued ON that stream
    (torch orders a fill on its current stream only: on another one it would race the kernel)."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _stream_ptr(torch, stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


_HOST = object()       # _call: the function takes no stream


def _call(name, *args, stream=_HOST, errors=None):
    """libmifsk's `name`(*args), and the handle of torch stream `stream` (None: the current one) behind
    them where one is given; raises where it returns non-zero: what errors[rc] makes of the message if
    there is one, else errors[None], else RuntimeError."""
    if stream is not _HOST:
        args += (_stream_ptr(_torch(), stream),)
    rc = getattr(_lib.load(), name)(*args)
    if rc != 0:
        errors = errors or {}
        raise errors.get(rc, errors.get(None, RuntimeError))("%s failed: %d" % (name, rc))


_EINVAL_IS_VALUE = {-22: ValueError}


# ---------------------------------------------------------------------------
# a batch of rows: what the batch entries' wrappers below share (csrc/mifsk_batch.h is the C++ side's)
# ---------------------------------------------------------------------------

_RowView = collections.namedtuple("_RowView", "t nstreams width stride s16 vec")


def _row_view(torch, t, cx=False, dtypes=None, one_row=True, whole=True, unit="samples", cuda=True):
    """A batch of rows as the C ABI takes it, from tensor `t` and what the entry accepts -> (the tensor as
    used, nstreams, width, elements between rows, PCM16?, elements of 16 bytes).  An element is a scalar,
    or with `cx` an I, Q pair.

    cx     : complex rows, interleaved: a last dimension of 2, or complex64 where `dtypes` names it
    dtypes : what the entry takes (default: float32 and int16)
    one_row: a 1-D tensor (complex: [w, 2]) is one row
    whole  : the kernels read whole 16-byte vectors: a lone row must hold them
    cuda   : refuse a tensor that is not on the device (the rest is a function of shape, strides and dtype)"""
    assert not cuda or t.is_cuda
    assert t.dtype in (dtypes or (torch.float32, torch.int16)), "the rows are not of the kind the entry takes"
    if t.dtype == torch.complex64:
        t = torch.view_as_real(t)
    per = 2 if cx else 1                    # scalars of an element
    if cx:
        assert t.shape[-1] == 2 and t.stride(-1) == 1, "complex rows are interleaved I, Q"
    if one_row and t.dim() == (2 if cx else 1):
        t = t[None]
    assert t.dim() == (3 if cx else 2) and t.stride(1) == per
    nstreams, width = int(t.shape[0]), int(t.shape[1])
    assert nstreams <= 1 or t.stride(0) % per == 0, "complex rows are interleaved I, Q"
    vec = 16 // (t.element_size() * per)
    # (a lone row's stride is arbitrary in torch -- numpy's x[None, :] has stride 0 -- so its width stands
    # in for it, and the row must hold the whole vectors that the kernels read)
    assert not whole or nstreams > 1 or width % vec == 0, \
        "a lone row must be padded to a multiple of %d %s" % (vec, unit)
    return _RowView(t, nstreams, width, t.stride(0) // per if nstreams > 1 else width, t.dtype == torch.int16, vec)


def _row_lengths(torch, nsamples, nstreams, width, allow_int=False, cuda=True):
    """The rows' lengths as the C ABI takes them -> (the address of [nstreams] uint32 or None, the length of
    every row then).  nsamples: None (the rows' width), an int where the entry allows one, or an
    int32/uint32 tensor [nstreams].  The address crosses as a raw pointer: what the kernels would silently
    misread (a CPU tensor, int64 lengths, a wrong shape) is refused."""
    if nsamples is None:
        return None, int(width)
    if allow_int and not torch.is_tensor(nsamples):
        return None, int(nsamples)
    assert torch.is_tensor(nsamples) and (nsamples.is_cuda or not cuda) \
        and nsamples.dtype in (torch.int32, torch.uint32), "nsamples must be a CUDA int32/uint32 tensor"
    assert nsamples.dim() == 1 and nsamples.shape[0] == nstreams and nsamples.is_contiguous()
    return nsamples.data_ptr(), int(width)


def _rows_io(io, v, lens, nstreams=None):
    """the rows at the head of every io (_lib.ROWS_FIELDS) from a view and its lengths -> io"""
    io.d_samples, io.stream_stride = (v.t.data_ptr() if v.t is not None else None), v.stride
    io.d_nsamples, io.nsamples = lens
    io.nstreams = v.nstreams if nstreams is None else nstreams
    return io


def _kind(s16):
    return _lib.FEED_S16 if s16 else _lib.FEED_F32


def _whole(n, vec):
    """n rounded up to whole vectors of `vec`, one at least"""
    return max(vec, (int(n) + vec - 1) // vec * vec)


def _new_outputs(torch, spec, device, stream):
    """New tensors {name: (shape, dtype, fill)} (fill None: not filled) for a launch on `stream`."""
    # (allocated and filled ON the launch stream: a fill queued on torch's current stream would race a
    # kernel launched on another one)
    with _on(torch, stream):
        out = {}
        for name, (shape, dtype, fill) in spec.items():
            if fill is None:
                out[name] = torch.empty(shape, dtype=dtype, device=device)
            elif fill == 0:
                out[name] = torch.zeros(shape, dtype=dtype, device=device)
            else:
                out[name] = torch.full(shape, fill, dtype=dtype, device=device)
    if stream is not None:
        # The tensors belong to `stream` in torch's caching allocator.  Whoever reads them on
        # another stream must order that read behind `stream` (an event, wait_stream); marking
        # them used on the current stream as well keeps the allocator from handing a dropped
        # tensor's block back out -- and its zero-fill onto `stream` -- under such a reader.
        cur = torch.cuda.current_stream()
        for t in out.values():
            t.record_stream(cur)
    return out


def _check_out_rows(torch, out, dtypes, nrows, tail=()):
    """What every entry asks of output rows that the caller brings: on the device, of one of `dtypes`,
    [nrows, stride, *tail], the rows filling their stride (every element up to the stride is written) -> out"""
    assert out.is_cuda and out.dtype in dtypes and out.dim() == 2 + len(tail)
    assert out.shape[0] == nrows and tuple(out.shape[2:]) == tuple(tail)
    assert out.is_contiguous(), "out's rows must fill their stride"
    return out


def _out_rows(torch, out, shape, dtype, device, stream, dtypes=None):
    """An entry's one tensor of output rows -> (it, elements between its rows): new, of `shape` and `dtype`,
    or the caller's `out` if it is of one of `dtypes` (default: `dtype`)."""
    if out is None:
        out = _new_outputs(torch, {"out": (shape, dtype, None)}, device, stream)["out"]
    else:
        _check_out_rows(torch, out, dtypes or (dtype,), shape[0], shape[2:])
    return out, int(out.shape[1])


def max_frames(cfg, nsamples):
    return int(_lib.load().mifsk_max_frames(C.byref(cfg), int(nsamples)))


def max_episodes(cfg, nsamples):
    return int(_lib.load().mifsk_max_episodes(C.byref(cfg), int(nsamples)))


def _default_caps(cfg, longest, frames_cap, episodes_cap):
    """The capacities a caller left open, from the longest stream."""
    return (max_frames(cfg, longest) if frames_cap is None else frames_cap,
            max_episodes(cfg, longest) if episodes_cap is None else episodes_cap)


def _io_flags(ring_exact=False, engine=None):
    return (_lib.IO_RING_EXACT if ring_exact else 0) | \
        (_lib.IO_ENGINE_WORKGROUP if engine == "workgroup" else 0) | \
        (_lib.IO_ENGINE_WAVE if engine == "wave" else 0)


def _struct_dict(st, drop_reserved=False):
    return {k: getattr(st, k) for k, _ in st._fields_ if not (drop_reserved and k == "reserved")}


def _demod_outputs(torch, cfg, dev, nstreams, want, frames_cap, episodes_cap, stream, counters=False):
    """demod_batch's output tensors; "counters" only where the caller can get them (demod_batch)."""
    n, u8, i32, i64 = nstreams, torch.uint8, torch.int32, torch.int64
    spec = {"nframes": ((n,), i32, 0), "status": ((n,), i32, 0)}
    if "bytes" in want:
        spec.update(bytes=((n, frames_cap), u8, 0), nbytes=((n,), i32, 0))
    if "bits" in want:
        spec["bits"] = ((n, frames_cap), i64, 0)
    if "frames" in want:
        spec["frames"] = ((n, frames_cap, FRAME_DTYPE.itemsize), u8, 0)
    if counters and "counters" in want:
        spec["counters"] = ((n, NCOUNTERS), i64, 0)
    if "carrier_band" in want or cfg.auto_carrier_threshold > 0:
        spec["carrier_band"] = ((n,), i32, -1)
    if "episodes" in want:
        spec.update(episodes=((n, episodes_cap, EPISODE_DTYPE.itemsize), u8, 0), nepisodes=((n,), i32, 0))
    return _new_outputs(torch, spec, dev, stream)


def _numpy_outputs(nstreams, want, frames_cap, episodes_cap):
    """The host entry points' result arrays."""
    res = {"nframes": np.zeros(nstreams, np.uint32), "status": np.zeros(nstreams, np.uint32),
           "carrier_band": np.full(nstreams, -1, np.int32)}
    if "bytes" in want:
        res["bytes"] = np.zeros((nstreams, frames_cap), np.uint8)
        res["nbytes"] = np.zeros(nstreams, np.uint32)
    if "bits" in want:
        res["bits"] = np.zeros((nstreams, frames_cap), np.uint64)
    if "frames" in want:
        res["frames"] = np.zeros((nstreams, frames_cap), FRAME_DTYPE)
    if "episodes" in want:
        res["episodes"] = np.zeros((nstreams, episodes_cap), EPISODE_DTYPE)
        res["nepisodes"] = np.zeros(nstreams, np.uint32)
    return res


def _result_io(out, nstreams, frames_cap, episodes_cap, address):
    """A DemodIO whose result pointers are the arrays of `out` (a dict as the two functions above
    make it; what it lacks stays NULL); address: how one of its values turns into an address."""
    io = _lib.DemodIO()
    io.nstreams = nstreams
    io.frames_cap = frames_cap
    io.episodes_cap = episodes_cap
    for name in ("bytes", "nbytes", "bits", "frames", "nframes", "episodes", "nepisodes", "status", "counters",
                 "carrier_band"):
        if out.get(name) is not None:
            setattr(io, "d_" + name, address(out[name]))
    return io


def _tensor_address(t):
    return t.data_ptr()


def _array_address(a):
    return a.ctypes.data


def demod_batch(ctx, cfg, samples, nsamples=None, want=("bytes", "episodes"),
                frames_cap=None, episodes_cap=8, stream=None, out=None, ring_exact=False,
                engine=None, force_engine=False):
    """Run the receive loop over a batch of streams resident in HBM.

    samples : torch.float32 CUDA tensor [nstreams, stride] (stride % 4 == 0)
    nsamples: optional torch.int32/uint32 CUDA tensor [nstreams]; default: stride
    Returns a dict of CUDA tensors (no synchronisation is performed).
    `out` may be a dict returned by a previous call with the same shapes, to
    reuse its buffers (nothing is allocated inside the timed region then).
    ring_exact: MIFSK_IO_RING_EXACT (the reference's stale-cell buffer semantics).
    engine: None (the library chooses), "wave" (one wavefront per stream,
    MIFSK_IO_ENGINE_WAVE) or "workgroup" (one workgroup of a master and 2-3 worker waves per stream,
    MIFSK_IO_ENGINE_WORKGROUP); force_engine=True makes None mean "wave".
    """
    torch = _torch()
    v = _row_view(torch, samples, dtypes=(torch.float32,), one_row=False)
    lens = _row_lengths(torch, nsamples, v.nstreams, v.width)      # (the kernels clamp lengths to the row width)
    if frames_cap is None:
        frames_cap = max_frames(cfg, v.width)
    if out is None:
        out = _demod_outputs(torch, cfg, samples.device, v.nstreams, want, frames_cap, episodes_cap, stream,
                             counters=True)
    io = _rows_io(_result_io(out, v.nstreams, frames_cap, episodes_cap, _tensor_address), v, lens)
    if engine is None and force_engine:
        engine = "wave"
    io.flags = _io_flags(ring_exact, engine)
    _call("mifsk_demod_batch", ctx.handle, C.byref(cfg), C.byref(io), stream=stream)
    return out


def frame_softbits(ctx, cfg, samples, out, nsamples=None, origin=None, rxnoise=0.0, stream=None, rawbits=True):
    """mifsk_frame_softbits: the mark and space magnitudes of every bit window of the frames in
    `out` -- a result dict of demod_batch / demod_long[_batch] made with "frames" in `want`.

    samples : torch.float32 or torch.int16 (PCM16) CUDA tensor [nstreams, stride] (stride % 4 == 0,
              % 8 == 0 for PCM16), or 1-D for one stream; the rows the frames were decoded from, or
              rows that start at `origin` in them
    nsamples: optional torch.int32/uint32 CUDA tensor [nstreams]; default: the rows' width
    origin  : optional torch.int64 CUDA tensor [nstreams], the stream index of each row's sample 0;
              frames that start before it get magnitudes of -1
    rxnoise : the --Xrxnoise factor, PCM16 only (mifsk_ingest_s16's term)
    Returns {"mag": float32 [nstreams, frames_cap, expect_n_bits, 2] (mark, space), "rawbits": int64
    [nstreams, frames_cap] (bit k = mark > space of bit window k; absent with rawbits=False)},
    allocated on the launch stream; entries at or beyond a stream's frame count are 0.  No
    synchronisation is performed."""
    torch = _torch()
    v = _row_view(torch, samples)
    nstreams = v.nstreams
    lens = _row_lengths(torch, nsamples, nstreams, v.width)
    frames, nframes = out["frames"], out["nframes"]
    assert frames.is_cuda and frames.is_contiguous() and frames.dim() == 3 and frames.shape[0] == nstreams \
        and frames.shape[2] == FRAME_DTYPE.itemsize, "out must hold the frames of these streams"
    assert nframes.is_cuda and nframes.is_contiguous() and nframes.shape == (nstreams,)
    if origin is not None:
        assert origin.is_cuda and origin.dtype == torch.int64 and origin.is_contiguous() \
            and origin.shape == (nstreams,)
    frames_cap = int(frames.shape[1])
    spec = {"mag": ((nstreams, frames_cap, int(cfg.expect_n_bits), 2), torch.float32, 0)}
    if rawbits:
        spec["rawbits"] = ((nstreams, frames_cap), torch.int64, 0)
    res = _new_outputs(torch, spec, v.t.device, stream)
    io = _rows_io(_lib.SoftbitsIO(), v, lens)
    io.kind = _kind(v.s16)
    io.rxnoise = float(rxnoise)
    io.d_origin = origin.data_ptr() if origin is not None else None
    io.d_frames = frames.data_ptr()
    io.d_nframes = nframes.data_ptr()
    io.frames_cap = frames_cap
    io.d_mag = res["mag"].data_ptr()
    io.d_rawbits = res["rawbits"].data_ptr() if rawbits else None
    _call("mifsk_frame_softbits", ctx.handle, C.byref(cfg), C.byref(io), stream=stream)
    return res


def carrier_windows(nsamples, window, hop=0, first=0):
    """mifsk_carrier_windows: how many whole windows of `window` samples, `hop` apart (0: window) from
    `first` on, a row of `nsamples` samples holds."""
    return int(_lib.load().mifsk_carrier_windows(int(nsamples), int(first), int(window), int(hop)))


def carrier_tones(cfg, band):
    """mifsk_carrier_tones: the tone pair --auto-carrier tunes to when it detects `band` ->
    {"b_mark", "b_space", "mark_f", "space_f"}.  ValueError for a band outside 1 .. nbands-1 or a
    configuration without a shift, IndexError where the space band falls outside 1 .. nbands-1 (the
    receive loop drops such a detection)."""
    bm, bs, fm, fs = C.c_uint(0), C.c_uint(0), C.c_float(0), C.c_float(0)
    outside = IndexError("band %d: the space band falls outside 1 .. %d" % (band, cfg.nbands - 1))
    _call("mifsk_carrier_tones", C.byref(cfg), int(band), C.byref(bm), C.byref(bs), C.byref(fm), C.byref(fs),
          errors={-34: lambda _: outside, None: ValueError})
    return {"b_mark": bm.value, "b_space": bs.value, "mark_f": fm.value, "space_f": fs.value}


def carrier_window_default(cfg):
    """The window --auto-carrier scans with: (unsigned)min(nsamples_per_bit, fftsize)
    (minimodem.c:1179-1190)."""
    return int(min(np.float32(cfg.nsamples_per_bit), np.float32(cfg.fftsize)))


def carrier_survey(ctx, cfg, samples, nsamples=None, window=None, hop=None, first=0, nwindows=None,
                   threshold=0.001, spectrum=False, rxnoise=0.0, stream=None, out=None):
    """mifsk_detect_carrier_batch: fsk_detect_carrier on every window of every stream.

    samples : torch.float32 or torch.int16 (PCM16) CUDA tensor [nstreams, stride] (stride % 4 == 0,
              % 8 == 0 for PCM16), or 1-D for one stream
    nsamples: optional torch.int32/uint32 CUDA tensor [nstreams]; default: the rows' width
    window  : samples per window (None: what --auto-carrier uses); hop: samples between window starts
              (None: window); first: start of window 0 in every row
    nwindows: windows per stream (None: carrier_windows of the rows' width)
    threshold: min_mag_threshold; spectrum: also return every band's magnitude
    rxnoise : the --Xrxnoise factor, PCM16 only
    out     : a dict a former call with the same shapes returned, to reuse its tensors
    Returns {"band": int32 [nstreams, nwindows] (the band, -1 = none reached the threshold, -2 = the
    window does not lie wholly inside the row), "mag": float32 [nstreams, nwindows], "spectrum":
    float32 [nstreams, nwindows, nbands] with spectrum=True, "window", "hop"}, allocated on the launch
    stream.  No synchronisation is performed."""
    torch = _torch()
    v = _row_view(torch, samples)
    nstreams = v.nstreams
    lens = _row_lengths(torch, nsamples, nstreams, v.width)
    window = carrier_window_default(cfg) if window is None else int(window)
    hop = window if not hop else int(hop)
    if nwindows is None:
        nwindows = max(1, carrier_windows(v.width, window, hop, first))
    nwindows = int(nwindows)
    if out is None:
        spec = {"band": ((nstreams, nwindows), torch.int32, _lib.CARRIER_NO_WINDOW),
                "mag": ((nstreams, nwindows), torch.float32, 0)}
        if spectrum:
            spec["spectrum"] = ((nstreams, nwindows, int(cfg.nbands)), torch.float32, 0)
        out = _new_outputs(torch, spec, v.t.device, stream)
    else:
        assert out["band"].shape == (nstreams, nwindows) and out["band"].is_contiguous()
        assert (not spectrum) or out["spectrum"].shape == (nstreams, nwindows, int(cfg.nbands))
    io = _rows_io(_lib.CarrierIO(), v, lens)
    io.kind = _kind(v.s16)
    io.rxnoise = float(rxnoise)
    io.first = int(first)
    io.window = window
    io.hop = hop
    io.nwindows = nwindows
    io.threshold = float(threshold)
    io.d_band = out["band"].data_ptr()
    io.d_mag = out["mag"].data_ptr()
    io.d_spectrum = out["spectrum"].data_ptr() if spectrum else None
    _call("mifsk_detect_carrier_batch", ctx.handle, C.byref(cfg), C.byref(io), stream=stream)
    out["window"], out["hop"] = window, hop
    return out


def channel_taps(ntaps, cutoff, sample_rate, gain=1.0):
    """mifsk_channel_taps: `ntaps` Hamming-windowed sinc taps with a cutoff of `cutoff` Hz at
    `sample_rate`, scaled to sum to `gain`, as a float32 numpy array (a real input wants gain 2)."""
    out = np.empty(int(ntaps), np.float32)
    _call("mifsk_channel_taps", int(ntaps), float(cutoff), float(sample_rate), float(gain), out.ctypes.data,
          errors={None: ValueError})
    return out


def _phase_params(p, taps, centres, phase_steps, flags, s16):
    """the fields mifsk_channel_params and mifsk_mux_params share -> (p, [the arrays it points to])"""
    taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
    centres = np.ascontiguousarray(centres, np.int32).reshape(-1)
    p.kind, p.flags = _lib.FEED_S16 if s16 else _lib.FEED_F32, flags
    p.phase_steps, p.ntaps, p.taps = int(phase_steps), taps.size, taps.ctypes.data
    p.nchannels, p.centres = centres.size, centres.ctypes.data
    return p, [taps, centres]


def _channel_params(taps, decim, centres, out_centre, phase_steps, complex_input, s16):
    """(mifsk_channel_params, the arrays it points to)"""
    p, keep = _phase_params(_lib.ChannelParams(), taps, centres, phase_steps,
                            _lib.CHANNEL_COMPLEX if complex_input else 0, s16)
    p.decim, p.out_centre = int(decim), int(out_centre)
    return p, keep


def channel_table(taps, centres, k, phase_steps):
    """mifsk_channel_table: channel k's G as a plan makes it, float64 [ntaps, 2] (host only)."""
    p, _keep = _channel_params(taps, 1, centres, 0, phase_steps, False, False)
    g = np.empty((p.ntaps, 2), np.float64)
    _call("mifsk_channel_table", C.byref(p), int(k), g.ctypes.data, errors={None: ValueError})
    return g


class _PhasePlan(_Handle):
    """what ChannelPlan and MuxPlan share: the handle the library makes of the parameters"""

    def _create(self, ctx, params, create, destroy):
        self._lib, self._destroy = _lib.load(), destroy
        p, _keep = params
        h = C.c_void_p()
        _call(create, ctx.handle, C.byref(p), C.byref(h), errors=_EINVAL_IS_VALUE)
        self.handle = h
        self.ctx = ctx                      # the plan must not outlive its context
        self.ntaps, self.nchannels, self.s16 = p.ntaps, p.nchannels, p.kind == _lib.FEED_S16
        return p


class _RowStream(_Handle):
    """what ChannelStream and MuxStream share: the object that the entries named `_entry`_... make of a plan for
    `nstreams` streams, and its counters"""

    def _create(self, plan, nstreams, *flags):
        self._lib, self._destroy = _lib.load(), self._entry + "_destroy"
        h = C.c_void_p()
        _call(self._entry + "_create", plan.handle, int(nstreams), *flags, C.byref(h), errors=_EINVAL_IS_VALUE)
        self.handle = h
        self.plan, self.nstreams = plan, int(nstreams)      # the object must not outlive its plan

    def seek(self, seen=None, stream=None):
        """..._seek: every stream has seen seen[s] elements (None: 0, the reset) and reads nothing in front of
        them again; the class says where the outputs go on.  Waits for `stream`."""
        arr = None
        if seen is not None:
            arr = np.ascontiguousarray(seen, np.uint64).reshape(-1)
            assert arr.size == self.nstreams, "one count per stream"
        _call(self._entry + "_seek", self.handle, None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_uint64)),
              stream=stream, errors=_EINVAL_IS_VALUE)

    def seen(self, stream=None):
        """..._seen: the elements every stream has seen, numpy uint64 [nstreams].  Waits for `stream` (None: the
        current one)."""
        out = np.empty(self.nstreams, np.uint64)
        _call(self._entry + "_seen", self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), stream=stream)
        return out


def _row_outputs(torch, nrows, full, vec, dtype, tail, device, stream, out):
    """The outputs of channelize and multiplex, {"rows": `dtype` [nrows, out_stride, *tail], "nsamples":
    int32 [nrows]}: made on the launch stream, out_stride the whole vectors of `vec` elements that hold
    `full` (one at least), or `out`, a dict of a former call, when its tensors are of that kind (`full`
    is not looked at then)."""
    if out is None:
        return _new_outputs(torch, {"rows": ((nrows, _whole(full, vec)) + tail, dtype, None),
                                    "nsamples": ((nrows,), torch.int32, None)}, device, stream)
    _check_out_rows(torch, out["rows"], (dtype,), nrows, tail)
    counts = out["nsamples"]
    assert counts.shape == (nrows,) and counts.dtype == torch.int32 and counts.is_contiguous()
    return out


def _phase_io(io, rows_field, v, lens, nstreams, out, nout_cap):
    """the fields mifsk_channel_io and mifsk_mux_io share (the output rows are `rows_field`) -> io"""
    out_stride = out["rows"].shape[1]
    _rows_io(io, v, lens, nstreams)
    setattr(io, rows_field, out["rows"].data_ptr())
    io.out_stride = out_stride
    io.nout_cap = out_stride if nout_cap is None else min(int(nout_cap), out_stride)
    io.d_nout = out["nsamples"].data_ptr()
    return io


class ChannelPlan(_PhasePlan):
    """mifsk_channel_plan: the tables of a channelizer on ctx's device.

    taps       : float32 filter taps (channel_taps), 1 .. 4096
    decim      : output m is the window that starts at input element m * decim
    centres    : the channels' centres in steps of fs_in / phase_steps Hz, negative allowed
    out_centre : where every channel is moved to, same unit (real rows out)
    complex_input: rows are interleaved I, Q; s16: the scalars are PCM16"""

    def __init__(self, ctx, taps, decim, centres, out_centre, phase_steps, complex_input=False, s16=False):
        p = self._create(ctx, _channel_params(taps, decim, centres, out_centre, phase_steps, complex_input, s16),
                         "mifsk_channel_plan_create", "mifsk_channel_plan_destroy")
        self.decim, self.complex_input = p.decim, bool(complex_input)


def _channel_io(plan, samples, nsamples, full, nout_cap, stream, out, iq):
    """What channelize and ChannelStream.feed do in front of their entry: `samples` and `nsamples` checked
    against the plan's kind, the outputs made (full(width): the outputs a row of that width needs room for)
    or `out` taken over -> (the outputs' dict, the mifsk_channel_io of the call)."""
    torch = _torch()
    kinds = (torch.int16,) if plan.s16 else (torch.float32, torch.complex64) if plan.complex_input else (torch.float32,)
    v = _row_view(torch, samples, cx=plan.complex_input, dtypes=kinds, unit="elements")
    lens = _row_lengths(torch, nsamples, v.nstreams, v.width)
    out = _row_outputs(torch, v.nstreams * plan.nchannels, out is None and full(v.width), 2 if iq else 4, torch.float32,
                       (2,) if iq else (), v.t.device, stream, out)
    return out, _phase_io(_lib.ChannelIO(), "d_rows", v, lens, v.nstreams, out, nout_cap)


def channelize(plan, samples, nsamples=None, nout_cap=None, stream=None, out=None, iq=False):
    """mifsk_channelize_batch: every channel of every row as a row demod_batch takes; with iq=True
    mifsk_channelize_iq_batch: every channel as a row of I, Q pairs, which fm_demod takes (plan the
    channelizer with out_centre=0 for the complex envelope).

    samples : CUDA tensor [nstreams, stride] (or 1-D for one stream) of the plan's kind: float32 or
              int16 (PCM16) for real rows; for complex rows complex64, or float32 / int16 with a last
              dimension of 2 (I, Q).  Rows are 16-byte aligned and a whole number of 16-byte vectors apart.
    nsamples: optional torch.int32/uint32 CUDA tensor [nstreams] of elements; default: the rows' width
    nout_cap: outputs per row at most (None: what a full row gives, at least 4, rounded up to 4)
    out     : a dict a former call with the same shapes returned, to reuse its tensors
    Returns {"rows": float32 [nstreams * nchannels, out_stride], "nsamples": int32 [nstreams * nchannels]}:
    row s * nchannels + k is channel k of stream s, zero behind its count.  Allocated on the launch
    stream.  No synchronisation is performed.
    iq=True : "rows" is float32 [nstreams * nchannels, out_stride, 2], element m of a row (I, Q); out_stride
              and nout_cap count such elements (None: what a full row gives, at least 2, rounded up to 2);
              "rows" and "nsamples" are what fm_demod takes as iq and nsamples."""
    def full(width):
        return carrier_windows(width, plan.ntaps, plan.decim) if nout_cap is None else int(nout_cap)
    out, io = _channel_io(plan, samples, nsamples, full, nout_cap, stream, out, iq)
    _call("mifsk_channelize_iq_batch" if iq else "mifsk_channelize_batch", plan.handle, C.byref(io), stream=stream)
    return out


def channel_stream_outputs(ntaps, decim, seen, k):
    """mifsk_channel_stream_outputs: the outputs a ChannelStream that has seen `seen` elements delivers for `k`
    more, M(seen + k) - M(seen) with M(n) = (n - ntaps) // decim + 1 for n >= ntaps, else 0 (host only)."""
    return int(_lib.load().mifsk_channel_stream_outputs(int(ntaps), int(decim), int(seen), int(k)))


class ChannelStream(_RowStream):
    """mifsk_channel_stream (include/mifsk/channel_stream.h): `plan`'s channelizer fed in pieces.  The concatenated
    outputs of the feeds are channelize's on the concatenated capture, bit for bit; every output comes with the
    feed that brings its last element.  Counters and tails of `nstreams` streams live on the plan's device.
    Feeds of one object are ordered by the caller: one stream, or events.  Behind seek(seen) a stream holds no
    tail: its next output is the first m with m * decim >= seen[s]."""
    _entry = "mifsk_channel_stream"

    def __init__(self, plan, nstreams):
        self._create(plan, nstreams)

    def feed(self, samples, nsamples=None, stream=None, out=None, iq=False):
        """mifsk_channel_stream_feed: the next piece of every stream, as channelize takes a batch: `samples`
        [nstreams, stride] of the plan's kind, `nsamples` None (the rows' width) or a CUDA int32/uint32 tensor
        [nstreams] of new elements (0: the stream stays as it is).  Returns channelize's dict, {"rows",
        "nsamples"}: what THIS piece completes, zero behind the counts.  The default out_stride is
        ceil(width / decim) rounded up to 4 (iq=True: to 2), which no piece of that width exceeds; `out`, a dict
        of a former feed, is reused when its tensors are of that kind.  No synchronisation is performed."""
        out, io = _channel_io(self.plan, samples, nsamples, lambda width: -(-width // self.plan.decim), None, stream, out, iq)
        _call("mifsk_channel_stream_feed", self.handle, C.byref(io), _lib.CHANNEL_STREAM_IQ if iq else 0,
              stream=stream, errors=_EINVAL_IS_VALUE)
        return out


def _mux_params(taps, interp, centres, in_centre, phase_steps, complex_output, s16, gains):
    """(mifsk_mux_params, the arrays it points to)"""
    p, keep = _phase_params(_lib.MuxParams(), taps, centres, phase_steps, _lib.MUX_COMPLEX if complex_output else 0, s16)
    p.interp, p.in_centre = int(interp), int(in_centre)
    if gains is not None:
        gains = np.ascontiguousarray(gains, np.float32).reshape(-1)
        assert gains.size == p.nchannels, "one gain per channel"
        p.gains = gains.ctypes.data
        keep.append(gains)
    return p, keep


def mux_table(taps, in_centre, phase_steps):
    """mifsk_mux_table: G as a multiplexer plan makes it, float64 [ntaps, 2] (host only)."""
    p, _keep = _mux_params(taps, 1, [0], in_centre, phase_steps, False, False, None)
    g = np.empty((p.ntaps, 2), np.float64)
    _call("mifsk_mux_table", C.byref(p), g.ctypes.data, errors={None: ValueError})
    return g


class MuxPlan(_PhasePlan):
    """mifsk_mux_plan: the tables of a multiplexer on ctx's device.

    taps       : float32 filter taps at the OUTPUT rate (channel_taps(T, fc, fs_out, 2 * interp) for
                 unit gain), 1 .. 4096
    interp     : output samples per input sample
    centres    : where each channel goes, in steps of fs_out / phase_steps Hz, negative allowed
    in_centre  : the input rows' tone centre, same unit: the band the filter keeps
    complex_output: rows are interleaved I, Q; s16: the scalars are PCM16
    gains      : None, or one float per channel
    For multiplex(..., iq=True) the input rows are complex envelopes: in_centre is the envelope's centre
    (0 for fm_modulate with centre=0), and unit gain wants taps that sum to interp,
    channel_taps(T, fc, fs_out, interp): a complex row is one-sided already."""

    def __init__(self, ctx, taps, interp, centres, in_centre, phase_steps, complex_output=False, s16=False,
                 gains=None):
        p = self._create(ctx, _mux_params(taps, interp, centres, in_centre, phase_steps, complex_output, s16, gains),
                         "mifsk_mux_plan_create", "mifsk_mux_plan_destroy")
        self.interp, self.complex_output = p.interp, bool(complex_output)


def _mux_io(plan, samples, nsamples, iq, nstreams, full, nout_cap, stream, out):
    """What multiplex and MuxStream.feed do in front of their entry: `samples` (`iq`: rows of I, Q pairs) and
    `nsamples` checked against the plan's channels and `nstreams` (None: as many as the rows give), the outputs
    made (full(width): the outputs rows of that width need room for) or `out` taken over -> (the outputs' dict,
    the mifsk_mux_io of the call)."""
    torch = _torch()
    if iq:
        v = _row_view(torch, samples, cx=True, dtypes=(torch.float32, torch.complex64), one_row=False, unit="elements")
    else:
        v = _row_view(torch, samples, dtypes=(torch.float32,), one_row=False, unit="floats")
    if nstreams is None:
        nstreams = v.nstreams // plan.nchannels
    assert v.nstreams > 0 and v.nstreams == nstreams * plan.nchannels, "samples holds nchannels rows per stream"
    lens = _row_lengths(torch, nsamples, v.nstreams, v.width)
    dtype = torch.int16 if plan.s16 else torch.float32
    vec = 16 // ((2 if plan.s16 else 4) * (2 if plan.complex_output else 1))
    out = _row_outputs(torch, nstreams, out is None and full(v.width), vec, dtype, (2,) if plan.complex_output else (),
                       samples.device, stream, out)
    return out, _phase_io(_lib.MuxIO(), "d_out", v, lens, nstreams, out, nout_cap)


def multiplex(plan, samples, nsamples=None, nout_cap=None, stream=None, out=None, iq=False):
    """mifsk_multiplex_batch: the channels of every stream summed into one wideband row; with iq=True
    mifsk_multiplex_iq_batch: the same from rows of I, Q pairs, what fm_modulate writes.

    samples : float32 CUDA tensor [nstreams * nchannels, stride], what synthesize_batch returns: row
              s * nchannels + k is channel k of stream s.  Rows are 16-byte aligned, stride % 4 == 0.
    nsamples: optional torch.int32/uint32 CUDA tensor [nstreams * nchannels]; default: the rows' width
    nout_cap: outputs per stream at most (None: what full rows give, (width - 1) * interp + ntaps)
    out     : a dict a former call with the same shapes returned, to reuse its tensors
    Returns {"rows": [nstreams, out_stride] (complex plans: [nstreams, out_stride, 2]) float32 or int16,
    "nsamples": int32 [nstreams]}; a row is zero behind its count.  Allocated on the launch stream.
    No synchronisation is performed.
    iq=True : samples is float32 [nstreams * nchannels, stride, 2] (I, Q) or complex64 [nstreams * nchannels,
              stride], stride % 2 == 0; nsamples counts such elements.  fm_modulate's float32 result goes in
              as it is, and so do "rows" and "nsamples" of channelize(..., iq=True).  The outputs are as above."""
    def full(width):
        return (width - 1) * plan.interp + plan.ntaps if nout_cap is None else int(nout_cap)
    out, io = _mux_io(plan, samples, nsamples, iq, None, full, nout_cap, stream, out)
    _call("mifsk_multiplex_iq_batch" if iq else "mifsk_multiplex_batch", plan.handle, C.byref(io), stream=stream)
    return out


def mux_stream_drain(ntaps, interp):
    """mifsk_mux_stream_drain: H = ceil(ntaps / interp) - 1, the samples of +0.0 that, fed behind the last piece
    of a MuxStream, bring out the rest of the filter's tail; 0 for interp == 0 (host only)."""
    return int(_lib.load().mifsk_mux_stream_drain(int(ntaps), int(interp)))


class MuxStream(_RowStream):
    """mifsk_mux_stream (include/mifsk/mux_stream.h): `plan`'s multiplexer fed in pieces.  The concatenated outputs
    of the feeds are multiplex's on the concatenated rows, bit for bit, on the first N * interp elements (N: the
    rows' length); mux_stream_drain(ntaps, interp) more samples of 0.0 bring out the filter's tail.  iq=True: the
    input rows are (I, Q) pairs, as multiplex(..., iq=True) takes them; the kind is fixed at creation.  Counters
    and tails of `nstreams` streams live on the plan's device.  Feeds of one object are ordered by the caller: one
    stream, or events.  Behind seek(seen) no sample in front of seen[s] exists: the next feed delivers the outputs
    from seen[s] * interp on."""
    _entry = "mifsk_mux_stream"

    def __init__(self, plan, nstreams, iq=False):
        self._create(plan, nstreams, _lib.MUX_STREAM_IQ if iq else 0)
        self.iq = bool(iq)

    def feed(self, samples, nsamples=None, stream=None, out=None):
        """mifsk_mux_stream_feed: the next piece of every row, as multiplex takes a batch: `samples`
        [nstreams * nchannels, stride] float32 (iq: [.., stride, 2] or complex64), `nsamples` None (the rows'
        width) or a CUDA int32/uint32 tensor [nstreams * nchannels] of new samples.  A stream advances by the
        longest of its rows, k; shorter rows are continued with 0.0 (all 0: the stream stays as it is).  Returns
        multiplex's dict, {"rows", "nsamples"}: the k * interp outputs of THIS piece, zero behind the counts.  The
        default out_stride is width * interp rounded up to the output kind's vector, which no piece of that
        width exceeds; `out`, a dict of a former feed, is reused when its tensors are of that kind.  No
        synchronisation is performed."""
        out, io = _mux_io(self.plan, samples, nsamples, self.iq, self.nstreams, lambda width: width * self.plan.interp,
                          None, stream, out)
        _call("mifsk_mux_stream_feed", self.handle, C.byref(io), stream=stream, errors=_EINVAL_IS_VALUE)
        return out


def snr_sigma(amplitude, snr_db):
    """mifsk_impair_sigma: the noise sigma that puts a tone of `amplitude` (power amplitude^2 / 2) at
    snr_db; float("inf") gives 0.0."""
    return float(_lib.load().mifsk_impair_sigma(C.c_float(amplitude), C.c_double(snr_db)))


def impair(ctx, samples, nsamples=None, seed=0, sigma=0.0, gain=1.0, dc=0.0, first_stream=0, first_sample=0,
           s16_out=None, out=None, stream=None):
    """mifsk_impair_batch, the channel model: out = gain * x + dc + sigma * z, z the library's noise field,
    a pure function of (seed, first_stream + row, first_sample + column).

    samples : CUDA tensor [nstreams, stride] (or 1-D for one stream), float32 or int16 (PCM16); rows are
              16-byte aligned and a whole number of 16-byte vectors apart.  None (with out=) or a shape
              (nstreams, width) gives noise rows: x = 0.
    nsamples: None (the rows' width), an int, or a torch.int32/uint32 CUDA tensor [nstreams]
    sigma, gain, dc: each a number or a float32 CUDA tensor [nstreams], one value per row
    first_stream, first_sample: where row 0 and column 0 lie in the field (a shard of the rows, a piece
              of the columns; first_sample % 4 == 0)
    s16_out : PCM16 output; None: out's kind, else the input's (float32 for noise rows)
    out     : the output tensor [nstreams, out_stride], float32 or int16, its rows filling their stride (every
              element up to the stride is written); out=samples is in place.  None: a new tensor, the width rounded up to whole 16-byte vectors, made on the launch stream.
    Returns out; a row is zero behind its length.  No synchronisation is performed."""
    torch = _torch()
    shape = None
    if samples is not None and not torch.is_tensor(samples):
        shape, samples = tuple(int(n) for n in samples), None
        assert len(shape) == 2, "a shape is (nstreams, width)"
    if samples is not None:
        if samples.dim() == 1 and out is not None and out.dim() == 1:
            out = out[None, :]
        v = _row_view(torch, samples)
        device = samples.device
    else:
        assert out is not None or shape is not None, "noise rows want out= or a shape"
        n, w = shape if shape is not None else out.shape
        v = _RowView(None, int(n), int(w), 0, False, 4)             # no rows: x = 0
        device = out.device if out is not None else torch.device("cuda")
    lens = _row_lengths(torch, nsamples, v.nstreams, v.width, allow_int=True)
    out_s16 = out.dtype == torch.int16 if out is not None else v.s16 if s16_out is None else bool(s16_out)
    out, out_stride = _out_rows(torch, out, (v.nstreams, _whole(v.width, 8 if out_s16 else 4)),
                                torch.int16 if out_s16 else torch.float32, device, stream,
                                dtypes=(torch.float32, torch.int16))
    assert s16_out is None or bool(s16_out) == out_s16, "out is not of the kind s16_out asks for"

    io = _rows_io(_lib.ImpairIO(), v, lens)
    io.kind, io.out_kind = _kind(v.s16), _kind(out_s16)
    io.d_out, io.out_stride = out.data_ptr(), out_stride
    io.seed, io.first_stream, io.first_sample = int(seed), int(first_stream), int(first_sample)
    for name, val in (("gain", gain), ("sigma", sigma), ("dc", dc)):
        if torch.is_tensor(val):
            assert val.is_cuda and val.dtype == torch.float32 and val.shape == (v.nstreams,) and val.is_contiguous(), \
                "%s: a float32 CUDA tensor [nstreams]" % name
            setattr(io, "d_" + name, val.data_ptr())
        else:
            setattr(io, name, float(val))
    _call("mifsk_impair_batch", ctx.handle, C.byref(io), stream=stream)
    return out


def fm_gain(sample_rate, deviation_hz):
    """mifsk_fm_gain: the discriminator gain that puts +-deviation_hz at +-1.0."""
    return float(_lib.load().mifsk_fm_gain(C.c_double(sample_rate), C.c_double(deviation_hz)))


def fm_step(deviation_hz, sample_rate):
    """mifsk_fm_step: Hertz as turns per sample, the modulator's `deviation` and `centre`."""
    return float(_lib.load().mifsk_fm_step(C.c_double(deviation_hz), C.c_double(sample_rate)))


def fm_demod(ctx, iq, nsamples=None, gain=1.0, prev=None, last=None, stream=None, out=None):
    """mifsk_fm_demod_batch, the NBFM discriminator: out[n] = gain * turn(z[n] * conj(z[n - 1])), the angle
    in turns by the library's own arithmetic (reproducible bit for bit; tools/fm_ref.c).

    iq      : CUDA tensor [nstreams, stride, 2] of interleaved I, Q, float32 or int16 (PCM16); rows are 16-byte
              aligned and a whole number of 16-byte vectors apart
    nsamples: None (the rows' width), an int, or a torch.int32/uint32 CUDA tensor [nstreams]
    gain    : fm_gain(sample_rate, deviation_hz) puts full deviation at +-1.0
    prev    : None ((0, 0): out[0] = 0), or a float32 CUDA tensor [nstreams, 2]: the sample before each row
    last    : None, or a float32 CUDA tensor [nstreams, 2] (not `prev`) that receives each row's last valid
              sample: the next piece's `prev`
    out     : the output tensor, float32 [nstreams, out_stride], out_stride % 4 == 0, its rows filling their
              stride.  None: a new tensor, the width rounded up to 4, made on the launch stream.
    Returns out; a row is zero behind its length.  No synchronisation is performed."""
    torch = _torch()
    v = _row_view(torch, iq, cx=True, one_row=False, unit="elements")
    nstreams = v.nstreams
    lens = _row_lengths(torch, nsamples, nstreams, v.width, allow_int=True)
    out, out_stride = _out_rows(torch, out, (nstreams, _whole(v.width, 4)), torch.float32, iq.device, stream)
    io = _rows_io(_lib.FmDemodIO(), v, lens)
    io.kind = _kind(v.s16)
    io.d_out, io.out_stride, io.gain = out.data_ptr(), out_stride, float(gain)
    for name, t in (("d_prev", prev), ("d_last", last)):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == (nstreams, 2) and t.is_contiguous(), \
                "%s: a float32 CUDA tensor [nstreams, 2]" % name[2:]
            setattr(io, name, t.data_ptr())
    assert prev is None or last is None or prev.data_ptr() != last.data_ptr(), "last must not be prev"
    _call("mifsk_fm_demod_batch", ctx.handle, C.byref(io), stream=stream)
    return out


def fm_modulate(ctx, samples, nsamples=None, deviation=None, centre=0.0, amplitude=1.0, phase0=None, phase_out=None,
                s16=False, stream=None, out=None):
    """mifsk_fm_modulate_batch, the FM modulator: I, Q = amplitude * cos, sin of an INTEGER phase that advances
    by rint((x * deviation + centre) * 2^48) per sample (2^48 to the turn), so pieces and the parallel scan on
    the device equal one serial loop bit for bit (tools/fm_ref.c).

    samples : float32 CUDA tensor [nstreams, stride] (or 1-D for one stream), what synthesize_batch returns;
              rows are 16-byte aligned, stride % 4 == 0
    nsamples: None (the rows' width), an int, or a torch.int32/uint32 CUDA tensor [nstreams]
    deviation, centre: turns per sample at x = 1.0 and at x = 0.0: fm_step(hertz, sample_rate)
    phase0  : None (0), or an int64/uint64 CUDA tensor [nstreams]: the phase before each row
    phase_out: None, or an int64/uint64 CUDA tensor [nstreams] that receives each row's last phase, the next
              piece's phase0 (it may be `phase0` itself)
    s16     : PCM16 output (when out is None)
    out     : the output tensor [nstreams, out_stride, 2], float32 or int16, its rows filling their stride.
              None: a new tensor, the width rounded up to whole 16-byte vectors, made on the launch stream.
    Returns out; a row is zero behind its length.  No synchronisation is performed."""
    torch = _torch()
    assert deviation is not None, "deviation: turns per sample at x = 1.0 (fm_step)"
    v = _row_view(torch, samples, dtypes=(torch.float32,), unit="floats")
    nstreams = v.nstreams
    lens = _row_lengths(torch, nsamples, nstreams, v.width, allow_int=True)
    if out is not None:
        s16 = out.dtype == torch.int16
    out, out_stride = _out_rows(torch, out, (nstreams, _whole(v.width, 4 if s16 else 2), 2),
                                torch.int16 if s16 else torch.float32, samples.device, stream,
                                dtypes=(torch.float32, torch.int16))
    io = _rows_io(_lib.FmModIO(), v, lens)
    io.out_kind = _kind(s16)
    io.d_out, io.out_stride = out.data_ptr(), out_stride
    io.deviation, io.centre, io.amplitude = float(deviation), float(centre), float(amplitude)
    for name, t in (("d_phase0", phase0), ("d_phase_out", phase_out)):
        if t is not None:
            assert t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.shape == (nstreams,) and t.is_contiguous(), \
                "%s: an int64/uint64 CUDA tensor [nstreams]" % name[2:]
            setattr(io, name, t.data_ptr())
    _call("mifsk_fm_modulate_batch", ctx.handle, C.byref(io), stream=stream)
    return out


def squelch_level(dbfs, window):
    """mifsk_fm_squelch_level: the energy of a window of `window` samples at dbfs (0 dBFS: |z| = 1), the
    unit of fm_squelch's levels."""
    return int(_lib.load().mifsk_fm_squelch_level(C.c_double(dbfs), C.c_uint32(window)))


def fm_squelch(ctx, iq, nsamples=None, window=None, open_db=None, close_db=None, hang=0, state=None, audio=None,
               span_cap=8, stream=None, out=None):
    """mifsk_fm_squelch_batch, the FM stage's power squelch (include/mifsk/squelch.h): the energy of every
    window of `window` samples of the I/Q rows as an integer, a gate with hysteresis and a hang time over the
    windows, the spans in which each row was keyed, and zeros over the discriminator's audio where the gate is
    closed -- all of it the same bits for a capture fed whole or in pieces (tools/squelch_ref.c).

    iq      : what fm_demod takes: CUDA tensor [nstreams, stride, 2], float32 or int16 (PCM16)
    nsamples: None (the rows' width), an int, or a torch.int32/uint32 CUDA tensor [nstreams]
    window  : B, samples per window, 1 .. 32768; windows lie on the grid of the samples since the state's start
    open_db, close_db: the gate opens at a window of open_db dBFS and counts one below close_db (None:
              open_db) as low: squelch_level(db, window) each
    hang    : low windows in a row that leave the gate open
    state   : None (all zero), or the "state" of a former call: taken as the start and overwritten with the
              end, so a live capture hands one tensor from piece to piece
    audio   : None, or fm_demod's output for the same rows, float32 [nstreams, audio_stride >= width]: zeroed
              where the gate of that moment is closed (it opens one window late), untouched elsewhere
    span_cap: spans stored per row (the count is the true one)
    out     : a former call's dict to write into; None: new tensors, made on the launch stream
    Returns {"energy": int64 [nstreams, win_stride] (the bits of uint64), "gate": uint8 [nstreams,
    win_stride], "nwindows": int32 [nstreams], "spans": int64 [nstreams, span_cap, 2] (first window, the
    window behind the last), "nspans": int32 [nstreams], "state": uint8 [nstreams, 32]
    (mifsk_fm_squelch_state)}; entry j of a row is window state.seen // window + j, entries behind nwindows and
    nspans are not written.  No synchronisation is performed."""
    torch = _torch()
    assert window is not None and open_db is not None, "window and open_db have no default"
    v = _row_view(torch, iq, cx=True, one_row=False, unit="elements")
    nstreams = v.nstreams
    lens = _row_lengths(torch, nsamples, nstreams, v.width, allow_int=True)
    kmax = v.stride if lens[0] is not None else min(lens[1], v.stride)
    win_stride = kmax // int(window) + 1
    level = [squelch_level(db, window) for db in (open_db, open_db if close_db is None else close_db)]
    if state is None:
        state = _new_outputs(torch, {"state": ((nstreams, 32), torch.uint8, 0)}, iq.device, stream)["state"]
    assert state.is_cuda and state.dtype == torch.uint8 and state.shape == (nstreams, 32) and state.is_contiguous(), \
        "state: a uint8 CUDA tensor [nstreams, 32]"
    if out is None:
        out = _new_outputs(torch, {"energy": ((nstreams, win_stride), torch.int64, None),
                                   "gate": ((nstreams, win_stride), torch.uint8, None),
                                   "nwindows": ((nstreams,), torch.int32, None),
                                   "spans": ((nstreams, int(span_cap), 2), torch.int64, None),
                                   "nspans": ((nstreams,), torch.int32, None)}, iq.device, stream)
    for name, dtype, tail in (("energy", torch.int64, ()), ("gate", torch.uint8, ())):
        _check_out_rows(torch, out[name], (dtype,), nstreams, tail)
    assert out["energy"].shape[1] == out["gate"].shape[1], "energy and gate rows are equally far apart"
    for name in ("nwindows", "nspans"):
        assert out[name].is_cuda and out[name].dtype == torch.int32 and out[name].shape == (nstreams,) \
            and out[name].is_contiguous(), "%s: an int32 CUDA tensor [nstreams]" % name
    spans = out["spans"]
    assert spans.is_cuda and spans.dtype == torch.int64 and spans.dim() == 3 and spans.shape[0] == nstreams \
        and spans.shape[2] == 2 and spans.is_contiguous(), "spans: an int64 CUDA tensor [nstreams, span_cap, 2]"
    io = _rows_io(_lib.FmSquelchIO(), v, lens)
    io.kind, io.window, io.hang = _kind(v.s16), int(window), int(hang)
    io.open_level, io.close_level = level
    io.d_state = io.d_state_out = state.data_ptr()
    io.d_energy, io.d_gate, io.win_stride = out["energy"].data_ptr(), out["gate"].data_ptr(), int(out["energy"].shape[1])
    io.d_nwindows, io.d_nspans = out["nwindows"].data_ptr(), out["nspans"].data_ptr()
    io.d_spans, io.span_cap = (spans.data_ptr() if spans.shape[1] else None), int(spans.shape[1])
    if audio is not None:
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2 and audio.shape[0] == nstreams \
            and audio.stride(1) == 1, "audio: fm_demod's float32 rows"
        io.d_audio, io.audio_stride = audio.data_ptr(), int(audio.stride(0)) if nstreams > 1 else int(audio.shape[1])
    _call("mifsk_fm_squelch_batch", ctx.handle, C.byref(io), stream=stream, errors=_EINVAL_IS_VALUE)
    return dict(out, state=state)


def demod_plan(ctx, cfg, nstreams, ring_exact=False, engine=None, nsamples=None):
    """mifsk_demod_plan[_ex]: what demod_batch would launch (kernel instantiation, engine,
    workgroup size, dynamic LDS per workgroup, workgroups per CU by LDS, LATTICE mode, and --
    for rows of `nsamples` samples; None: long ones -- the groups x time chunks a large batch
    is cut into)."""
    info = _lib.LaunchInfo()
    flags = _io_flags(ring_exact, engine)
    rc = _lib.load().mifsk_demod_plan_ex(ctx.handle, C.byref(cfg), int(nstreams),
                                         0xFFFFFFFF if nsamples is None else int(nsamples), flags, C.byref(info))
    if rc != 0:
        raise RuntimeError("mifsk_demod_plan failed: %d" % rc)
    d = _struct_dict(info)
    d["kernel"] = d["kernel"].decode()
    d["engine"] = "workgroup" if d["engine"] == _lib.IO_ENGINE_WORKGROUP else "wave"
    return d


def _time_split_params(chunk, warmup, chunks, engine, reject_all):
    p = _lib.TimeSplit()
    p.chunk = int(chunk or 0)
    p.warmup = int(warmup or 0)
    p.chunks = int(chunks or 0)
    p.flags = _io_flags(False, engine) | (_lib.TIME_SPLIT_REJECT_ALL if reject_all else 0)
    return p


def time_split_plan(cfg, nsamples, chunk=None, warmup=None, chunks=None, engine=None):
    """mifsk_time_split_plan_get: how demod_long would cut `nsamples` samples (host only)."""
    st = _lib.TimeSplitStats()
    rc = _lib.load().mifsk_time_split_plan_get(C.byref(cfg), int(nsamples),
                                               C.byref(_time_split_params(chunk, warmup, chunks, engine, False)),
                                               C.byref(st))
    if rc != 0:
        raise ValueError("mifsk_time_split_plan_get failed: %d" % rc)
    return _struct_dict(st)


def demod_long(ctx, cfg, samples, chunk=None, warmup=None, chunks=None, want=("bytes", "episodes"),
               frames_cap=None, episodes_cap=None, engine=None, reject_all=False, stream=None,
               rxnoise=0.0):
    """mifsk_demod_long: ONE long recording decoded across the whole chip by cutting it in
    time (DESIGN.md "cutting a stream in time"), bit for bit what demod_batch gives for it.

    samples: a 1-D torch.float32 CUDA tensor (16-byte aligned), or torch.int16 (PCM16: the chunks'
    rows are gathered straight from it, mifsk_demod_long_batch_s16 -- what ingest_s16 and this call
    give, without the float copy).  chunk / warmup / chunks: the planner's parameters (None: the
    library's choice).  reject_all: every speculative chunk is re-run (tests).  rxnoise: the
    --Xrxnoise factor (a float tensor is decoded as ingest_rxnoise on a copy; the caller's stays
    untouched).  Returns demod_batch's dict for a batch of one stream plus "stats" (the planner's
    figures and what verification accepted); synchronous."""
    torch = _torch()
    assert samples.is_cuda and samples.dtype in (torch.int16, torch.float32) and samples.dim() == 1
    assert samples.is_contiguous() and samples.data_ptr() % 16 == 0
    n = int(samples.shape[0])
    if samples.dtype == torch.float32 and rxnoise:
        with _on(torch, stream):
            samples = samples.clone()
        ingest_rxnoise(ctx, samples[None, :], rxnoise, stream=stream)
    # (a lone row's stride means nothing to the library; PCM16: the length rounded up to 8)
    out = _demod_long(torch, ctx, cfg, samples, (n + 7) & ~7, [n], rxnoise, want, frames_cap, episodes_cap,
                      _time_split_params(chunk, warmup, chunks, engine, reject_all), stream, lone=True)
    out["stats"] = out["stats"][0]
    return out


def time_split_plan_batch(cfg, nsamples_list, chunk=None, warmup=None, chunks=None, engine=None):
    """mifsk_time_split_plan_batch_get: how demod_long_batch would cut streams of these lengths with
    one chunk and one warmup (host only).  A list of dicts, one per stream."""
    lens = [int(n) for n in nsamples_list]
    arr = (C.c_uint64 * max(1, len(lens)))(*lens)
    st = (_lib.TimeSplitStats * max(1, len(lens)))()
    rc = _lib.load().mifsk_time_split_plan_batch_get(
        C.byref(cfg), arr, len(lens), C.byref(_time_split_params(chunk, warmup, chunks, engine, False)), st)
    if rc != 0:
        raise ValueError("mifsk_time_split_plan_batch_get failed: %d" % rc)
    return [_struct_dict(st[m]) for m in range(len(lens))]


def demod_long_batch(ctx, cfg, samples, nsamples=None, chunk=None, warmup=None, chunks=None,
                     want=("bytes", "episodes"), frames_cap=None, episodes_cap=None, engine=None,
                     reject_all=False, stream=None, rxnoise=0.0):
    """mifsk_demod_long_batch: a small batch of long recordings decoded across the whole chip by
    cutting all of them in time with one plan, bit for bit what demod_batch gives for the batch.

    samples: a 2-D contiguous torch.float32 CUDA tensor [nstreams, stride], stride % 4 == 0 (16-byte
    aligned), or torch.int16 with stride % 8 == 0 (PCM16, mifsk_demod_long_batch_s16: what
    ingest_s16 and this call give, without the float copy).  nsamples: a HOST sequence of ints, the
    streams' lengths (None: every row is full).  chunk / warmup / chunks / reject_all / rxnoise: as
    for demod_long.  Returns demod_batch's dict for nstreams streams plus "stats", a list of dicts
    (per stream: the plan and what verification accepted); the default caps come from the longest
    stream.  Synchronous."""
    torch = _torch()
    s16 = samples.dtype == torch.int16
    assert samples.is_cuda and (s16 or samples.dtype == torch.float32) and samples.dim() == 2
    assert samples.is_contiguous() and samples.data_ptr() % 16 == 0
    nstreams, width = (int(v) for v in samples.shape)
    if s16:
        assert nstreams >= 1 and width % 8 == 0, "PCM16 rows must be whole 16-byte vectors"
    else:
        assert nstreams >= 1 and width % 4 == 0, "rows must be whole float4s"
    lens = [width] * nstreams if nsamples is None else [int(n) for n in nsamples]
    assert len(lens) == nstreams and all(0 <= n <= width for n in lens)
    if not s16 and rxnoise:
        with _on(torch, stream):
            samples = samples.clone()
            dn = torch.tensor(lens, dtype=torch.int32, device=samples.device)
        ingest_rxnoise(ctx, samples, rxnoise, nsamples=dn, stream=stream)
    return _demod_long(torch, ctx, cfg, samples, width, lens, rxnoise, want, frames_cap, episodes_cap,
                       _time_split_params(chunk, warmup, chunks, engine, reject_all), stream)


def _demod_long(torch, ctx, cfg, samples, stride, lens, rxnoise, want, frames_cap, episodes_cap, params, stream,
                lone=False):
    """demod_long / demod_long_batch once the samples are checked: outputs, the C call, stats.  An
    int16 tensor goes to mifsk_demod_long_batch_s16, which adds rxnoise as it gathers the rows
    (floats: the callers have added it to a copy); a 1-D float tensor (`lone`) to mifsk_demod_long,
    whose one row need not be whole float4s; a float batch to mifsk_demod_long_batch."""
    lib = _lib.load()
    nstreams = len(lens)
    frames_cap, episodes_cap = _default_caps(cfg, max(lens), frames_cap, episodes_cap)
    out = _demod_outputs(torch, cfg, samples.device, nstreams, want, frames_cap, episodes_cap, stream)
    io = _result_io(out, nstreams, frames_cap, episodes_cap, _tensor_address)
    arr = (C.c_uint64 * nstreams)(*lens)
    st = (_lib.TimeSplitStats * nstreams)()
    head = (ctx.handle, C.byref(cfg), C.c_void_p(samples.data_ptr()))
    tail = (C.byref(params), C.byref(io), st, _stream_ptr(torch, stream))
    if samples.dtype == torch.int16:
        name, args = "mifsk_demod_long_batch_s16", head + (stride, arr, nstreams, C.c_float(rxnoise)) + tail
    elif lone:
        name, args = "mifsk_demod_long", head + (lens[0],) + tail
    else:
        name, args = "mifsk_demod_long_batch", head + (stride, arr, nstreams) + tail
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed: %d" % (name, rc))
    out["stats"] = [_struct_dict(st[m]) for m in range(nstreams)]
    return out


def results_to_host(out):
    """Copy a demod_batch() result to numpy (synchronises)."""
    res = {}
    for k, t in out.items():
        a = t.cpu().numpy()
        if k == "frames":
            a = a.view(FRAME_DTYPE).reshape(a.shape[0], a.shape[1])
        elif k == "episodes":
            a = a.view(EPISODE_DTYPE).reshape(a.shape[0], a.shape[1])
        elif k == "bits":
            a = a.view(np.uint64)
        res[k] = a
    return res


def find_frame_batch(ctx, cfg, samples, problems, stream=None):
    """N independent fsk_find_frame() problems over a flat CUDA float buffer.
    `problems` is a numpy array of SEARCH_DTYPE; returns numpy RESULT_DTYPE."""
    torch = _torch()
    lib = _lib.load()
    assert samples.is_cuda and samples.dtype == torch.float32
    problems = np.ascontiguousarray(problems, dtype=SEARCH_DTYPE)
    n = problems.shape[0]
    with _on(torch, stream):
        d_prob = torch.from_numpy(problems.view(np.uint8).reshape(-1).copy()).to(samples.device)
        d_res = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device=samples.device)
    rc = lib.mifsk_find_frame_batch(ctx.handle, C.byref(cfg), C.c_void_p(samples.data_ptr()),
                                    C.c_void_p(d_prob.data_ptr()), C.c_void_p(d_res.data_ptr()),
                                    n, _stream_ptr(torch, stream))
    if rc != 0:
        raise RuntimeError("mifsk_find_frame_batch failed: %d" % rc)
    return d_res.cpu().numpy().view(RESULT_DTYPE)


class LegacyPlan:
    """The reference's fsk.h API (include/fsk.h), called through the C ABI with
    host buffers exactly as src/minimodem.c calls it."""

    def __init__(self, sample_rate, f_mark, f_space, filter_bw):
        self._lib = _lib.load()
        self.p = self._lib.fsk_plan_new(sample_rate, f_mark, f_space, filter_bw)
        if not self.p:
            raise OSError(C.get_errno(), "fsk_plan_new failed")

    def __getattr__(self, name):
        return getattr(self.p.contents, name)

    def find_frame(self, samples, frame_nsamples, try_first, try_max, try_step, limit, expect):
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        bits, ampl, start = C.c_ulonglong(0), C.c_float(0), C.c_uint(0)
        conf = self._lib.fsk_find_frame(self.p, samples.ctypes.data, frame_nsamples, try_first,
                                        try_max, try_step, C.c_float(limit),
                                        expect.encode() if isinstance(expect, str) else expect,
                                        C.byref(bits), C.byref(ampl), C.byref(start))
        return float(conf), int(bits.value), float(ampl.value), int(start.value)

    def detect_carrier(self, samples, min_mag_threshold):
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        return int(self._lib.fsk_detect_carrier(self.p, samples.ctypes.data, samples.shape[0],
                                                C.c_float(min_mag_threshold)))

    def set_tones_by_bandshift(self, b_mark, b_shift):
        self._lib.fsk_set_tones_by_bandshift(self.p, b_mark, b_shift)

    def close(self):
        if self.p:
            self._lib.fsk_plan_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synthesize(cfg, words, lut=4096, amplitude=1.0, leading_silence=0, s16=False):
    """FSK audio for `words` exactly as `minimodem --tx --file` writes it
    (host-side generator, csrc/mifsk_tx.cpp).  Returns float32 numpy."""
    lib = _lib.load()
    words = np.ascontiguousarray(np.frombuffer(bytes(words), dtype=np.uint8)
                                 if isinstance(words, (bytes, bytearray)) else words,
                                 dtype=np.uint8)
    n = lib.mifsk_tx_synthesize(C.byref(cfg), words.ctypes.data, words.shape[0], lut,
                                C.c_float(amplitude), leading_silence, 1 if s16 else 0,
                                None, 0)
    if n < 0:
        raise ValueError("mifsk_tx_synthesize failed: %d" % n)
    out = np.zeros(n, dtype=np.float32)
    lib.mifsk_tx_synthesize(C.byref(cfg), words.ctypes.data, words.shape[0], lut,
                            C.c_float(amplitude), leading_silence, 1 if s16 else 0,
                            out.ctypes.data, n)
    return out


# ---------------------------------------------------------------------------
# multi-GPU: streams are independent, so ranks own contiguous stream ranges and
# the only exchange is a gather of decoded bytes (RCCL over xGMI on GPUs; the
# same code runs over gloo on CPU tensors in the tests).
# ---------------------------------------------------------------------------

def shard_range(nstreams, rank, world):
    """Contiguous, balanced [lo, hi) stream range of `rank`."""
    q, r = divmod(nstreams, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def gather_bytes(local_bytes, local_nbytes, dst=0, group=None):
    """Gather every rank's decoded bytes ([n_local, cap] uint8 + [n_local] int32
    counts) to rank `dst`.  Returns (bytes, nbytes) lists on dst, None elsewhere."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if world == 1:
        return [local_bytes], [local_nbytes]
    torch = _torch()
    shape = torch.tensor([local_bytes.shape[0], local_bytes.shape[1]], dtype=torch.int64,
                         device=local_bytes.device)
    shapes = [torch.zeros_like(shape) for _ in range(world)]
    dist.all_gather(shapes, shape, group=group)
    if rank == dst:
        bufs = [torch.empty((int(s[0]), int(s[1])), dtype=torch.uint8, device=local_bytes.device)
                for s in shapes]
        cnts = [torch.empty(int(s[0]), dtype=torch.int32, device=local_bytes.device)
                for s in shapes]
        bufs[dst] = local_bytes
        cnts[dst] = local_nbytes
        reqs = []
        for r in range(world):
            if r == dst:
                continue
            reqs.append(dist.P2POp(dist.irecv, bufs[r], r, group))
            reqs.append(dist.P2POp(dist.irecv, cnts[r], r, group))
        for w in dist.batch_isend_irecv(reqs):
            w.wait()
        return bufs, cnts
    reqs = [dist.P2POp(dist.isend, local_bytes.contiguous(), dst, group),
            dist.P2POp(dist.isend, local_nbytes.contiguous(), dst, group)]
    for w in dist.batch_isend_irecv(reqs):
        w.wait()
    return None, None


class _DevArray:
    """A device array the library owns, for torch.as_tensor (zero copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2, "strides": None}


class Pipeline(_Handle):
    """mifsk_pipeline_*: `depth` batches in flight behind the C ABI -- lanes of a context, a HIP
    stream and a completion event each, and (outputs(...)) one set of output arrays per lane,
    all owned by the library.  submit() is mifsk_demod_batch as the pipeline's next pass and
    returns its ticket; pass t runs on lane t % depth.  Results are those of demod_batch.

        pipe = M.Pipeline(device, depth=3)
        pipe.outputs(nstreams, frames_cap, want=("bytes",))
        t = pipe.submit(cfg, samples)            # ... more submits: they overlap on the device
        pipe.wait(t); out = pipe.result(t)       # dict of torch views of that pass's set
    """
    _destroy = "mifsk_pipeline_destroy"

    def __init__(self, device=-1, depth=3):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.mifsk_pipeline_create(C.byref(h), int(device), int(depth))
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_create failed: %d" % rc)
        self.handle = h
        info = _lib.PipelineInfo()
        self._lib.mifsk_pipeline_info_get(self.handle, C.byref(info))
        self.depth, self.depth_requested, self.hw_queues = int(info.depth), int(info.depth_requested), int(info.hw_queues)
        self._views = {}
        self._shape = None

    def info(self):
        info = _lib.PipelineInfo()
        self._lib.mifsk_pipeline_info_get(self.handle, C.byref(info))
        return _struct_dict(info)

    def outputs(self, nstreams, frames_cap, episodes_cap=8, want=("bytes",)):
        flags = (_lib.WANT_BYTES if "bytes" in want else 0) | (_lib.WANT_BITS if "bits" in want else 0) | \
            (_lib.WANT_FRAMES if "frames" in want else 0) | (_lib.WANT_EPISODES if "episodes" in want else 0)
        rc = self._lib.mifsk_pipeline_outputs_alloc(self.handle, int(nstreams), int(frames_cap),
                                                    int(episodes_cap), flags)
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_outputs_alloc failed: %d" % rc)
        self._views = {}
        self._shape = (int(nstreams), int(frames_cap), int(episodes_cap))

    def result(self, ticket):
        """torch views (no copy, no synchronisation) of the output set pass `ticket` writes"""
        lane = int(ticket) % self.depth
        if lane in self._views:
            return self._views[lane]
        torch = _torch()
        io = _lib.DemodIO()
        rc = self._lib.mifsk_pipeline_outputs_get(self.handle, int(ticket), C.byref(io))
        if rc != 0:
            raise RuntimeError("no output sets: call outputs() first (%d)" % rc)
        ns, fc, ec = self._shape
        dev = torch.device("cuda", torch.cuda.current_device())

        def view(ptr, shape, typestr, dtype):
            return torch.as_tensor(_DevArray(ptr, shape, typestr), device=dev).view(dtype) if ptr else None
        out = {"nframes": view(io.d_nframes, (ns,), "<i4", torch.int32),
               "nbytes": view(io.d_nbytes, (ns,), "<i4", torch.int32),
               "status": view(io.d_status, (ns,), "<i4", torch.int32)}
        if io.d_bytes:
            out["bytes"] = view(io.d_bytes, (ns, fc), "|u1", torch.uint8)
        if io.d_bits:
            out["bits"] = view(io.d_bits, (ns, fc), "<i8", torch.int64)
        if io.d_frames:
            out["frames"] = view(io.d_frames, (ns, fc, FRAME_DTYPE.itemsize), "|u1", torch.uint8)
        if io.d_episodes:
            out["episodes"] = view(io.d_episodes, (ns, int(io.episodes_cap), EPISODE_DTYPE.itemsize), "|u1", torch.uint8)
            out["nepisodes"] = view(io.d_nepisodes, (ns,), "<i4", torch.int32)
        self._views[lane] = out
        return out

    def submit(self, cfg, samples, nsamples=None, after="current", ring_exact=False, engine=None):
        """`after`: the torch stream the batch was produced on ("current": torch's current
        stream), or None when nothing has to be waited for."""
        torch = _torch()
        v = _row_view(torch, samples, dtypes=(torch.float32,), one_row=False)
        io = _rows_io(_lib.DemodIO(), v, _row_lengths(torch, nsamples, v.nstreams, v.width))
        io.flags = _io_flags(ring_exact, engine)
        if after == "current":
            after = torch.cuda.current_stream()
        prod = _lib.PIPELINE_NO_PRODUCER if after is None else C.c_void_p(after.cuda_stream)
        t = C.c_uint64(0)
        rc = self._lib.mifsk_pipeline_submit(self.handle, C.byref(cfg), C.byref(io), prod, C.byref(t))
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_submit failed: %d" % rc)
        return int(t.value)

    def next_ticket(self):
        return int(self._lib.mifsk_pipeline_next_ticket(self.handle))

    def wait(self, ticket):
        rc = self._lib.mifsk_pipeline_wait(self.handle, int(ticket))
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_wait(%d) failed: %d" % (ticket, rc))

    def join(self, ticket, stream=None):
        """torch stream `stream` (default: the current one) waits for pass `ticket` on the device"""
        torch = _torch()
        rc = self._lib.mifsk_pipeline_join(self.handle, int(ticket), _stream_ptr(torch, stream))
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_join(%d) failed: %d" % (ticket, rc))

    def drain(self):
        rc = self._lib.mifsk_pipeline_drain(self.handle)
        if rc != 0:
            raise RuntimeError("mifsk_pipeline_drain failed: %d" % rc)

    def stream(self, ticket):
        """the lane's HIP stream as a torch stream (what a gather of that pass's results is queued on)"""
        torch = _torch()
        return torch.cuda.ExternalStream(int(self._lib.mifsk_pipeline_stream(self.handle, int(ticket))))

    def close(self):
        if self.handle:
            self._views = {}
        super().close()


class ByteGatherer:
    """Overlapped gather of decoded bytes to rank 0 for a pipelined caller
    (bench.py): start(bytes, nbytes) posts one grouped send/recv -- every peer
    sends on its own link to the root (RCCL over xGMI on GPUs, gloo in the CPU
    tests) -- and returns the work handles; the caller waits on them before it
    reuses the buffers it passed.  On the root, received(r) is what peer r >= 1
    sent in the most recently STARTED gather, once its handles have been waited
    on; the root keeps `slots` sets of receive buffers (default two) and cycles
    through them like the caller does with its outputs, so that with that many
    gathers in flight an older one's data is not overwritten by a newer one's
    arrival (received(r, slot) names a set: the k-th start() fills set k % slots).

    cols: how many columns of the [nstreams, frames_cap] byte buffer can hold
    data at all (the caller knows its streams' lengths: mifsk_max_frames of the
    longest) -- only those are shipped, from a narrow staging copy made on the
    caller's stream (`slots` of them, used in turn like the caller's buffers).
    rows: streams per rank when the shards differ in size (default: all ranks
    hold as many as this one).
    loopback (world size 1 only): the one rank sends to ITSELF and receives it in the same
    group -- the whole transport (narrow staging copy, grouped isend/irecv, receive sets) on one
    GPU, which is how the N > 1 step structure is exercised where only one GPU is there;
    received(0) is then what it sent itself."""

    def __init__(self, dist, rank, world, cols=None, rows=None, slots=2, loopback=False):
        self.dist, self.rank, self.world = dist, rank, world
        self.cols, self.rows = cols, rows
        self.loopback = bool(loopback) and world == 1
        self.slots = max(2, int(slots))
        self._rx = [None] * self.slots
        self._tx = [None] * self.slots
        self._k = 0
        self._last = 0

    def bytes_per_peer(self, nstreams):
        """what one peer sends per step (bytes + counts)"""
        return int(nstreams) * (int(self.cols) if self.cols else 0) + 4 * int(nstreams)

    def start(self, local_bytes, local_nbytes):
        dist = self.dist
        if self.world == 1 and not self.loopback:
            return []
        cols = local_bytes.shape[1] if self.cols is None else min(int(self.cols), local_bytes.shape[1])
        self.cols = cols
        if self.loopback:
            torch = _torch()
            slot = self._k % self.slots
            self._k += 1
            self._last = slot
            if self._rx[slot] is None:
                self._rx[slot] = [(torch.empty((local_bytes.shape[0], cols), dtype=local_bytes.dtype, device=local_bytes.device),
                                   torch.empty_like(local_nbytes))]
                self._tx[slot] = torch.empty((local_bytes.shape[0], cols), dtype=local_bytes.dtype,
                                             device=local_bytes.device)
            self._tx[slot].copy_(local_bytes[:, :cols])
            rb, rn = self._rx[slot][0]
            ops = [dist.P2POp(dist.irecv, rb, 0), dist.P2POp(dist.irecv, rn, 0),
                   dist.P2POp(dist.isend, self._tx[slot], 0), dist.P2POp(dist.isend, local_nbytes, 0)]
            return dist.batch_isend_irecv(ops)
        if self.rank == 0:
            slot = self._k % self.slots
            self._k += 1
            self._last = slot
            if self._rx[slot] is None:
                torch = _torch()
                rows = self.rows or [local_bytes.shape[0]] * self.world
                self._rx[slot] = [(torch.empty((rows[r], cols), dtype=local_bytes.dtype, device=local_bytes.device),
                                   torch.empty((rows[r],), dtype=local_nbytes.dtype, device=local_nbytes.device))
                                  for r in range(1, self.world)]
            rx = self._rx[slot]
            ops = []
            for r in range(1, self.world):
                ops.append(dist.P2POp(dist.irecv, rx[r - 1][0], r))
                ops.append(dist.P2POp(dist.irecv, rx[r - 1][1], r))
        else:
            tx = local_bytes
            if cols != local_bytes.shape[1]:
                b = self._k % self.slots
                self._k += 1
                if self._tx[b] is None:
                    self._tx[b] = _torch().empty((local_bytes.shape[0], cols), dtype=local_bytes.dtype,
                                                 device=local_bytes.device)
                self._tx[b].copy_(local_bytes[:, :cols])
                tx = self._tx[b]
            ops = [dist.P2POp(dist.isend, tx, 0), dist.P2POp(dist.isend, local_nbytes, 0)]
        return dist.batch_isend_irecv(ops)

    def received(self, r, slot=None):
        return self._rx[self._last if slot is None else slot % self.slots][0 if self.loopback else r - 1]


class NativeGatherer(_Handle):
    """mifsk_gather_*: the same gather behind the C ABI (csrc/mifsk_gather.cpp: RCCL opened with
    dlopen, a communicator of the library's own).  Interface of ByteGatherer -- start(bytes,
    nbytes) enqueues ONE gather on torch's current stream and returns no handles (it is complete
    when that stream reaches the point behind the call); received(r, slot) on rank 0 is what peer
    r sent in the gather that filled set `slot` (default: the most recently started one), as torch
    views of the library's receive set.

    `dist`: a torch.distributed module whose default group carries rank 0's id to the others
    (None at world size 1); the communicator itself is made by the library."""
    _destroy = "mifsk_gather_destroy"

    def __init__(self, dist, rank, world, cols=None, rows=None, slots=2, loopback=False, device=-1):
        torch = _torch()
        self._lib = _lib.load()
        self.rank, self.world = int(rank), int(world)
        self.cols, self.rows = cols, rows
        self.loopback = bool(loopback) and world == 1
        self.slots = max(2, int(slots))
        self._tickets = []
        ident = None
        if world > 1 or self.loopback:
            buf = (C.c_ubyte * _lib.GATHER_ID_BYTES)()
            if rank == 0:
                rc = self._lib.mifsk_gather_unique_id(buf)
                if rc != 0:
                    raise RuntimeError("mifsk_gather_unique_id failed: %d" % rc)
            if world > 1:
                # (through the job's own process group: on the device for RCCL, on the host for gloo)
                dev = "cuda" if str(dist.get_backend()) == "nccl" else "cpu"
                t = torch.tensor(list(bytes(buf)), dtype=torch.uint8, device=dev)
                dist.broadcast(t, src=0)
                buf = (C.c_ubyte * _lib.GATHER_ID_BYTES)(*t.cpu().tolist())
            ident = buf
        h = C.c_void_p()
        rc = self._lib.mifsk_gather_create(C.byref(h), ident, self.rank, self.world, int(device), self.slots,
                                           _lib.GATHER_LOOPBACK if self.loopback else 0)
        if rc != 0:
            raise RuntimeError("mifsk_gather_create failed: %d" % rc)
        self.handle = h

    def info(self):
        gi = _lib.GatherInfo()
        self._lib.mifsk_gather_info_get(self.handle, C.byref(gi))
        return _struct_dict(gi)

    def bytes_per_peer(self, nstreams):
        return int(nstreams) * (int(self.cols) if self.cols else 0) + 4 * int(nstreams)

    def start(self, local_bytes, local_nbytes):
        torch = _torch()
        cols = local_bytes.shape[1] if self.cols is None else min(int(self.cols), local_bytes.shape[1])
        self.cols = cols
        assert local_bytes.dtype == torch.uint8 and local_nbytes.dtype == torch.int32 and local_bytes.stride(1) == 1
        rows = None
        if self.rows is not None and not self.loopback:
            rows = (C.c_int * self.world)(*[int(r) for r in self.rows])
        tk = C.c_uint64()
        rc = self._lib.mifsk_gather_start(self.handle, C.c_void_p(local_bytes.data_ptr()), int(local_bytes.stride(0)),
                                          C.c_void_p(local_nbytes.data_ptr()), int(local_bytes.shape[0]), cols, rows,
                                          _stream_ptr(torch, torch.cuda.current_stream()), C.byref(tk))
        if rc != 0:
            raise RuntimeError("mifsk_gather_start failed: %d" % rc)
        self._tickets.append(int(tk.value))
        del self._tickets[:-self.slots]
        return []

    def received(self, r, slot=None):
        torch = _torch()
        tk = self._tickets[-1]
        if slot is not None:
            tk = [t for t in self._tickets if t % self.slots == slot % self.slots][-1]
        pb, pn, rows, cols = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
        rc = self._lib.mifsk_gather_received(self.handle, tk, 0 if self.loopback else int(r), C.byref(pb), C.byref(pn),
                                             C.byref(rows), C.byref(cols))
        if rc != 0:
            raise RuntimeError("mifsk_gather_received failed: %d" % rc)
        dev = torch.device("cuda", torch.cuda.current_device())
        b = torch.as_tensor(_DevArray(pb.value, (rows.value, cols.value), "|u1"), device=dev)
        n = torch.as_tensor(_DevArray(pn.value, (rows.value,), "<i4"), device=dev)
        return b, n


DECODERS = {"ascii8": 0, "baudot": 1, "binary": 2, "callerid": 3, "uic-ground": 4, "uic-train": 5}
TEXT_PRINT_FILTER = 1
TEXT_QUIET = 2


class DataBits:
    """One databits decoder with its state (include/mifsk.h, reference
    src/databits.h:49-92): decode(bits, n_databits) -> bytes, reset()."""

    def __init__(self, decoder):
        self._lib = _lib.load()
        self.h = C.c_void_p()
        kind = DECODERS[decoder] if isinstance(decoder, str) else int(decoder)
        rc = self._lib.mifsk_databits_create(C.byref(self.h), kind)
        if rc != 0:
            raise ValueError("mifsk_databits_create -> %d" % rc)
        self._buf = C.create_string_buffer(4096)

    def reset(self):
        self._lib.mifsk_databits_reset(self.h)

    def decode(self, bits, n_databits):
        n = self._lib.mifsk_databits_decode(self.h, self._buf, 4096, int(bits), int(n_databits))
        return self._buf.raw[:n]

    def __del__(self):
        try:
            if self.h:
                self._lib.mifsk_databits_destroy(self.h)
                self.h = None
        except Exception:
            pass


def stream_text(cfg, bits, episodes, print_filter=False, quiet=False, b_mark=None):
    """What minimodem writes for one stream: (stdout bytes, stderr str) from the
    frame data bits (numpy uint64, loop order) and its episodes (EPISODE_DTYPE);
    host post-pass mifsk_stream_text (reference src/minimodem.c:253-291,1336-1461).
    The "### CARRIER ... @ f Hz" line is printed from each episode's own b_mark
    (`b_mark` is accepted for callers of the older signature and ignored)."""
    lib = _lib.load()
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    episodes = np.ascontiguousarray(episodes, dtype=EPISODE_DTYPE)
    flags = (TEXT_PRINT_FILTER if print_filter else 0) | (TEXT_QUIET if quiet else 0)
    out_cap = 64 + 320 * max(1, bits.shape[0])
    err_cap = 256 + 512 * max(1, episodes.shape[0])
    out = C.create_string_buffer(out_cap)
    err = C.create_string_buffer(err_cap)
    nout, nerr = C.c_size_t(0), C.c_size_t(0)
    rc = lib.mifsk_stream_text(C.byref(cfg), bits.ctypes.data, bits.shape[0],
                               episodes.ctypes.data, episodes.shape[0], flags,
                               out, out_cap, C.byref(nout), err, err_cap, C.byref(nerr))
    if rc != 0:
        raise RuntimeError("mifsk_stream_text -> %d" % rc)
    return out.raw[:nout.value], err.raw[:nerr.value].decode("latin-1")


def wav_parse(data):
    """RIFF/WAVE header of a `--rx --file` input (mifsk_wav_parse): dict with
    sample_rate, channels, bits_per_sample, is_float, data_offset, nframes."""
    info = _lib.WavInfo()
    rc = _lib.load().mifsk_wav_parse(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError("mifsk_wav_parse -> %d" % rc)
    return _struct_dict(info)


def ingest_s16(ctx, pcm, nsamples=None, rxnoise=0.0, stride=None, stream=None):
    """libsndfile's S16 -> float conversion (+ the --Xrxnoise term) on the device:
    pcm is a torch.int16 CUDA tensor [nstreams, width]; returns float32
    [nstreams, stride] (stride defaults to width rounded up to a multiple of 4)."""
    torch = _torch()
    v = _row_view(torch, pcm, dtypes=(torch.int16,), one_row=False, whole=False)
    d_nsamples, width = _row_lengths(torch, nsamples, v.nstreams, v.width)
    if stride is None:
        stride = (width + 3) & ~3
    out, stride = _out_rows(torch, None, (v.nstreams, stride), torch.float32, pcm.device, stream)
    _call("mifsk_ingest_s16", ctx.handle, C.c_void_p(pcm.data_ptr()), v.stride, C.c_void_p(out.data_ptr()), stride,
          C.c_void_p(d_nsamples), width, v.nstreams, C.c_float(rxnoise), stream=stream)
    return out


def ingest_rxnoise(ctx, samples, rxnoise, nsamples=None, stream=None):
    """The --Xrxnoise term applied in place to float32 CUDA samples [nstreams, stride]."""
    torch = _torch()
    v = _row_view(torch, samples, dtypes=(torch.float32,), one_row=False, whole=False)
    d_nsamples, width = _row_lengths(torch, nsamples, v.nstreams, v.width)
    _call("mifsk_ingest_rxnoise_f32", ctx.handle, C.c_void_p(samples.data_ptr()), v.stride, C.c_void_p(d_nsamples),
          width, v.nstreams, C.c_float(rxnoise), stream=stream)
    return samples


def synthesize_batch(ctx, cfg, words, nwords=None, lut=4096, amplitude=1.0, leading_silence=0,
                     s16=False, stride=None, stream=None):
    """The transmitter for a whole batch on the device (mifsk_tx_synthesize_batch):
    words is a torch.uint8 CUDA tensor [nstreams, max_words]; nwords / leading_silence
    may be int32 CUDA tensors [nstreams] or scalars.  Returns (samples float32
    [nstreams, stride], lengths int32 [nstreams]); rows are zero after their length."""
    torch = _torch()
    v = _row_view(torch, words, dtypes=(torch.uint8,), one_row=False, whole=False)
    nstreams = v.nstreams
    d_nwords, nw_u = _row_lengths(torch, nwords, nstreams, v.width, allow_int=True)
    d_lead, ls_u = _row_lengths(torch, leading_silence, nstreams, 0, allow_int=True)
    if stride is None:
        max_lead = int(leading_silence.max()) if d_lead and nstreams else ls_u
        max_words = int(nwords.max()) if d_nwords and nstreams else nw_u
        one = np.zeros(max(1, max_words), np.uint8)
        n = _lib.load().mifsk_tx_synthesize(C.byref(cfg), one.ctypes.data, max_words, lut,
                                            C.c_float(amplitude), max_lead, 0, None, 0)
        stride = (max(int(n), 4) + 3) & ~3
    res = _new_outputs(torch, {"out": ((nstreams, stride), torch.float32, None), "lens": ((nstreams,), torch.int32, 0)},
                       words.device, stream)
    out, lens = res["out"], res["lens"]
    _call("mifsk_tx_synthesize_batch", ctx.handle, C.byref(cfg), C.c_void_p(words.data_ptr()), v.stride,
          C.c_void_p(d_nwords), nw_u, nstreams, int(lut), C.c_float(amplitude), C.c_void_p(d_lead), ls_u,
          1 if s16 else 0, C.c_void_p(out.data_ptr()), stride, C.c_void_p(lens.data_ptr()), stream=stream)
    return out, lens


_PINNED = {}


def host_alloc(shape, dtype=np.float32):
    """A numpy array in page-locked host memory (mifsk_host_alloc): input rows the host entry
    points copy by DMA from where they are.  Release with host_free()."""
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    ptr = _lib.load().mifsk_host_alloc(max(nbytes, 1))
    if not ptr:
        raise MemoryError("mifsk_host_alloc(%d)" % nbytes)
    buf = (C.c_char * max(nbytes, 1)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    _PINNED[arr.ctypes.data] = ptr
    return arr


def host_free(arr):
    ptr = _PINNED.pop(arr.ctypes.data, None)
    if ptr:
        _lib.load().mifsk_host_free(ptr)


def demod_batch_host(ctx, cfg, samples, nsamples=None, frames_cap=None, episodes_cap=8,
                     ring_exact=False, want=("bytes", "bits", "frames", "episodes"), rxnoise=0.0,
                     stats=False, engine=None):
    """mifsk_demod_batch_host[_ex]: the whole batch from HOST memory in one call -- chunks of
    streams cross PCIe on a copy stream while the chunk before is demodulated and the one
    before that is copied back.  samples is a float32 numpy array [nstreams, stride], or
    int16 (PCM16 as a WAV file holds it: MIFSK_IO_HOST_S16, converted on the device); rows
    from host_alloc() are copied by DMA from where they are.  Returns a dict of numpy arrays
    (plus "stats" when asked).  `ctx` may be a list of Contexts (one per GPU):
    mifsk_demod_batch_host_multi shards the streams over them inside this one process."""
    lib = _lib.load()
    s16 = samples.dtype == np.int16
    if not (s16 or (samples.dtype == np.float32 and samples.flags.c_contiguous)):
        samples = np.ascontiguousarray(samples, dtype=np.float32)
    assert samples.ndim == 2 and samples.flags.c_contiguous
    nstreams, stride = samples.shape
    if frames_cap is None:
        frames_cap = max_frames(cfg, stride)
    res = _numpy_outputs(nstreams, want, frames_cap, episodes_cap)
    io = _result_io(res, nstreams, frames_cap, episodes_cap, _array_address)
    io.d_samples = samples.ctypes.data
    io.stream_stride = stride
    if nsamples is not None:
        nsamples = np.ascontiguousarray(nsamples, dtype=np.uint32)
        io.d_nsamples = nsamples.ctypes.data
    io.nsamples = stride
    io.flags = _io_flags(ring_exact, engine) | (_lib.IO_HOST_S16 if s16 else 0)
    if isinstance(ctx, (list, tuple)):
        assert not s16 and not rxnoise
        handles = (C.c_void_p * len(ctx))(*[c.handle for c in ctx])
        rc = lib.mifsk_demod_batch_host_multi(handles, len(ctx), C.byref(cfg), C.byref(io))
    else:
        st = _lib.HostStats()
        rc = lib.mifsk_demod_batch_host_ex(ctx.handle, C.byref(cfg), C.byref(io), C.c_float(rxnoise),
                                           C.byref(st))
        if stats:
            res["stats"] = _struct_dict(st, drop_reserved=True)
    if rc != 0:
        raise RuntimeError("mifsk_demod_batch_host failed: %d" % rc)
    return res


def demod_long_host(ctx, cfg, arrays, chunk=None, warmup=None, chunks=None,
                    want=("bytes", "bits", "frames", "episodes"), rxnoise=0.0, engine=None, reject_all=False,
                    stats=False, frames_cap=None, episodes_cap=None):
    """mifsk_demod_long_batch_host: a few long recordings in HOST memory decoded across the whole
    chip by cutting them in time.  arrays: a list of 1-D numpy arrays, all int16 (PCM16 as a WAV
    file holds it: it crosses the bus as 16-bit and the chunks' rows are gathered straight from it)
    or all float32; arrays from host_alloc() are copied by DMA from where they are.  chunk / warmup
    / chunks / reject_all: as for demod_long.  Returns numpy results as demod_batch_host does, plus
    "stats" (a list of per-stream dicts: the plan and what verification accepted) and, with
    stats=True, "host_stats"."""
    lib = _lib.load()
    arrays = list(arrays)
    assert arrays and all(a.ndim == 1 for a in arrays)
    s16 = arrays[0].dtype == np.int16
    assert all(a.dtype == (np.int16 if s16 else np.float32) and a.flags.c_contiguous for a in arrays), \
        "all int16 or all float32, contiguous"
    nstreams = len(arrays)
    lens = [int(a.shape[0]) for a in arrays]
    frames_cap, episodes_cap = _default_caps(cfg, max(lens), frames_cap, episodes_cap)
    res = _numpy_outputs(nstreams, want, frames_cap, episodes_cap)
    io = _result_io(res, nstreams, frames_cap, episodes_cap, _array_address)
    rows = (C.c_void_p * nstreams)(*[a.ctypes.data for a in arrays])
    arr = (C.c_uint64 * nstreams)(*lens)
    st = (_lib.TimeSplitStats * nstreams)()
    hst = _lib.HostStats()
    rc = lib.mifsk_demod_long_batch_host(ctx.handle, C.byref(cfg), rows, arr, nstreams,
                                         _lib.IO_HOST_S16 if s16 else 0, C.c_float(rxnoise),
                                         C.byref(_time_split_params(chunk, warmup, chunks, engine, reject_all)),
                                         C.byref(io), st, C.byref(hst))
    if rc != 0:
        raise RuntimeError("mifsk_demod_long_batch_host failed: %d" % rc)
    res["stats"] = [_struct_dict(st[m]) for m in range(nstreams)]
    if stats:
        res["host_stats"] = _struct_dict(hst, drop_reserved=True)
    return res


def demod_files(ctx, paths, baudmode="1200", rxnoise=0.0, ring_exact=False, want_frames=False,
                engine=None, time_split=False, **opts):
    """mifsk_demod_files: `minimodem --rx --file F <baudmode>` for a list of WAV files (PCM16 or
    float32, any mix of lengths and sample rates) as batches on the device: raw samples are
    pread() into pinned memory by worker threads, cross PCIe as they are in the file and are
    converted there.  Returns (list of per-file dicts, stats dict); a file that could not be
    decoded has {"error": -errno}.  Each dict carries the RxConfig it was decoded with.
    time_split: True, or a dict with any of chunk / warmup / chunks / reject_all, decodes every
    (sample rate, sample format) group of files as long recordings cut in time across the chip
    (mifsk_demod_files_long); each decoded file's dict then carries "time_split", its plan and
    verification figures.  Not with ring_exact."""
    if time_split is not False and time_split is not None and ring_exact:
        raise ValueError("time_split cannot be combined with ring_exact")
    lib = _lib.load()
    a = ModemArgs()
    lib.mifsk_modem_args_default(C.byref(a))
    a.baudmode = str(baudmode).encode()
    if "sync_byte" in opts:
        a.have_sync_byte = 1
    for k, v in opts.items():
        if not hasattr(a, k):
            raise TypeError("unknown modem option %r" % k)
        setattr(a, k, v)
    enc = [os.fsencode(p) for p in paths]
    arr = (C.c_char_p * max(1, len(enc)))(*enc)
    flags = _io_flags(ring_exact, engine) | (_lib.FILES_WANT_FRAMES if want_frames else 0)
    h = C.c_void_p()
    split = time_split is not False and time_split is not None
    if split:
        kw = dict(time_split) if isinstance(time_split, dict) else {}
        unknown = set(kw) - {"chunk", "warmup", "chunks", "reject_all"}
        if unknown:
            raise TypeError("unknown time_split option(s) %s" % sorted(unknown))
        p = _time_split_params(kw.get("chunk"), kw.get("warmup"), kw.get("chunks"), None, kw.get("reject_all", False))
        rc = lib.mifsk_demod_files_long(ctx.handle, C.byref(a), arr, len(enc), C.c_float(rxnoise), flags,
                                        C.byref(p), C.byref(h))
    else:
        rc = lib.mifsk_demod_files(ctx.handle, C.byref(a), arr, len(enc), C.c_float(rxnoise), flags, C.byref(h))
    if rc != 0:
        if h:
            lib.mifsk_files_free(h)
        raise RuntimeError("mifsk_demod_files%s failed: %d" % ("_long" if split else "", rc))
    out = []
    try:
        for i in range(lib.mifsk_files_count(h)):
            fr = lib.mifsk_files_get(h, i).contents
            d = {"error": fr.error, "path": paths[i],
                 "info": _struct_dict(fr.info)}
            if fr.error == 0:
                cfg = RxConfig()
                C.memmove(C.byref(cfg), fr.cfg, C.sizeof(RxConfig))
                d["cfg"] = cfg
                d["status"] = fr.status
                d["carrier_band"] = fr.carrier_band
                d["bits"] = np.ctypeslib.as_array((C.c_uint64 * max(1, fr.nframes)).from_address(fr.bits))[:fr.nframes].copy()
                d["bytes"] = bytes((C.c_uint8 * max(1, fr.nbytes)).from_address(fr.bytes))[:fr.nbytes]
                d["episodes"] = np.frombuffer(
                    (C.c_char * (max(1, fr.nepisodes) * EPISODE_DTYPE.itemsize)).from_address(fr.episodes),
                    dtype=EPISODE_DTYPE)[:fr.nepisodes].copy()
                if fr.frames:
                    d["frames"] = np.frombuffer(
                        (C.c_char * (max(1, fr.nframes) * FRAME_DTYPE.itemsize)).from_address(fr.frames),
                        dtype=FRAME_DTYPE)[:fr.nframes].copy()
                if split:
                    ts = lib.mifsk_files_time_split(h, i)
                    if ts:
                        d["time_split"] = _struct_dict(ts.contents)
            out.append(d)
        st = lib.mifsk_files_stats(h).contents
        stats = _struct_dict(st, drop_reserved=True)
    finally:
        lib.mifsk_files_free(h)
    return out, stats


# ---------------------------------------------------------------------------
# streams that arrive in pieces (mifsk_demod_slab)
# ---------------------------------------------------------------------------

STATE_DTYPE = np.dtype([("base", "<u8"), ("rp", "<u8"), ("carrier_nsamples", "<u8"),
                        ("nframes_total", "<u8"), ("advance", "<u4"), ("flags", "<u4"),
                        ("confidence_total", "<f4"), ("amplitude_total", "<f4"),
                        ("nframes_decoded", "<u4"), ("noconfidence", "<u4"),
                        ("track_amplitude", "<f4"), ("peak_confidence", "<f4"),
                        ("carrier_band", "<i4"), ("first_band", "<i4"), ("b_mark", "<u4"),
                        ("ep_b_mark", "<u4"), ("ep_first", "<u4"), ("nbytes_total", "<u4"),
                        ("nepisodes_total", "<u4"), ("status", "<u4")])
assert STATE_DTYPE.itemsize == 96
STATE_FINISHED = 4
# C struct name -> the numpy dtype that mirrors it (the ctypes mirrors: _lib.STRUCTS)
DTYPES = {"mifsk_frame": FRAME_DTYPE, "mifsk_episode": EPISODE_DTYPE, "mifsk_stream_state": STATE_DTYPE,
          "mifsk_search": SEARCH_DTYPE, "mifsk_search_result": RESULT_DTYPE}


class SlabSession:
    """A batch of streams fed in pieces (mifsk_demod_slab; reference: the half-buffer refills of
    src/minimodem.c:1144-1174).  feed(new_samples, final) appends each stream's new samples
    behind what the receive loop has not passed yet, runs the loop as far as the data allows
    and returns the frames / bytes / episodes that this made; the loop's state lives in device
    memory between calls, the unconsumed tail of every stream on the host.  Whatever the cuts,
    the concatenated output is the single call's, bit for bit."""

    def __init__(self, ctx, cfg, nstreams, episodes_cap=16, engine=None, ring_exact=False):
        """engine: None (the library chooses, as demod_batch does), "wave" or "workgroup"; may
        be changed between feeds (self.engine): the state record is the same for both.
        ring_exact: the reference's buffer semantics (mifsk_demod_slab_ring): its samplebuf
        cells persist in device memory between the feeds."""
        torch = _torch()
        self.ctx, self.cfg, self.n = ctx, cfg, int(nstreams)
        self.engine = engine
        self.ring = None
        if ring_exact:
            nf = int(_lib.load().mifsk_ring_floats(C.byref(cfg)))
            assert nf > 0
            self.ring = torch.zeros((self.n, nf), dtype=torch.float32, device="cuda")
        self.episodes_cap = episodes_cap
        self.state = torch.zeros((self.n, STATE_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.origin = np.zeros(self.n, np.uint64)
        self.tail = [np.zeros(0, np.float32) for _ in range(self.n)]

    def feed(self, new, final=False, stream=None):
        torch = _torch()
        assert len(new) == self.n
        for i, x in enumerate(new):
            if x is not None and len(x):
                self.tail[i] = np.concatenate([self.tail[i], np.asarray(x, np.float32)])
        if stream is not None:
            # (state and ring were made -- and on the first feed zero-filled -- on the stream that
            # was current then: this stream starts behind it)
            stream.wait_stream(torch.cuda.current_stream())
        width = (max([len(t) for t in self.tail] + [4]) + 3) & ~3
        host = np.zeros((self.n, width), np.float32)
        lens = np.zeros(self.n, np.int32)
        for i, t in enumerate(self.tail):
            host[i, :len(t)] = t
            lens[i] = len(t)
        with _on(torch, stream):
            d = torch.from_numpy(host).cuda()
            dl = torch.from_numpy(lens).cuda()
            do = torch.from_numpy(self.origin.view(np.int64).copy()).cuda()
        v = _row_view(torch, d, dtypes=(torch.float32,), one_row=False)
        fc = max_frames(self.cfg, width)
        out = _demod_outputs(torch, self.cfg, d.device, self.n, ("bytes", "bits", "frames", "episodes", "carrier_band"),
                             fc, self.episodes_cap, stream)
        io = _rows_io(_result_io(out, self.n, fc, self.episodes_cap, _tensor_address), v,
                      _row_lengths(torch, dl, self.n, width))
        io.flags = _io_flags(False, self.engine)
        args = (self.ctx.handle, C.byref(self.cfg), C.byref(io), C.c_void_p(self.state.data_ptr()), C.c_void_p(do.data_ptr()))
        if self.ring is not None:
            io.flags = _lib.IO_RING_EXACT
            _call("mifsk_demod_slab_ring", *args, C.c_void_p(self.ring.data_ptr()), 1 if final else 0, stream=stream)
        else:
            _call("mifsk_demod_slab", *args, 1 if final else 0, stream=stream)
        torch.cuda.synchronize()
        res = results_to_host(out)
        st = self.state.cpu().numpy().view(STATE_DTYPE).reshape(self.n)
        for i in range(self.n):
            drop = int(st["base"][i]) - int(self.origin[i])
            if drop > 0:
                self.tail[i] = self.tail[i][drop:]
                self.origin[i] = st["base"][i]
        res["state"] = st.copy()
        return res


class Session(_Handle):
    """mifsk_session_*: SlabSession's job behind the C ABI (csrc/mifsk_session.cpp) -- the
    unconsumed tails, origins, loop state, RING cells and output arrays are the library's.
    feed(new, final) returns one dict per stream of what THIS feed made of it (numpy copies).

    resident=True (MIFSK_SESSION_RESIDENT) keeps the tails in device memory: a feed uploads only
    the new samples.  Such a session takes `new` as a list of numpy float32 or int16 (PCM16)
    arrays, all of one kind, None for "nothing new" -- or as one CUDA torch.float32 / torch.int16
    tensor [n, k] whose row i holds stream i's nsamples[i] new samples (default: k for every
    stream), produced on the current torch stream.  rxnoise is the --Xrxnoise term, added to the
    new samples on the device."""
    _destroy = "mifsk_session_destroy"

    def __init__(self, ctx, cfg, nstreams, engine=None, ring_exact=False, want_frames=True, resident=False):
        self._lib = _lib.load()
        self.n = int(nstreams)
        self.resident = bool(resident)
        flags = _io_flags(ring_exact, engine) | (_lib.SESSION_WANT_FRAMES if want_frames else 0)
        flags |= _lib.SESSION_RESIDENT if resident else 0
        h = C.c_void_p()
        rc = self._lib.mifsk_session_create(C.byref(h), ctx.handle, C.byref(cfg), self.n, flags)
        if rc != 0:
            raise RuntimeError("mifsk_session_create failed: %d" % rc)
        self.handle = h

    def _feed_host(self, new, final):
        keep = [np.ascontiguousarray(x, dtype=np.float32) if x is not None and len(x) else None for x in new]
        ptrs = (C.c_void_p * self.n)(*[k.ctypes.data if k is not None else None for k in keep])
        cnts = (C.c_uint32 * self.n)(*[len(k) if k is not None else 0 for k in keep])
        return self._lib.mifsk_session_feed(self.handle, ptrs, cnts, 1 if final else 0), "mifsk_session_feed"

    def _feed_resident(self, new, final, rxnoise, nsamples):
        if hasattr(new, "is_cuda"):
            torch = _torch()
            if not new.is_cuda or new.dim() != 2 or new.shape[0] != self.n or new.dtype not in (torch.float32, torch.int16):
                raise ValueError("a resident session takes a CUDA float32 or int16 tensor [nstreams, k]")
            if new.shape[1] > 1 and new.stride(1) != 1:
                raise ValueError("the samples of a row must be contiguous")
            kind = _lib.FEED_S16 if new.dtype == torch.int16 else _lib.FEED_F32
            k = int(new.shape[1])
            lens = [k] * self.n if nsamples is None else [int(v) for v in nsamples]
            if len(lens) != self.n or any(v < 0 or v > k for v in lens):
                raise ValueError("nsamples: one count per stream, none beyond the tensor's width")
            cnts = (C.c_uint32 * self.n)(*lens)
            stride = int(new.stride(0)) if self.n > 1 else k
            rc = self._lib.mifsk_session_feed_device(
                self.handle, C.c_void_p(new.data_ptr() if k else None), stride, cnts, kind, C.c_float(rxnoise),
                1 if final else 0, _stream_ptr(torch, None))
            return rc, "mifsk_session_feed_device"
        if nsamples is not None:
            raise ValueError("nsamples goes with a device tensor")
        assert len(new) == self.n
        kinds = {np.asarray(x).dtype for x in new if x is not None and len(x)}
        if not kinds <= {np.dtype(np.float32), np.dtype(np.int16)} or len(kinds) > 1:
            raise ValueError("a resident session takes float32 or int16 pieces, all of one kind")
        dtype = kinds.pop() if kinds else np.dtype(np.float32)
        keep = [np.ascontiguousarray(x, dtype=dtype) if x is not None and len(x) else None for x in new]
        ptrs = (C.c_void_p * self.n)(*[k.ctypes.data if k is not None else None for k in keep])
        cnts = (C.c_uint32 * self.n)(*[len(k) if k is not None else 0 for k in keep])
        kind = _lib.FEED_S16 if dtype == np.int16 else _lib.FEED_F32
        rc = self._lib.mifsk_session_feed_ex(self.handle, ptrs, cnts, kind, C.c_float(rxnoise), 1 if final else 0)
        return rc, "mifsk_session_feed_ex"

    def feed(self, new, final=False, rxnoise=0.0, nsamples=None):
        if self.resident:
            rc, what = self._feed_resident(new, final, float(rxnoise), nsamples)
        else:
            if rxnoise != 0.0 or nsamples is not None or hasattr(new, "is_cuda"):
                raise ValueError("rxnoise, nsamples and device tensors need Session(..., resident=True)")
            assert len(new) == self.n
            rc, what = self._feed_host(new, final)
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))
        out = []
        for i in range(self.n):
            r = self._lib.mifsk_session_get(self.handle, i).contents

            def arr(ptr, count, dtype):
                if not ptr or not count:
                    return np.zeros(0, dtype)
                nb = count * np.dtype(dtype).itemsize
                return np.frombuffer(C.string_at(ptr, nb), dtype=dtype).copy()
            out.append({"frames": arr(r.frames, r.nframes, FRAME_DTYPE), "bits": arr(r.bits, r.nframes, np.uint64),
                        "bytes": arr(r.bytes, r.nbytes, np.uint8).tobytes(),
                        "episodes": arr(r.episodes, r.nepisodes, EPISODE_DTYPE), "status": int(r.status),
                        "carrier_band": int(r.carrier_band), "consumed": int(r.consumed), "finished": bool(r.finished),
                        "pending": int(self._lib.mifsk_session_pending(self.handle, i))})
        return out

    def info(self):
        """mifsk_session_info: resident, feeds, row_capacity, device_bytes, h2d_bytes_last / _total"""
        info = _lib.SessionInfo()
        rc = self._lib.mifsk_session_info_get(self.handle, C.byref(info))
        if rc != 0:
            raise RuntimeError("mifsk_session_info_get failed: %d" % rc)
        return _struct_dict(info, drop_reserved=True)


def scan_plan(cfg, kind):
    """mifsk_scan_plan_get: the shared-segment plan of scan `kind` (2 * fine + carrier) as a dict
    of numpy arrays, or None when that scan correlates every window by itself."""
    sp = _lib.ScanPlan()
    rc = _lib.load().mifsk_scan_plan_get(C.byref(cfg), int(kind), C.byref(sp))
    if rc != 0:
        raise RuntimeError("mifsk_scan_plan_get -> %d" % rc)
    if not sp.valid:
        return None
    n, w = sp.nseg, sp.nwin
    return {"nseg": n, "npass": sp.npass, "nwin": w, "span_hi": sp.span_hi,
            "pass_len": list(sp.pass_len), "pass_min": list(sp.pass_min), "bound_c": sp.bound_c,
            "seg_rel": np.array(sp.seg_rel[:n]), "seg_len": np.array(sp.seg_len[:n]),
            "slot_seg": np.array(sp.slot_seg[:64 * sp.npass]),
            "win_first": np.array(sp.win_first[:w]), "win_count": np.array(sp.win_count[:w])}
