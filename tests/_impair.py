"""What tests/test_impair_args.py, tests/test_impair_ref.py and tests/test_gpu_impair.py share: the
channel model's host restatement (tools/impair_ref.c) and the device's own header compiled for the
host (tools/gauss_check.c, which includes minimodem_amd/csrc/mifsk_gauss.h), both as temporary
shared objects (_phase.ref_lib), and the words at the transform's corners."""
import ctypes as C

import numpy as np

import _phase
from _phase import F32, ROOT, same_bits  # noqa: F401 (for the tests)

F32K, S16K = 0, 1                       # MIFSK_FEED_F32 / MIFSK_FEED_S16
U64, VP = C.c_uint64, C.c_void_p


def ref_lib():
    """tools/impair_ref.c as a shared object"""
    return _phase.ref_lib("impair_ref", (
        ("impair_ref_philox", None, (VP, VP, VP)),
        ("impair_ref_words", None, (VP, U64, VP, VP)),
        ("impair_ref_z", C.c_double, (U64, U64, U64)),
        ("impair_ref_field", None, (U64, U64, U64, U64, VP)),
        ("impair_ref_rows", None, (VP, U64, VP, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, VP, U64, U64, U64, U64,
                                   VP, VP, VP, C.c_float, C.c_float, C.c_float))))


def header_lib():
    """minimodem_amd/csrc/mifsk_gauss.h compiled for the host (tools/gauss_check.c)"""
    return _phase.ref_lib("gauss_check", (
        ("gauss_check_words", None, (VP, U64, VP, VP)),
        ("gauss_check_field", None, (U64, U64, U64, U64, VP, VP)),
        ("gauss_check_sweep", None, (U64, VP))))


def ref_philox(counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.empty(4, np.uint32)
    ref_lib().impair_ref_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return out


def _words(fn, words):
    words = np.ascontiguousarray(words, np.uint32)
    assert words.ndim == 2 and words.shape[1] == 2
    rcs, z = np.empty((words.shape[0], 3), np.float64), np.empty((words.shape[0], 2), np.float64)
    fn(words.ctypes.data, words.shape[0], rcs.ctypes.data, z.ctypes.data)
    return rcs, z


def ref_words(words):
    """uint32 [n, 2] -> (float64 [n, 3]: R(w[0]), C(w[1]), S(w[1]); float64 [n, 2]: R C, R S) by the restatement"""
    return _words(ref_lib().impair_ref_words, words)


def header_words(words):
    """... by the header"""
    return _words(header_lib().gauss_check_words, words)


def ref_field(seed, S, n0, count):
    """z(seed, S, n0 .. n0 + count), n0 % 4 == 0"""
    out = np.empty(count, np.float64)
    ref_lib().impair_ref_field(seed, S, n0, count, out.ctypes.data)
    return out


def header_field(seed, S, n0, count):
    assert n0 % 4 == 0 and count % 4 == 0
    out = np.empty(count, np.float64)
    header_lib().gauss_check_field(seed, S, n0 // 4, count // 4, None, out.ctypes.data)
    return out


def ref_impair(x, lens, out_s16, out_stride, seed=0, first_stream=0, first_sample=0, gain=1.0, sigma=0.0, dc=0.0,
               nsamples=None, shape=None):
    """The restatement of the entry on host arrays.  x: float32 or int16 [nstreams, stride], or None with
    shape = (nstreams, anything); lens: uint32 [nstreams] or None (then `nsamples` for all, default the
    width); gain / sigma / dc: a number or an array [nstreams] -> out [nstreams, out_stride]"""
    if x is not None:
        x = np.ascontiguousarray(x)
        assert x.dtype in (np.float32, np.int16) and x.ndim == 2
        nstreams, stride = x.shape
        kind = S16K if x.dtype == np.int16 else F32K
    else:
        nstreams, stride = shape
        kind = F32K
    if lens is not None:
        lens = np.ascontiguousarray(lens, np.uint32)
        assert lens.shape == (nstreams,)
    keep, ptr, val = [], {}, {}
    for name, v in (("gain", gain), ("sigma", sigma), ("dc", dc)):
        if np.ndim(v):
            a = np.ascontiguousarray(v, F32)
            assert a.shape == (nstreams,)
            keep.append(a)
            ptr[name], val[name] = a.ctypes.data, 0.0
        else:
            ptr[name], val[name] = None, float(v)
    out = np.full((nstreams, out_stride), 99, np.int16 if out_s16 else F32)
    ref_lib().impair_ref_rows(None if x is None else x.ctypes.data, stride, None if lens is None else lens.ctypes.data,
                              stride if nsamples is None else nsamples, nstreams, kind, S16K if out_s16 else F32K,
                              out.ctypes.data, out_stride, seed, first_stream, first_sample,
                              ptr["gain"], ptr["sigma"], ptr["dc"], val["gain"], val["sigma"], val["dc"])
    return out


def corner_words():
    """The words at the transform's corners: 0, 1, 2, 0xFFFFFFFE, 0xFFFFFFFF; every octant
    boundary k 2^29 and its two neighbours; the two t = w + 1 on either side of each crossing of m = sqrt 2
    for e = 1, 16, 31 -- as a list of uint32"""
    ws = [0, 1, 2, 0xFFFFFFFE, 0xFFFFFFFF]
    for k in range(9):
        ws += [(k << 29) + d for d in (-1, 0, 1)]
    root2 = 0x16A09E667F3BCD            # sqrt 2 * 2^52, rounded down: m > root2 / 2^52 halves m
    for e in (1, 16, 31):
        t = (root2 << e) >> 52          # the last t = m 2^e with m <= the threshold; t + 1 is halved
        ws += [t - 2, t - 1, t, t + 1]  # w = t - 1: the two t on either side, and one more each way
    return [w % (1 << 32) for w in ws]
