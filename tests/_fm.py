"""What tests/test_fm_args.py, tests/test_fm_ref.py and tests/test_gpu_fm.py share: the FM stage's host
restatement (tools/fm_ref.c) and the device's own angle header compiled for the host
(tools/angle_check.c, which includes minimodem_amd/csrc/mifsk_angle.h), both as temporary shared
objects (_phase.ref_lib), and the pairs at the angle's corners."""
import ctypes as C

import numpy as np

import _phase
from _phase import F32, ROOT, same_bits  # noqa: F401 (for the tests)

F32K, S16K = 0, 1                       # MIFSK_FEED_F32 / MIFSK_FEED_S16
U64, VP = C.c_uint64, C.c_void_p
TAN_PI_8 = float.fromhex("0x1.a827999fcef32p-2")


def ref_lib():
    """tools/fm_ref.c as a shared object"""
    return _phase.ref_lib("fm_ref", (
        ("fm_ref_turn", C.c_double, (C.c_double, C.c_double)),
        ("fm_ref_turns", None, (VP, VP, U64, VP)),
        ("fm_ref_step", U64, (C.c_float, C.c_double, C.c_double)),
        ("fm_ref_demod_rows", None, (VP, U64, VP, C.c_uint32, C.c_int, C.c_uint32, VP, U64, VP, VP, C.c_float)),
        ("fm_ref_mod_rows", None, (VP, U64, VP, C.c_uint32, C.c_int, C.c_uint32, VP, U64, C.c_double, C.c_double,
                                   VP, VP, C.c_float))))


def header_lib():
    """minimodem_amd/csrc/mifsk_angle.h compiled for the host (tools/angle_check.c)"""
    return _phase.ref_lib("angle_check", (
        ("angle_check_turns", None, (VP, VP, U64, VP)),
        ("angle_check_sweep", C.c_double, (U64,))))


def _turns(fn, y, x):
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    assert y.shape == x.shape and y.ndim == 1
    out = np.empty(y.shape, np.float64)
    fn(y.ctypes.data, x.ctypes.data, y.size, out.ctypes.data)
    return out


def ref_turns(y, x):
    """turn(y[i], x[i]) by the restatement"""
    return _turns(ref_lib().fm_ref_turns, y, x)


def header_turns(y, x):
    """... by the header"""
    return _turns(header_lib().angle_check_turns, y, x)


def corner_pairs():
    """(y, x) float64 arrays at the angle's corners: both axes with +-0.0; |x| = |y| in all four quadrants;
    ratios one ulp either side of tan(pi/8) and of 1, in every quadrant and either way round; subnormals;
    1e308 (mn + mx overflows); +-Inf and NaN on either side."""
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    pairs = []
    for z in (0.0, -0.0):
        for v in (1.0, -1.0, 0.0, -0.0, 3.5, -2.0 ** -1040, 1e308, -1e308):
            pairs += [(z, v), (v, z)]
    for m in (1.0, 0.3, 7e-310, 1e308, 2.0 ** -1074):
        pairs += [(sy * m, sx * m) for sy in (1, -1) for sx in (1, -1)]
    for big in (1.0, 1.75, 3e-300, 1e300):
        for ratio in (TAN_PI_8, 1.0):
            for small in (down(down(big * ratio)), down(big * ratio), big * ratio, up(big * ratio), up(up(big * ratio))):
                for sy in (1, -1):
                    for sx in (1, -1):
                        pairs += [(sy * small, sx * big), (sy * big, sx * small)]
    sub = (2.0 ** -1074, 3 * 2.0 ** -1074, 2.0 ** -1030, 2.0 ** -1023, 2.2250738585072014e-308)
    for a in sub:
        for b in sub + (1.0, 1e-300):
            pairs += [(a, b), (-b, a), (a, -b), (-b, -a), (-a, -b)]
    for a in (1e308, 1.7e308, 0.5e308):
        for b in (1e308, 0.42e308, 1.0, 2.0 ** -1074):
            pairs += [(a, b), (b, -a), (-a, -b)]
    special = (np.inf, -np.inf, np.nan)
    for a in special:
        for b in special + (0.0, -0.0, 1.0, -1.0, 1e308, 2.0 ** -1074):
            pairs += [(a, b), (b, a)]
    y, x = (np.array([p[i] for p in pairs], np.float64) for i in range(2))
    return y, x


def _lens(lens, nstreams):
    if lens is None:
        return None
    lens = np.ascontiguousarray(lens, np.uint32)
    assert lens.shape == (nstreams,)
    return lens


def ref_demod(iq, lens, out_stride, gain=1.0, prev=None, nsamples=None):
    """The restatement of the discriminator on host arrays.  iq: float32 or int16 [nstreams, stride, 2]; lens:
    uint32 [nstreams] or None (then `nsamples` for all, default the width); prev: float32 [nstreams, 2] or None
    -> (out float32 [nstreams, out_stride], last float32 [nstreams, 2])"""
    iq = np.ascontiguousarray(iq)
    assert iq.dtype in (np.float32, np.int16) and iq.ndim == 3 and iq.shape[2] == 2
    nstreams, stride = iq.shape[:2]
    lens = _lens(lens, nstreams)
    if prev is not None:
        prev = np.ascontiguousarray(prev, F32)
        assert prev.shape == (nstreams, 2)
    out, last = np.full((nstreams, out_stride), 99, F32), np.full((nstreams, 2), 99, F32)
    ref_lib().fm_ref_demod_rows(iq.ctypes.data, stride, None if lens is None else lens.ctypes.data,
                                stride if nsamples is None else nsamples, nstreams,
                                S16K if iq.dtype == np.int16 else F32K, out.ctypes.data, out_stride,
                                None if prev is None else prev.ctypes.data, last.ctypes.data, gain)
    return out, last


def ref_modulate(x, lens, out_s16, out_stride, deviation, centre=0.0, amplitude=1.0, phase0=None, nsamples=None):
    """The restatement of the modulator on host arrays.  x: float32 [nstreams, stride]; phase0: uint64
    [nstreams] or None -> (out float32 or int16 [nstreams, out_stride, 2], phase_out uint64 [nstreams])"""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    nstreams, stride = x.shape
    lens = _lens(lens, nstreams)
    if phase0 is not None:
        phase0 = np.ascontiguousarray(phase0, np.uint64)
        assert phase0.shape == (nstreams,)
    out = np.full((nstreams, out_stride, 2), 99, np.int16 if out_s16 else F32)
    phase_out = np.full(nstreams, 99, np.uint64)
    ref_lib().fm_ref_mod_rows(x.ctypes.data, stride, None if lens is None else lens.ctypes.data,
                              stride if nsamples is None else nsamples, nstreams, S16K if out_s16 else F32K,
                              out.ctypes.data, out_stride, deviation, centre,
                              None if phase0 is None else phase0.ctypes.data, phase_out.ctypes.data, amplitude)
    return out, phase_out
