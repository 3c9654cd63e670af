"""What tests/test_channel_iq_args.py and tests/test_gpu_channel_iq.py share: the I/Q channelizer's host
restatement (channel_ref_iq of tools/channel_ref.c, compiled by _phase.ref_lib), the float64 evaluation
of its Q plane, and the end-to-end input: three FM channels in one complex capture, with the host chain
that makes every stage of it from the transmitted audio."""
import ctypes as C

import numpy as np

import _fm as Fm
import _impair as Im
import _phase
from _channel import COMPLEX, F32, KINDS, S16, numpy_channelize, same_f32, size_cases  # noqa: F401 (for the tests)


def ref_lib():
    """tools/channel_ref.c as a shared object, channel_ref_iq bound"""
    return _phase.ref_lib("channel_ref", (
        ("channel_ref_iq", C.c_uint64, (C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                        C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p)),))


def ref_channelize_iq(x, kind, P, taps, D, centres, r, n=None):
    """The restatement on one row (numpy float32 / int16; complex rows [n, 2]) -> float32 [K, M, 2]: I, Q."""
    x = np.ascontiguousarray(x)
    assert x.dtype == (np.int16 if kind & S16 else F32) and x.ndim == (2 if kind & COMPLEX else 1)
    n = x.shape[0] if n is None else min(int(n), x.shape[0])
    taps = np.ascontiguousarray(taps, F32)
    centres = np.ascontiguousarray(centres, np.int32)
    T, K = taps.size, centres.size
    M = (n - T) // D + 1 if n >= T else 0
    out = np.zeros((K, max(M, 1), 2), F32)
    g = np.empty((T, 2), np.float64)
    got = ref_lib().channel_ref_iq(x.ctypes.data, n, kind, P, T, taps.ctypes.data, D, K, centres.ctypes.data, int(r),
                                   out.ctypes.data, out.shape[1], g.ctypes.data)
    assert got == M
    return out[:, :M]


def numpy_channelize_q(x, kind, P, taps, D, centres, r):
    """The Q plane in numpy float64 -> (float64 [K, M], the bound's sum per output [M]): .imag of the product
    numpy_channelize takes .real of.  Im(z) = Re(-j z), and the product is linear in the row, so it is
    numpy_channelize itself on the row times -j, which is exact: (xr, xi) -> (xi, -xr) of the widened
    scalars, as a complex float32 row."""
    v = x.astype(F32) / F32(32768.0) if kind & S16 else x.astype(F32)
    xr, xi = (v[:, 0], v[:, 1]) if kind & COMPLEX else (v, np.zeros_like(v))
    return numpy_channelize(np.stack([xi, -xr], axis=1), COMPLEX, P, taps, D, centres, r)


def centres_of(rng, K, P):
    """K centres: both ends, the middle and zero first, then random ones"""
    fixed = [0, -1, P // 2, -(P - 1), 1, -(P // 2)]
    more = rng.integers(-(P - 1), P, max(0, K - len(fixed)))
    return np.array((fixed + [int(v) for v in more])[:K], np.int32)


def random_rows(rng, kind, nrows, n):
    shape = (nrows, n, 2) if kind & COMPLEX else (nrows, n)
    if kind & S16:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return rng.standard_normal(shape).astype(F32)


# ---------------------------------------------------------------------------
# end to end: three FM channels of one capture
# ---------------------------------------------------------------------------
FS, P_FM, D_FM = 192000, 1920, 4                    # 100 Hz steps; 48 kHz out
OFFSETS = (-30000.0, 3000.0, 41000.0)               # the FM channels' centres in the capture, Hz
CENTRES = (-300, 30, 410)                           # ... in steps
LEAD = (12, 301, 150)                               # leading silence of each message, samples at FS
DEVIATION_HZ, CARRIER, SEED = 3000.0, 0.3, 7
NTAPS, CUTOFF = 129, 6000.0


def fm_messages():
    """three Bell-202 messages of 16 printable bytes -> uint8 [3, 16]"""
    return np.random.default_rng(355).integers(0x20, 0x7F, size=(3, 16), dtype=np.uint8)


def fm_sigma(M, cnr_db):
    """the noise sigma over the capture as 2n reals: three carriers of amplitude 0.3 at cnr_db, None: none"""
    return 0.0 if cnr_db is None else M.snr_sigma(CARRIER * np.sqrt(2.0), cnr_db)


def fm_host_chain(M, audio, lens, sigma):
    """The host's chain from the transmitted audio (float32 [3, n] at FS, uint32 lengths): fm_ref.c per channel
    at its centre, the float32 sum in channel order, impair_ref.c over the row as 2n reals, channel_ref_iq,
    fm_ref.c -> dict(capture [n, 2], noisy [n, 2], iq [3, M, 2], audio [3, M rounded up to 4], nout)"""
    n = audio.shape[1]
    dev = M.fm_step(DEVIATION_HZ, FS)
    rows = [Fm.ref_modulate(audio[k:k + 1], lens[k:k + 1], False, n, dev, centre=M.fm_step(off, FS),
                            amplitude=CARRIER)[0][0] for k, off in enumerate(OFFSETS)]
    capture = (rows[0] + rows[1]) + rows[2]
    assert capture.dtype == F32 and capture.shape == (n, 2)
    noisy = Im.ref_impair(capture.reshape(1, 2 * n), None, False, 2 * n, seed=SEED, sigma=sigma).reshape(n, 2)
    taps = M.channel_taps(NTAPS, CUTOFF, float(FS), 1.0)
    iq = ref_channelize_iq(noisy, COMPLEX, P_FM, taps, D_FM, CENTRES, 0)
    nout = iq.shape[1]
    stride = (nout + 3) // 4 * 4
    padded = np.zeros((3, stride, 2), F32)
    padded[:, :nout] = iq
    out, _last = Fm.ref_demod(padded, np.full(3, nout, np.uint32), stride, gain=M.fm_gain(FS / D_FM, DEVIATION_HZ))
    return {"capture": capture, "noisy": noisy, "iq": iq, "audio": out, "nout": nout, "taps": taps}
