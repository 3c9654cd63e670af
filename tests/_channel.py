"""What tests/test_channel_args.py and tests/test_gpu_channel.py share: the channelizer's host
restatement (tools/channel_ref.c, compiled into a temporary shared object), a vectorised float64
evaluation of the definition, and the two end-to-end inputs with their condition."""
import ctypes as C
import functools

import numpy as np

import _phase
from _phase import COMPLEX, F32, KINDS, ROOT, S16, same_bits  # noqa: F401 (for the tests)


def ref_lib():
    """tools/channel_ref.c as a shared object (_phase.ref_lib)"""
    return _phase.ref_lib("channel_ref", (
        ("channel_ref_table", None, (C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p)),
        ("channel_ref", C.c_uint64, (C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p))))


# the sampled product of the GPU test's sizes
TS = (1, 2, 63, 64, 65, 385)
KS = (1, 2, 3, 63, 64, 65, 130)
PS = (7, 4799, 4800, 65536)


def d_rules(T):
    return (1, 3, 4, 7, T, T + 5)


def size_cases():
    """(kind name, T, D, K, P), 7 per kind: every T, every D rule, every K and every P with every kind"""
    cases = []
    for ki, name in enumerate(KINDS):
        for i, K in enumerate(KS):
            T = TS[(i + ki) % 6]
            cases.append((name, T, d_rules(T)[(i + 2 * ki + 1) % 6], K, PS[(i + ki) % 4]))
    return cases


def ref_table(P, taps, q):
    taps = np.ascontiguousarray(taps, F32)
    g = np.empty((taps.size, 2), np.float64)
    ref_lib().channel_ref_table(P, taps.size, taps.ctypes.data, int(q), g.ctypes.data)
    return g


def ref_channelize(x, kind, P, taps, D, centres, r, n=None):
    """The restatement on one row (numpy float32 / int16; complex rows [n, 2]) -> float32 [K, M]."""
    x = np.ascontiguousarray(x)
    assert x.dtype == (np.int16 if kind & S16 else F32) and x.ndim == (2 if kind & COMPLEX else 1)
    n = x.shape[0] if n is None else min(int(n), x.shape[0])
    taps = np.ascontiguousarray(taps, F32)
    centres = np.ascontiguousarray(centres, np.int32)
    T, K = taps.size, centres.size
    M = (n - T) // D + 1 if n >= T else 0
    out = np.zeros((K, max(M, 1)), F32)
    g = np.empty((T, 2), np.float64)
    got = ref_lib().channel_ref(x.ctypes.data, n, kind, P, T, taps.ctypes.data, D, K, centres.ctypes.data, int(r),
                                out.ctypes.data, out.shape[1], g.ctypes.data)
    assert got == M
    return out[:, :M]


def widen(x, kind):
    """a row's scalars as the definition widens them -> float64 (complex128 for complex rows)"""
    v = (x.astype(F32) / F32(32768.0)).astype(np.float64) if kind & S16 else x.astype(np.float64)
    return v[:, 0] + 1j * v[:, 1] if kind & COMPLEX else v


def numpy_channelize(x, kind, P, taps, D, centres, r):
    """The definition evaluated in numpy float64, vectorised -> (float64 [K, M], the bound's
    sum_t |h[t]| (|xr| + |xi|) per output [M])."""
    v = widen(x, kind)
    taps = np.asarray(taps, F32).astype(np.float64)
    T, n = taps.size, v.shape[0]
    M = (n - T) // D + 1 if n >= T else 0
    idx = (np.arange(M, dtype=np.int64) * D)[:, None] + np.arange(T, dtype=np.int64)[None, :]
    win = v[idx] if M else np.zeros((0, T), v.dtype)
    mag = (np.abs(win.real) + np.abs(win.imag)) @ np.abs(taps)
    out = np.empty((len(centres), M), np.float64)
    t = np.arange(T, dtype=np.int64)
    md = (np.arange(M, dtype=np.int64) * D) % P
    for k, q in enumerate(centres):
        q = int(q) % P
        g = taps * np.exp(-2j * np.pi * ((q * t) % P) / P)
        y = win @ g
        p = (((int(r) - q) % P) * md) % P
        out[k] = (y * np.exp(2j * np.pi * p / P)).real
    return out, mag


def same_f32(a, b):
    """equal float bit patterns, any NaN equal to any NaN"""
    return same_bits(np.asarray(a, F32), np.asarray(b, F32))


# ---------------------------------------------------------------------------
# the two end-to-end inputs
# ---------------------------------------------------------------------------
def payload_condition(decoded, payload):
    """the payload as one contiguous run, at most 2 bytes beside it"""
    at = decoded.find(payload)
    return at >= 0 and len(decoded) - len(payload) <= 2


@functools.lru_cache(maxsize=None)
def three_bell103():
    """Three 300-baud signals keyed 0, +1200 and -600 Hz off the Bell-103 tones, amplitude 0.3, summed
    into one real row at 48 kHz.  P = 4800 (10 Hz steps), 385 taps, cutoff 400 Hz, sum 2, D = 1.
    -> dict(x, kind, P, taps, D, centres, r, payloads, mode)"""
    import minimodem_amd as M
    rng = np.random.default_rng(103)
    base = M.rx_config("300")
    centre = (float(base.mark_f) + float(base.space_f)) / 2.0            # 1170 Hz
    offsets = (0.0, 1200.0, -600.0)
    payloads = [bytes(rng.integers(0x20, 0x7F, 18, dtype=np.uint8)) for _ in offsets]
    sigs = []
    for off, words in zip(offsets, payloads):
        cfg = M.rx_config("300", mark_f=float(base.mark_f) + off, space_f=float(base.space_f) + off)
        sigs.append(M.synthesize(cfg, words, amplitude=0.3))
    n = (max(s.size for s in sigs) + 400 + 7) // 8 * 8
    x = np.zeros(n, F32)
    for s in sigs:
        x[200:200 + s.size] += s
    P = 4800
    assert int(base.sample_rate) == 48000 and centre * P % 48000 == 0
    return {"x": x, "kind": 0, "P": P, "taps": M.channel_taps(385, 400.0, 48000.0, 2.0), "D": 1,
            "centres": np.array([int(round((centre + off) * P / 48000)) for off in offsets], np.int32),
            "r": int(round(centre * P / 48000)), "payloads": payloads, "mode": "300"}


@functools.lru_cache(maxsize=None)
def three_bell202_iq():
    """Three Bell-202 signals of 24 random words at -30, +3 and +41 kHz of a complex capture at 192 kHz,
    each starting at another sample, plus Gaussian noise of sigma 0.05.  P = 1920 (100 Hz steps), 129
    taps, cutoff 2.4 kHz, D = 4 (48 kHz out), r at 1700 Hz."""
    import minimodem_amd as M
    rng = np.random.default_rng(202)
    fs, P, D = 192000, 1920, 4
    offsets = (-30000.0, 3000.0, 41000.0)
    starts = (64, 301, 150)
    payloads = [bytes(rng.integers(0x20, 0x7F, 24, dtype=np.uint8)) for _ in offsets]
    cfg = M.rx_config("1200", sample_rate=fs)
    sigs = [M.synthesize(cfg, words, amplitude=0.3) for words in payloads]
    n = (max(a + s.size for a, s in zip(starts, sigs)) + 200 + 3) // 4 * 4
    z = np.zeros(n, np.complex128)
    t = np.arange(n, dtype=np.float64)
    for off, a, s in zip(offsets, starts, sigs):
        real = np.zeros(n, np.float64)
        real[a:a + s.size] = s
        spec = np.fft.fft(real)                                         # the analytic signal
        spec[n // 2 + 1:] = 0.0
        spec[1:(n + 1) // 2] *= 2.0
        z += np.fft.ifft(spec) * np.exp(2j * np.pi * (off - 1700.0) * t / fs)
    z += 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.stack([z.real, z.imag], axis=1).astype(F32)
    return {"x": x, "kind": COMPLEX, "P": P, "taps": M.channel_taps(129, 2400.0, float(fs), 1.0), "D": D,
            "centres": np.array([int(round(off * P / fs)) for off in offsets], np.int32),
            "r": int(round(1700.0 * P / fs)), "payloads": payloads, "mode": "1200"}
