"""What tests/test_mux_args.py and tests/test_gpu_mux.py share: the multiplexer's host restatement
(tools/mux_ref.c, compiled into a temporary shared object), a vectorised float64 evaluation of the
definition with its rounding bound, the sampled sizes of the GPU test, and the closed-loop input."""
import ctypes as C
import functools

import numpy as np

import _phase
from _phase import COMPLEX, F32, KINDS, ROOT, S16, same_bits, vec_of  # noqa: F401 (for the tests)


def ref_lib():
    """tools/mux_ref.c as a shared object (_phase.ref_lib)"""
    return _phase.ref_lib("mux_ref", (
        ("mux_ref_table", None, (C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p)),
        ("mux_ref", C.c_uint64, (C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64,
                                 C.c_uint64, C.c_void_p))))


def full_outputs(n, L, T):
    return (n - 1) * L + T if n > 0 else 0


def ref_table(P, taps, r):
    taps = np.ascontiguousarray(taps, F32)
    g = np.empty((taps.size, 2), np.float64)
    ref_lib().mux_ref_table(P, taps.size, taps.ctypes.data, int(r), g.ctypes.data)
    return g


def ref_multiplex(x, lens, kind, P, taps, L, centres, r, gains=None, out_stride=None, nout_cap=None):
    """The restatement on one stream: x float32 [K, stride], lens [K] (None: the stride) ->
    (out [out_stride] or [out_stride, 2], float32 or int16, zero behind the count; the count)."""
    x = np.ascontiguousarray(x, F32)
    K, stride = x.shape
    lens = np.full(K, stride, np.uint32) if lens is None else np.ascontiguousarray(lens, np.uint32)
    taps = np.ascontiguousarray(taps, F32)
    centres = np.ascontiguousarray(centres, np.int32)
    assert lens.shape == (K,) and centres.shape == (K,)
    gains = None if gains is None else np.ascontiguousarray(gains, F32)
    if out_stride is None:
        v = vec_of(kind)
        out_stride = max(v, (full_outputs(int(min(lens.max(), stride)), L, taps.size) + v - 1) // v * v)
    nout_cap = out_stride if nout_cap is None else nout_cap
    shape = (out_stride, 2) if kind & COMPLEX else (out_stride,)
    out = np.full(shape, 99, np.int16 if kind & S16 else F32)
    g = np.empty((taps.size, 2), np.float64)
    cnt = ref_lib().mux_ref(x.ctypes.data, stride, lens.ctypes.data, kind, P, taps.size, taps.ctypes.data, L, K,
                            centres.ctypes.data, int(r), None if gains is None else gains.ctypes.data,
                            out.ctypes.data, out_stride, nout_cap, g.ctypes.data)
    return out, int(cnt)


def numpy_s16(v):
    """the stated PCM16 conversion of float32 values, in numpy"""
    t = np.asarray(v, F32) * F32(32767.0)
    t = np.where(t > F32(32767.0), F32(32767.0), t)
    t = np.where(t < F32(-32768.0), F32(-32768.0), t)
    nan = np.isnan(t)
    return np.where(nan, 0, np.rint(np.where(nan, F32(0.0), t))).astype(np.int16)


def numpy_multiplex(x, lens, P, taps, L, centres, r, gains=None):
    """The definition evaluated in numpy float64 / complex128, vectorised -> (complex128 [M]: o + j oi,
    float64 [M]: S[n] = sum_k |gain_k| sum_j |h[t]| |x_k[i]|, the bound's magnitude)."""
    x = np.asarray(x, F32).astype(np.float64)
    K, stride = x.shape
    lens = [stride] * K if lens is None else [min(int(n), stride) for n in lens]
    h = np.asarray(taps, F32).astype(np.float64)
    T = h.size
    M = full_outputs(max(lens), L, T)
    t = np.arange(T, dtype=np.int64)
    rr = int(r) % P
    g = h * np.exp(2j * np.pi * ((rr * t) % P) / P)
    n = np.arange(M, dtype=np.int64)
    out, mag = np.zeros(M, np.complex128), np.zeros(M, np.float64)
    for k in range(K):
        if lens[k] == 0:
            continue
        up = np.zeros((lens[k] - 1) * L + 1, np.float64)
        up[::L] = x[k, :lens[k]]
        gain = 1.0 if gains is None else float(F32(gains[k]))
        y = np.convolve(up, g) * gain
        p = (((int(centres[k]) % P - rr) % P) * (n[:y.size] % P)) % P
        out[:y.size] += y * np.exp(2j * np.pi * p / P)
        mag[:y.size] += np.convolve(np.abs(up), np.abs(h)) * abs(gain)
    return out, mag


# ---------------------------------------------------------------------------
# the sampled product of the GPU test's sizes
# ---------------------------------------------------------------------------
LS = (1, 2, 3, 40, 63, 64, 65, 300)         # 300: one group of 8 L outputs spans several workgroups
KS = (1, 2, 3, 64, 65)
PS = (1, 7, 4800)


def t_rules(L):
    """1, below L, L, one above a multiple of L, about 10 L"""
    return (1, max(1, L - 1), L, 2 * L + 1, min(4096, 10 * L + 3))


def size_cases():
    """(kind name, L, T, K, P), two rounds over LS: every L twice, every T rule, every K and every P with
    at least one kind each, every kind four times"""
    names = list(KINDS)
    cases = []
    for rnd in range(2):
        for i, L in enumerate(LS):
            j = i + 3 * rnd
            cases.append((names[(i + rnd) % 4], L, t_rules(L)[(j + rnd) % 5], KS[(j + 2 * rnd) % 5], PS[j % 3]))
    return cases


# ---------------------------------------------------------------------------
# the closed loop: synthesize -> multiplex -> channelize -> demodulate
# ---------------------------------------------------------------------------
# Chosen so that the restatement alone decodes (tests/test_mux_args.py proves it): the Bell-202 tones
# (1200 / 2200 Hz, centre 1700 Hz) of a 48 kHz row reappear, zero-stuffed by L = 4, around +-1700 Hz
# and around every multiple of 48 kHz of the 192 kHz row.  G keeps 1700 +- MUX_CUTOFF Hz; its
# Hamming transition, about 3.3 * 192000 / MUX_TAPS = 1650 Hz wide, ends before the image at
# -1200 .. -2200 Hz (2900 Hz and more from the centre) begins.
MUX_TAPS, MUX_CUTOFF = 385, 1200.0
MUX_L, MUX_P, MUX_FS_IN = 4, 1920, 48000
MUX_OFFSETS = (-30000.0, 3000.0, 41000.0)           # tests/_channel.py:three_bell202_iq's
MUX_GAINS = (1.0, 0.25, 1.0)                        # the middle channel 12 dB down


@functools.lru_cache(maxsize=None)
def three_bell202_rows():
    """Three Bell-202 rows of 24 random words from M.synthesize at 48 kHz, amplitude 0.3, behind 16, 75
    and 37 samples of silence, for centres at -30, +3 and +41 kHz of a 192 kHz capture (P = 1920: 100 Hz
    steps, r at 1700 Hz).  -> dict(x [3, stride], lens, P, L, taps, centres, r, gains, payloads, mode,
    rx_taps {complex: ..., real: ...}, rx_D)"""
    import minimodem_amd as M
    rng = np.random.default_rng(2020)
    fs_out = MUX_FS_IN * MUX_L
    payloads = [bytes(rng.integers(0x20, 0x7F, 24, dtype=np.uint8)) for _ in MUX_OFFSETS]
    cfg = M.rx_config("1200", sample_rate=MUX_FS_IN)
    sigs = [M.synthesize(cfg, words, amplitude=0.3, leading_silence=lead)
            for words, lead in zip(payloads, (16, 75, 37))]
    stride = (max(s.size for s in sigs) + 3) // 4 * 4
    x = np.zeros((3, stride), F32)
    for k, s in enumerate(sigs):
        x[k, :s.size] = s
    return {"x": x, "lens": np.array([s.size for s in sigs], np.int32), "P": MUX_P, "L": MUX_L,
            "taps": M.channel_taps(MUX_TAPS, MUX_CUTOFF, float(fs_out), 2.0 * MUX_L),
            "centres": np.array([int(round(off * MUX_P / fs_out)) for off in MUX_OFFSETS], np.int32),
            "r": int(round(1700.0 * MUX_P / fs_out)), "gains": np.array(MUX_GAINS, F32),
            "payloads": payloads, "mode": "1200",
            # the receive side: three_bell202_iq's channelizer, 129 taps, 2.4 kHz, D = 4; a real capture
            # wants taps that sum to 2
            "rx_taps": {True: M.channel_taps(129, 2400.0, float(fs_out), 1.0),
                        False: M.channel_taps(129, 2400.0, float(fs_out), 2.0)},
            "rx_D": MUX_L}
