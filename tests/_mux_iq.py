"""What tests/test_mux_iq_args.py and tests/test_gpu_mux_iq.py share: the I/Q multiplexer's host restatement
(mux_ref_iq of tools/mux_ref.c, compiled by _phase.ref_lib), a float64 / complex128 evaluation of its
definition, and the end-to-end input: three FM channels made at the narrow rate and put on one complex
capture, with the host chain that makes every stage of it from the transmitted audio."""
import ctypes as C

import numpy as np

import _channel_iq as Iq
import _fm as Fm
import _impair as Im
import _mux as Mx
import _phase
from _mux import COMPLEX, F32, KINDS, S16, full_outputs, numpy_s16, same_bits, size_cases, vec_of  # noqa: F401 (for the tests)

_MUX_ARGS = (C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)


def ref_lib():
    """tools/mux_ref.c as a shared object, mux_ref_iq bound"""
    return _phase.ref_lib("mux_ref", (("mux_ref_iq", C.c_uint64, _MUX_ARGS),))


def ref_multiplex_iq(x, lens, kind, P, taps, L, centres, r, gains=None, out_stride=None, nout_cap=None):
    """The restatement on one stream: x float32 [K, stride, 2], lens [K] of (I, Q) elements (None: the
    stride) -> (out [out_stride] or [out_stride, 2], float32 or int16, zero behind the count; the count)."""
    x = np.ascontiguousarray(x, F32)
    assert x.ndim == 3 and x.shape[2] == 2
    K, stride = x.shape[:2]
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
    cnt = ref_lib().mux_ref_iq(x.ctypes.data, stride, lens.ctypes.data, kind, P, taps.size, taps.ctypes.data, L, K,
                               centres.ctypes.data, int(r), None if gains is None else gains.ctypes.data,
                               out.ctypes.data, out_stride, nout_cap, g.ctypes.data)
    return out, int(cnt)


def numpy_multiplex_iq(x, lens, P, taps, L, centres, r, gains=None):
    """_mux.numpy_multiplex with the zero-stuffed row complex: x float32 [K, stride, 2] -> (complex128 [M]:
    o + j oi, float64 [M]: S[n] = sum_k |gain_k| sum_j |h[t]| (|I_k[i]| + |Q_k[i]|), the bound's magnitude)."""
    x = np.asarray(x, F32).astype(np.float64)
    K, stride = x.shape[:2]
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
        up = np.zeros((lens[k] - 1) * L + 1, np.complex128)
        up[::L] = x[k, :lens[k], 0] + 1j * x[k, :lens[k], 1]
        gain = 1.0 if gains is None else float(F32(gains[k]))
        y = np.convolve(up, g) * gain
        p = (((int(centres[k]) % P - rr) % P) * (n[:y.size] % P)) % P
        out[:y.size] += y * np.exp(2j * np.pi * p / P)
        mag[:y.size] += np.convolve(np.abs(up.real) + np.abs(up.imag), np.abs(h)) * abs(gain)
    return out, mag


def iq_rows(rng, nrows, n, scale=1.0):
    return (rng.standard_normal((nrows, n, 2)) * scale).astype(F32)


def even(n):
    return (int(n) + 1) // 2 * 2


# ---------------------------------------------------------------------------
# end to end: three FM channels made at 48 kHz, put on one 192 kHz capture and taken off it again
# ---------------------------------------------------------------------------
# The receive side is _channel_iq's (129 taps, 6 kHz, D = 4, out_centre 0, the centres and the noise).  The
# transmit filter was chosen from the spectrum: Carson's bandwidth of 3 kHz deviation around 2.2 kHz audio is
# +-5.2 kHz, the images of the zero-stuffed 48 kHz rows begin 48 - 5.2 = 42.8 kHz from each centre, and the
# Hamming transition of 129 taps at 192 kHz (about 3.3 * 192000 / 129 = 4.9 kHz wide) around 12 kHz ends near
# 14.5 kHz.  A complex row is one-sided: the taps sum to L.
FS_IN, L_FM, TX_NTAPS, TX_CUTOFF = 48000, 4, 129, 12000.0
TX_LEAD = (3, 75, 37)                               # leading silence of each message, samples at FS_IN


def fm_tx_audio(M):
    """the three messages as audio at 48 kHz from the host transmitter -> (words, float32 [3, n], uint32 [3])"""
    words = Iq.fm_messages()
    cfg = M.rx_config("1200", sample_rate=FS_IN)
    sigs = [M.synthesize(cfg, words[k], amplitude=1.0, leading_silence=TX_LEAD[k]) for k in range(3)]
    n = (max(s.size for s in sigs) + 3) // 4 * 4
    audio = np.zeros((3, n), F32)
    for k, s in enumerate(sigs):
        audio[k, :s.size] = s
    return words, audio, np.array([s.size for s in sigs], np.uint32)


def fm_tx_taps(M):
    return M.channel_taps(TX_NTAPS, TX_CUTOFF, float(Iq.FS), float(L_FM))


def fm_host_chain(M, audio, lens, sigma):
    """The host's chain from the transmitted audio (float32 [3, n] at FS_IN, uint32 lengths), every array of the
    shape the device's stage gives it: fm_ref.c at centre 0 -> mux_ref_iq -> impair_ref.c over the whole row as
    2 stride reals -> channel_ref_iq on the row's count -> fm_ref.c
    -> dict(iq [3, n, 2], capture [S, 2], count, noisy [S, 2], ch [3, C, 2], audio [3, A], nout, taps, rx_taps)"""
    n = audio.shape[1]
    iq = Fm.ref_modulate(audio, lens, False, n, M.fm_step(Iq.DEVIATION_HZ, FS_IN), centre=0.0, amplitude=Iq.CARRIER)[0]
    taps = fm_tx_taps(M)
    stride = even(full_outputs(n, L_FM, TX_NTAPS))
    capture, count = ref_multiplex_iq(iq, lens, COMPLEX, Iq.P_FM, taps, L_FM, Iq.CENTRES, 0, out_stride=stride)
    assert count == full_outputs(int(lens.max()), L_FM, TX_NTAPS)
    noisy = Im.ref_impair(capture.reshape(1, 2 * stride), None, False, 2 * stride, seed=Iq.SEED,
                          sigma=sigma).reshape(stride, 2)
    rx_taps = M.channel_taps(Iq.NTAPS, Iq.CUTOFF, float(Iq.FS), 1.0)
    rows = Iq.ref_channelize_iq(noisy, COMPLEX, Iq.P_FM, rx_taps, Iq.D_FM, Iq.CENTRES, 0, n=count)
    nout = rows.shape[1]
    ch_stride = max(2, even((stride - Iq.NTAPS) // Iq.D_FM + 1))
    ch = np.zeros((3, ch_stride, 2), F32)
    ch[:, :nout] = rows
    out, _last = Fm.ref_demod(ch, np.full(3, nout, np.uint32), (ch_stride + 3) // 4 * 4,
                              gain=M.fm_gain(Iq.FS / Iq.D_FM, Iq.DEVIATION_HZ))
    return {"iq": iq, "capture": capture, "count": count, "noisy": noisy, "ch": ch, "audio": out, "nout": nout,
            "taps": taps, "rx_taps": rx_taps}
