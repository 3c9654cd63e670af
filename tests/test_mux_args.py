"""The multiplexer (include/mifsk.h, minimodem_amd/csrc/mifsk_mux.hip) without a device: what
mifsk_mux_plan_create and mifsk_multiplex_batch refuse before any HIP call (the context is a block of
zeroed host memory, the device pointers are numbers), the host table, the host restatement
tools/mux_ref.c against a float64 evaluation of the definition, and the condition the GPU test's
end-to-end cases rely on: the restatement's captures, channelized by the channelizer's restatement,
decode through the oracle."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _mux as Mx
import _oracle as O
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32


def test_the_python_names_are_public():
    assert _lib.MUX_COMPLEX == M.MUX_COMPLEX
    for name in ("MuxPlan", "multiplex", "mux_table", "MuxParams", "MuxIO", "MUX_COMPLEX"):
        assert name in M.__all__ and hasattr(M, name), name
    assert M.MuxParams is _lib.MuxParams and M.MuxIO is _lib.MuxIO


def _params(keep, **kw):
    """valid parameters (4 taps, 3 channels, P = 4800, L = 4) with the fields of kw replaced"""
    taps = np.array(kw.pop("taps_array", [0.25, 0.5, 0.5, 0.25]), F32)
    centres = np.array(kw.pop("centres_array", [117, -60, 2400]), np.int32)
    keep += [taps, centres]
    p = _lib.MuxParams()
    p.kind, p.flags, p.phase_steps = _lib.FEED_F32, 0, 4800
    p.ntaps, p.taps, p.interp = taps.size, taps.ctypes.data, 4
    p.nchannels, p.centres, p.in_centre, p.gains = centres.size, centres.ctypes.data, 170, None
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_plan_create_refuses_before_any_hip_call(lib, fake_ctx):
    ctx, _keep = fake_ctx
    keep = []

    def rc(ctx=ctx, params=True, out=True, **kw):
        h = C.c_void_p()
        return lib.mifsk_mux_plan_create(ctx, C.byref(_params(keep, **kw)) if params else None,
                                         C.byref(h) if out else None)

    assert rc(ctx=None) == EINVAL and rc(params=False) == EINVAL and rc(out=False) == EINVAL
    assert rc(taps=None) == EINVAL and rc(centres=None) == EINVAL
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    assert rc(flags=2) == EINVAL and rc(flags=0x80000001) == EINVAL
    assert rc(phase_steps=0) == EINVAL and rc(phase_steps=(1 << 20) + 1) == EINVAL
    assert rc(ntaps=0) == EINVAL and rc(ntaps=4097) == EINVAL
    assert rc(interp=0) == EINVAL and rc(interp=65536) == EINVAL
    assert rc(nchannels=0) == EINVAL and rc(nchannels=4097) == EINVAL
    for bad in (4800, -4800, 4801, -(1 << 31), (1 << 31) - 1):              # |centre| >= P
        assert rc(centres_array=[117, bad, 0]) == EINVAL, bad
        assert rc(in_centre=bad) == EINVAL, bad
    assert rc(phase_steps=7, centres_array=[0, 7], in_centre=0) == EINVAL
    assert rc(phase_steps=1, centres_array=[0], in_centre=1) == EINVAL
    # the earlier checks win over the later ones
    assert rc(ctx=None, ntaps=0) == EINVAL and rc(kind=5, centres_array=[4800]) == EINVAL
    # the same verdicts from the host-only table entry
    g = np.zeros((4, 2))
    for kw in (dict(ntaps=0), dict(kind=2), dict(flags=4), dict(phase_steps=0), dict(centres_array=[4800]),
               dict(interp=0), dict(nchannels=0), dict(in_centre=-4800), dict(taps=None)):
        assert lib.mifsk_mux_table(C.byref(_params(keep, **kw)), g.ctypes.data) == EINVAL, kw
    assert lib.mifsk_mux_table(C.byref(_params(keep)), None) == EINVAL
    assert lib.mifsk_mux_table(None, g.ctypes.data) == EINVAL
    assert lib.mifsk_mux_table(C.byref(_params(keep)), g.ctypes.data) == 0
    # gains are data: any pointer, any values
    gains = np.array([np.nan, np.inf, -0.0], F32)
    assert lib.mifsk_mux_table(C.byref(_params(keep, gains=gains.ctypes.data)), g.ctypes.data) == 0


def _io(**kw):
    base = 1 << 20                                  # 16-byte aligned; never dereferenced
    io = _lib.MuxIO()
    io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = base, 4000, None, 4000, 2
    io.d_out, io.out_stride, io.nout_cap, io.d_nout = base + (1 << 24), 16000, 16000, base + (1 << 26)
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_multiplex_refuses_without_a_plan(lib):
    """mifsk_multiplex_batch on a NULL plan comes back with -EINVAL, with or without an io.  The
    output's kind is the plan's, so what the entry refuses of an io can only be asked with a plan, and
    a plan needs a device: those refusals, in their order and before any launch, are
    tests/test_gpu_mux.py::test_what_multiplex_refuses_of_the_io."""
    assert lib.mifsk_multiplex_batch(None, None, None) == EINVAL
    assert lib.mifsk_multiplex_batch(None, C.byref(_io()), None) == EINVAL


def test_the_gpu_tests_sampled_sizes_cover_every_value():
    cases = Mx.size_cases()
    assert {c[1] for c in cases} >= {1, 2, 3, 40, 63, 64, 65}
    assert {c[3] for c in cases} == {1, 2, 3, 64, 65} and {c[4] for c in cases} == {1, 7, 4800}
    assert {c[0] for c in cases} == set(Mx.KINDS)
    rules = set()
    for _n, L, T, _K, _P in cases:
        rules |= {i for i, t in enumerate(Mx.t_rules(L)) if t == T}
    assert rules == set(range(5)), rules
    assert any(T < L for _n, L, T, _K, _P in cases) and any(T > 9 * L and L > 1 for _n, L, T, _K, _P in cases)
    assert any(T % L == 1 and T > L > 1 for _n, L, T, _K, _P in cases)


@pytest.mark.parametrize("P", [1, 7, 4799, 4800, 1 << 20])
def test_mux_table_equals_the_restatement_bit_for_bit(P):
    rng = np.random.default_rng(P)
    taps = np.concatenate([M.channel_taps(385, 1200.0, 192000.0, 8.0), rng.standard_normal(40).astype(F32)])
    for r in (0, 1, -1, P // 2, -(P - 1), P - 1):
        if abs(r) >= P:
            continue
        got = M.mux_table(taps, r, P)
        want = Mx.ref_table(P, taps, r)
        assert got.shape == (taps.size, 2)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (P, r)
    # r = 0 is the taps themselves; r and r - P are the same table
    g0 = M.mux_table(taps, 0, P)
    assert np.array_equal(g0[:, 0], taps.astype(np.float64)) and not np.any(g0[:, 1])
    if P > 1:
        assert np.array_equal(M.mux_table(taps, 1, P), M.mux_table(taps, -(P - 1), P))
        # the conjugate of the channelizer's table at the same centre
        ch = M.channel_table(taps, [1], 0, P)
        g1 = M.mux_table(taps, 1, P)
        assert np.array_equal(g1[:, 0], ch[:, 0]) and np.array_equal(g1[:, 1], -ch[:, 1])


@pytest.mark.parametrize("P", [1, 7, 4800, 1 << 20])
def test_mux_table_is_the_channelizers_table_with_the_second_column_negated(P):
    """The two tables are one routine (mifsk_phase.h, phase_rotated_taps): entry for entry the same bits
    but for the sign bit of the second column (IEEE negation: of zeros and NaNs too)."""
    rng = np.random.default_rng(P + 1)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf], F32)
    assert np.all(np.abs(special[2:4]) < np.finfo(F32).tiny) and np.all(special[2:4] != 0)     # subnormal
    taps = np.concatenate([special, rng.standard_normal(19).astype(F32), special[::-1]])
    sign = np.uint64(1) << np.uint64(63)
    tried = 0
    for q in (0, 1, -1, P - 1, -(P - 1)):
        if abs(q) >= P:
            continue
        mx = M.mux_table(taps, q, P).view(np.uint64)
        ch = M.channel_table(taps, [q], 0, P).view(np.uint64)
        assert mx.shape == ch.shape == (taps.size, 2)
        assert np.array_equal(mx[:, 0], ch[:, 0]) and np.array_equal(mx[:, 1], ch[:, 1] ^ sign), (P, q)
        tried += 1
    assert tried == (3 if P == 1 else 5)                # P = 1: 0, P - 1 and -(P - 1) are all 0


@pytest.mark.parametrize("gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name", list(Mx.KINDS))
def test_the_restatement_against_float64(name, gains):
    """With J = ceil(T / L) tap steps, K channels and S[n] = sum_k |gain_k| sum_j |h[t]| |x_k[i]|, each of
    o and oi of the restatement lies within
        E = (2 J + 2 K + 40) 2^-52 S[n]
    of the float64 value.  Per channel A_k bounds |re| and |im| and every partial sum; re and im each
    carry J FMA roundings (J 2^-53 A_k), a table error of at most 8 2^-52 A_k (the product's rounding,
    sincos's last place, and two roundings of an angle below 2 pi: 16 2^-53 |h|) and the gain's
    rounding, (J / 2 + 9) 2^-52 A_k each; W's entries have the same 8 2^-52, acting on |re| + |im| <=
    2 A_k; the 2 K FMAs of the channel chain round partial sums below 2 S, 2 K 2^-52 S in all:
    (J + 18 + 16 + 2 K) 2^-52 S <= E.  A float output adds its conversion, 2^-24 |v| + 2^-149.  A PCM16
    output is lrintf of t = v * 32767.0f: half a step of rounding, the product's 2^-24 |t|, and
    32767 times the float's error.  Derived, not measured."""
    kind = Mx.KINDS[name]
    rng = np.random.default_rng(kind + 31 + 7 * gains)
    for L, T, K, P, n in ((1, 1, 1, 1, 60), (1, 33, 2, 7, 300), (3, 2, 3, 4799, 200), (4, 385, 3, 1920, 700),
                          (40, 401, 5, 4800, 90), (65, 64, 2, 1 << 16, 40)):
        taps = M.channel_taps(T, 1200.0, 192000.0, 2.0 * L) if T > 2 else rng.standard_normal(T).astype(F32)
        centres = np.array([q if abs(q) < P else 0 for q in (0, 1, -1, P // 2, -(P - 1))][:K], np.int32)
        gv = (rng.standard_normal(K) * 2).astype(F32) if gains else None
        scale = 0.02 if kind & Mx.S16 else 1.0                 # PCM16: inside the range, mostly
        x = (rng.standard_normal((K, n)) * scale).astype(F32)
        lens = [n] + [int(v) for v in rng.integers(0, n + 1, K - 1)]
        for r in (0, int(centres[-1])):
            got, cnt = Mx.ref_multiplex(x, lens, kind, P, taps, L, centres, r, gv)
            want, mag = Mx.numpy_multiplex(x, lens, P, taps, L, centres, r, gv)
            assert cnt == want.size == (n - 1) * L + T and not np.any(got[cnt:])
            J = -(-T // L)
            E = (2 * J + 2 * K + 40) * 2.0 ** -52 * mag
            parts = (want.real, want.imag) if kind & Mx.COMPLEX else (want.real,)
            got = got[:cnt].reshape(cnt, -1).astype(np.float64)
            for c, v in enumerate(parts):
                if kind & Mx.S16:
                    t = np.clip(v * 32767.0, -32768.0, 32767.0)
                    bound = 0.5 + 2.0 ** -24 * np.abs(t) + 32767.0 * (E + 2.0 ** -24 * np.abs(v) + 2.0 ** -149)
                    err = np.abs(got[:, c] - t)
                else:
                    bound = E + 2.0 ** -24 * np.abs(v) + 2.0 ** -149
                    err = np.abs(got[:, c] - v)
                assert np.all(err <= bound), (name, L, T, K, P, r, c, float((err / bound).max()))
    # no output where every row is empty; phases without a tap are exact zeros
    out, cnt = Mx.ref_multiplex(np.ones((2, 8), F32), [0, 0], kind, 7, np.ones(3, F32), 5, [1, 2], 0, None, 16)
    assert cnt == 0 and not np.any(out)
    out, cnt = Mx.ref_multiplex(np.ones((1, 8), F32), None, kind, 7, np.ones(2, F32), 5, [3], 1, None, 40)
    rows, phase = out.reshape(40, -1)[:37], np.arange(37) % 5
    assert cnt == 37 and not np.any(rows[phase >= 2]) and np.all(rows[phase == 0, 0] != 0)


def test_the_pcm16_conversion_in_numpy_is_the_restatements():
    lib = Mx.ref_lib()
    lib.mux_ref_s16.restype, lib.mux_ref_s16.argtypes = C.c_int16, [C.c_float]
    rng = np.random.default_rng(16)
    ties = (np.arange(-8, 9, dtype=np.float64) + 0.5) / 32767.0
    v = np.concatenate([rng.standard_normal(2000) * 0.6, ties, [1.0, -1.0, 1.00002, -1.00003, 32768 / 32767.0, 5.0, -5.0,
                        np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-30, -1e-30]]).astype(F32)
    want = np.array([lib.mux_ref_s16(float(a)) for a in v], np.int16)
    assert np.array_equal(Mx.numpy_s16(v), want)
    assert want.max() == 32767 and want.min() == -32768


@pytest.mark.parametrize("cx", [True, False], ids=["complex", "real"])
def test_the_restatements_capture_decodes_every_signal(cx):
    """The closed loop on the CPU: M.synthesize -> mux_ref (L = 4, one channel 12 dB down through gains)
    -> channel_ref -> oracle_rx_stream.  Every channel's bytes hold that signal's payload as one
    contiguous run with at most 2 bytes beside it."""
    c = Mx.three_bell202_rows()
    cfg = O.oracle_config(c["mode"])
    kind = Mx.COMPLEX if cx else 0
    cap, cnt = Mx.ref_multiplex(c["x"], c["lens"], kind, c["P"], c["taps"], c["L"], c["centres"], c["r"], c["gains"])
    assert cnt == (int(c["lens"].max()) - 1) * c["L"] + Mx.MUX_TAPS and cnt <= 40000
    rows = Ch.ref_channelize(cap[:cnt], Ch.COMPLEX if cx else 0, c["P"], c["rx_taps"][cx], c["rx_D"],
                             c["centres"], c["r"])
    assert rows.shape[0] == 3
    for k, payload in enumerate(c["payloads"]):
        decoded = O.oracle_rx_stream(cfg, rows[k])["bytes"]
        assert Ch.payload_condition(decoded, payload), (k, decoded, payload)
        # unit gain: the rows went out at 0.3, the middle one a quarter of that
        assert abs(float(np.abs(rows[k]).max()) / (0.3 * Mx.MUX_GAINS[k]) - 1.0) < 0.15, k
