"""The channelizer (include/mifsk.h, minimodem_amd/csrc/mifsk_channel.hip) without a device:
what mifsk_channel_plan_create and mifsk_channelize_batch refuse before any HIP call (the context is
a block of zeroed host memory, the device pointers are numbers), the two host helpers, the host
restatement tools/channel_ref.c against a float64 evaluation of the definition, and the condition
the GPU test's end-to-end cases rely on: the restatement's rows decode through the oracle."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _oracle as O
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32


def test_the_python_names_are_public():
    for name in ("channel_taps", "ChannelPlan", "channelize"):
        assert name in M.__all__ and callable(getattr(M, name)), name


def _params(keep, **kw):
    """valid parameters (4 taps, 3 channels, P = 4800) with the fields of kw replaced"""
    taps = np.array(kw.pop("taps_array", [0.25, 0.5, 0.5, 0.25]), F32)
    centres = np.array(kw.pop("centres_array", [117, -60, 2400]), np.int32)
    keep += [taps, centres]
    p = _lib.ChannelParams()
    p.kind, p.flags, p.phase_steps = _lib.FEED_F32, 0, 4800
    p.ntaps, p.taps, p.decim = taps.size, taps.ctypes.data, 1
    p.nchannels, p.centres, p.out_centre = centres.size, centres.ctypes.data, 117
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_plan_create_refuses_before_any_hip_call(lib, fake_ctx):
    ctx, _keep = fake_ctx
    keep = []

    def rc(ctx=ctx, params=True, out=True, **kw):
        h = C.c_void_p()
        return lib.mifsk_channel_plan_create(ctx, C.byref(_params(keep, **kw)) if params else None,
                                             C.byref(h) if out else None)

    assert rc(ctx=None) == EINVAL and rc(params=False) == EINVAL and rc(out=False) == EINVAL
    assert rc(taps=None) == EINVAL and rc(centres=None) == EINVAL
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    assert rc(flags=2) == EINVAL and rc(flags=0x80000001) == EINVAL
    assert rc(ntaps=0) == EINVAL and rc(ntaps=4097) == EINVAL
    assert rc(decim=0) == EINVAL and rc(decim=65536) == EINVAL
    assert rc(nchannels=0) == EINVAL and rc(nchannels=4097) == EINVAL
    assert rc(phase_steps=0) == EINVAL and rc(phase_steps=(1 << 20) + 1) == EINVAL
    for bad in (4800, -4800, 4801, -(1 << 31), (1 << 31) - 1):              # |centre| >= P
        assert rc(centres_array=[117, bad, 0]) == EINVAL, bad
    assert rc(phase_steps=7, centres_array=[0, 7]) == EINVAL and rc(phase_steps=1, centres_array=[1]) == EINVAL
    # K * T above 2^22: 4096 taps x 1025 channels
    assert rc(taps_array=np.zeros(4096, F32), centres_array=np.zeros(1025, np.int32)) == EINVAL
    # the earlier checks win over the later ones
    assert rc(ctx=None, ntaps=0) == EINVAL and rc(kind=5, centres_array=[4800]) == EINVAL
    # the same verdicts from the host-only table entry
    g = np.zeros((4, 2))
    for kw in (dict(ntaps=0), dict(kind=2), dict(phase_steps=0), dict(centres_array=[4800]), dict(decim=0)):
        assert lib.mifsk_channel_table(C.byref(_params(keep, **kw)), 0, g.ctypes.data) == EINVAL, kw
    assert lib.mifsk_channel_table(C.byref(_params(keep)), 3, g.ctypes.data) == EINVAL
    assert lib.mifsk_channel_table(C.byref(_params(keep)), 0, None) == EINVAL
    assert lib.mifsk_channel_table(None, 0, g.ctypes.data) == EINVAL
    assert lib.mifsk_channel_table(C.byref(_params(keep)), 2, g.ctypes.data) == 0


def _io(**kw):
    base = 1 << 20                                  # 16-byte aligned; never dereferenced
    io = _lib.ChannelIO()
    io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = base, 4000, None, 4000, 2
    io.d_rows, io.out_stride, io.nout_cap, io.d_nout = base + (1 << 24), 4000, 4000, base + (1 << 26)
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_channelize_refuses_without_a_plan(lib):
    """mifsk_channelize_batch on a NULL plan comes back with -EINVAL, with or without an io.  The rows'
    kind is the plan's, so what the entry refuses of an io (base, stride per kind, out_stride,
    nout_cap) can only be asked with a plan, and a plan needs a device: those refusals are
    tests/test_gpu_channel.py::test_what_channelize_refuses_of_the_io."""
    assert lib.mifsk_channelize_batch(None, None, None) == EINVAL
    assert lib.mifsk_channelize_batch(None, C.byref(_io()), None) == EINVAL


def test_the_gpu_tests_sampled_sizes_cover_every_value_with_every_kind():
    for name in Ch.KINDS:
        mine = [c for c in Ch.size_cases() if c[0] == name]
        assert {c[1] for c in mine} == set(Ch.TS) and {c[3] for c in mine} == set(Ch.KS)
        assert {c[4] for c in mine} == set(Ch.PS)
        rules = set()
        for _n, T, D, _K, _P in mine:
            rules |= {i for i, d in enumerate(Ch.d_rules(T)) if d == D}
        assert rules == set(range(6)), (name, rules)


def _numpy_taps(T, fc, fs, gain):
    if T == 1:
        return np.array([gain], np.float64)
    t = np.arange(T, dtype=np.float64)
    f = 2.0 * fc / fs
    h = f * np.sinc(f * (t - (T - 1) / 2.0)) * (0.54 - 0.46 * np.cos(2.0 * np.pi * t / (T - 1)))
    return h * (gain / h.sum())


@pytest.mark.parametrize("T", [1, 2, 64, 385])
def test_channel_taps_against_the_formula(lib, T):
    for fc, fs, gain in ((400.0, 48000.0, 2.0), (2400.0, 192000.0, 1.0), (1000.0, 8000.0, 0.5)):
        got = M.channel_taps(T, fc, fs, gain)
        want = _numpy_taps(T, fc, fs, gain)
        assert got.dtype == F32 and got.shape == (T,)
        # the formula in float64, rounded once: the same float.  numpy's sin, cos and sum may differ
        # from the C library's in the last places of a double, so a tap whose double lies within
        # 2^-50 (relative) of a float rounding boundary may be the float on either side of it
        exact = got == want.astype(F32)
        below, above = (want * (1.0 - 2.0 ** -50)).astype(F32), (want * (1.0 + 2.0 ** -50)).astype(F32)
        at_boundary = (below != above) & ((got == below) | (got == above))
        assert np.all(exact | at_boundary), (T, fc, np.flatnonzero(~(exact | at_boundary)))
        assert np.count_nonzero(~exact) <= 1, (T, fc)
        assert abs(float(got.astype(np.float64).sum()) - gain) <= T * 2.0 ** -24 * gain
    if T > 1:
        assert np.array_equal(M.channel_taps(T, 400.0, 48000.0)[::-1], M.channel_taps(T, 400.0, 48000.0))
    out = np.zeros(4, F32)
    for bad in ((0, 400.0, 48000.0), (4097, 400.0, 48000.0), (4, 0.0, 48000.0), (4, 400.0, 0.0),
                (4, float("nan"), 48000.0), (4, 400.0, float("inf"))):
        assert lib.mifsk_channel_taps(bad[0], bad[1], bad[2], 1.0, out.ctypes.data) == EINVAL, bad
    assert lib.mifsk_channel_taps(4, 400.0, 48000.0, 1.0, None) == EINVAL


@pytest.mark.parametrize("P", [7, 4799, 4800, 1 << 20])
def test_channel_table_equals_the_restatement_bit_for_bit(P):
    rng = np.random.default_rng(P)
    taps = np.concatenate([M.channel_taps(385, 400.0, 48000.0, 2.0), rng.standard_normal(40).astype(F32)])
    centres = np.array([0, 1, -1, P // 2, -(P - 1)], np.int32)
    for k, q in enumerate(centres):
        got = M.channel_table(taps, centres, k, P)
        want = Ch.ref_table(P, taps, q)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (P, q)
    # q and q - P are the same channel; q = 0 is the taps themselves
    g0 = M.channel_table(taps, centres, 0, P)
    assert np.array_equal(g0[:, 0], taps.astype(np.float64)) and not np.any(g0[:, 1])
    assert np.array_equal(M.channel_table(taps, centres, 1, P), M.channel_table(taps, centres, 4, P))


def _random_row(rng, kind, n):
    shape = (n, 2) if kind & Ch.COMPLEX else (n,)
    if kind & Ch.S16:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return rng.standard_normal(shape).astype(F32)


@pytest.mark.parametrize("name", list(Ch.KINDS))
def test_the_restatement_against_float64(name):
    """|restatement - float64| <= 2^-24 |v| + 2^-149 + (2 T + 8) 2^-52 sum_t |h[t]| (|xr| + |xi|): one
    rounding per FMA (at most 2 T on a sum whose partial sums the last term bounds), per table product
    and per sincos result, plus the final conversion to float.  Derived, not measured."""
    kind = Ch.KINDS[name]
    rng = np.random.default_rng(kind + 11)
    for T, D, P, n in ((1, 1, 7, 50), (2, 3, 4799, 300), (65, 4, 4800, 1500), (385, 7, 1 << 16, 3000)):
        taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
        centres = np.array([0, 1, -1, P // 2, -(P - 1), int(rng.integers(0, P))], np.int32)
        for r in (0, int(centres[5])):
            x = _random_row(rng, kind, n)
            got = Ch.ref_channelize(x, kind, P, taps, D, centres, r)
            want, mag = Ch.numpy_channelize(x, kind, P, taps, D, centres, r)
            assert got.shape == want.shape == (6, (n - T) // D + 1)
            bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -149 + (2 * T + 8) * 2.0 ** -52 * mag[None, :]
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= bound), (name, T, D, P, float((err / bound).max()))
    # no output where the row is shorter than the taps
    assert Ch.ref_channelize(_random_row(rng, kind, 64), kind, 4800, np.ones(65, F32), 1, [3], 0).shape == (1, 0)


@pytest.mark.parametrize("make", [Ch.three_bell103, Ch.three_bell202_iq])
def test_the_restatements_rows_decode_every_signal(make):
    """End to end on the CPU: restatement, then oracle_rx_stream.  Every channel's bytes hold that
    signal's payload as one contiguous run with at most 2 bytes beside it; the plain real row decodes
    only the signal on the nominal tones."""
    c = make()
    cfg = O.oracle_config(c["mode"])
    rows = Ch.ref_channelize(c["x"], c["kind"], c["P"], c["taps"], c["D"], c["centres"], c["r"])
    assert rows.shape[0] == 3 and c["x"].shape[0] <= 40000
    for k, payload in enumerate(c["payloads"]):
        decoded = O.oracle_rx_stream(cfg, rows[k])["bytes"]
        assert Ch.payload_condition(decoded, payload), (k, decoded, payload)
    if not c["kind"] & Ch.COMPLEX:
        plain = O.oracle_rx_stream(cfg, c["x"])["bytes"]
        assert c["payloads"][0] in plain
        assert c["payloads"][1] not in plain and c["payloads"][2] not in plain
