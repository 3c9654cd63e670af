"""mifsk_impair_batch and mifsk_selftest_gauss (include/mifsk.h, minimodem_amd/csrc/mifsk_impair.hip,
mifsk_gauss.h) against the host restatement tools/impair_ref.c: every output element of every case bit
for bit, no tolerance (a NaN equals a NaN).  Rows are a few thousand samples at most (one case of
65 537 rows of 8); the input and the output rows lie inside larger pools whose cells around them every
call must leave alone."""
import numpy as np
import pytest

import _impair as Im
import _oracle as O
from _impair import F32, same_bits

pytestmark = pytest.mark.gpu

GUARD = 512                         # scalars either side: the rows stay 16-byte aligned
F32_GUARD, S16_GUARD = F32(7.25), 12345
KIND_PAIRS = [(False, False), (True, True), (False, True), (True, False)]       # (PCM16 in, PCM16 out)
KIND_IDS = ["f32-f32", "s16-s16", "f32-s16", "s16-f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _pool(torch, rows, stride, s16):
    """rows x stride scalars inside a pool of guard cells -> (pool, the rows' view)"""
    guard = S16_GUARD if s16 else float(F32_GUARD)
    pool = torch.full((rows * stride + 2 * GUARD,), guard, dtype=torch.int16 if s16 else torch.float32, device="cuda")
    return pool, pool[GUARD:GUARD + rows * stride].view(rows, stride)


def _guards_intact(pool, s16):
    host = pool.cpu().numpy()
    guard = host.dtype.type(S16_GUARD if s16 else F32_GUARD)
    assert np.all(host[:GUARD] == guard) and np.all(host[-GUARD:] == guard), "the guard cells were written"
    return host[GUARD:-GUARD]


def _param(torch, v):
    return torch.from_numpy(np.ascontiguousarray(v, F32)).cuda() if np.ndim(v) else v


def impair(gpu, x, out_s16, out_stride, rows=None, lens=None, nsamples=None, in_place=False, **params):
    """One call between guard cells -> out [rows, out_stride] as numpy.  x: numpy [rows, stride] float32 or
    int16, or None for noise rows (then `rows`); in_place: the output is the input's rows."""
    M, torch, ctx = gpu
    dev = {k: _param(torch, v) for k, v in params.items()}
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    pin = d = None
    if x is not None:
        rows, stride = x.shape
        pin, d = _pool(torch, rows, stride, x.dtype == np.int16)
        d.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    if in_place:
        assert out_stride == stride and out_s16 == (x.dtype == np.int16)
        pout, o = pin, d
    else:
        pout, o = _pool(torch, rows, out_stride, out_s16)
    torch.cuda.synchronize()
    res = M.impair(ctx, d, nsamples=dl if dl is not None else nsamples, out=o, **dev)
    torch.cuda.synchronize()
    assert res is o
    got = _guards_intact(pout, out_s16).reshape(rows, out_stride)
    if pin is not None and not in_place:
        assert same_bits(_guards_intact(pin, x.dtype == np.int16).reshape(x.shape), x), "the input rows were written"
    return got


def assert_same(got, want):
    if not same_bits(got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
        diff = got != want
        if got.dtype != np.int16:
            diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        bad = np.argwhere(diff)
        raise AssertionError("%d elements differ, first at %s: %r != %r" % (
            len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def check(gpu, x, out_s16, out_stride, rows=None, lens=None, nsamples=None, in_place=False, **params):
    got = impair(gpu, x, out_s16, out_stride, rows=rows, lens=lens, nsamples=nsamples, in_place=in_place, **params)
    want = Im.ref_impair(x, lens, out_s16, out_stride, nsamples=nsamples,
                         shape=None if x is not None else (rows, out_stride), **params)
    assert_same(got, want)
    return got


def rows_of(rng, rows, stride, s16):
    if s16:
        return rng.integers(-32768, 32768, size=(rows, stride)).astype(np.int16)
    return (rng.standard_normal((rows, stride)) * 0.3).astype(F32)


# ---------------------------------------------------------------------------
# the transform's corners
# ---------------------------------------------------------------------------
def test_the_transform_at_its_corners_and_on_random_words(gpu):
    _M, _torch, ctx = gpu
    corners = np.array(Im.corner_words(), np.uint32)
    edge = np.stack([np.repeat(corners, corners.size), np.tile(corners, corners.size)], axis=1)
    rng = np.random.default_rng(2016)
    words = np.concatenate([edge, rng.integers(0, 1 << 32, size=(1 << 16, 2), dtype=np.uint64).astype(np.uint32)])
    _rcs, want = Im.ref_words(words)
    got = ctx.selftest_gauss(words)
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        raise AssertionError("%d normals differ, first for words %s: %s != %s" % (
            len(bad), ["%08x" % w for w in words[bad[0][0]]], got[tuple(bad[0])].hex(), want[tuple(bad[0])].hex()))
    # the corners are among them: w = 0xFFFFFFFF gives R = -0.0, and with it a zero of either sign
    i = int(np.flatnonzero((words[:, 0] == 0xFFFFFFFF) & (words[:, 1] == 0))[0])
    assert got[i, 0] == 0.0 and np.signbit(got[i, 0])
    assert ctx.selftest_gauss(np.empty((0, 2), np.uint32)).shape == (0, 2)


# ---------------------------------------------------------------------------
# row shapes
# ---------------------------------------------------------------------------
RAGGED = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1025)
STRIDE_IN, STRIDE_OUT = 1032, 1040


@pytest.mark.parametrize("in_s16,out_s16", KIND_PAIRS, ids=KIND_IDS)
def test_ragged_rows_of_every_kind(gpu, in_s16, out_s16):
    """13 rows of ragged lengths, 1032 elements apart in and 1040 out: the tails are zero up to the output's
    stride (the restatement writes them), and neither pool's guard cells are touched."""
    rng = np.random.default_rng(13 + 2 * in_s16 + out_s16)
    n = len(RAGGED)
    x = rows_of(rng, n, STRIDE_IN, in_s16)
    gain, sigma, dc = (rng.uniform(0.5, 1.5, n).astype(F32), rng.uniform(0.0, 0.4, n).astype(F32),
                       rng.uniform(-0.1, 0.1, n).astype(F32))
    seed = 0xC0FFEE0000000001
    # scalars only
    got = check(gpu, x, out_s16, STRIDE_OUT, lens=RAGGED, seed=seed, gain=0.75, sigma=0.125, dc=0.0625)
    for s, ln in enumerate(RAGGED):
        assert not got[s, ln:].any(), s
    assert got[-1, :1025].any() and got[1, 0] != 0
    # all three per-row arrays; mixed arrays and scalars
    check(gpu, x, out_s16, STRIDE_OUT, lens=RAGGED, seed=seed, gain=gain, sigma=sigma, dc=dc)
    check(gpu, x, out_s16, STRIDE_OUT, lens=RAGGED, seed=seed, gain=gain, sigma=0.25, dc=dc)
    check(gpu, x, out_s16, STRIDE_OUT, lens=RAGGED, seed=seed, gain=1.0, sigma=sigma, dc=0.0)
    # uniform lengths above and below the strides
    got = check(gpu, x, out_s16, STRIDE_OUT, nsamples=2000, seed=seed, sigma=sigma)
    assert got[:, 1031].any() and not got[:, 1032:].any()
    got = check(gpu, x, out_s16, STRIDE_OUT, nsamples=500, seed=seed, sigma=sigma)
    assert not got[:, 500:].any()
    if not in_s16:
        # noise rows: the length is cut at the output's stride alone
        got = check(gpu, None, out_s16, STRIDE_OUT, rows=n, lens=RAGGED, seed=seed, sigma=sigma, dc=dc)
        assert got[-1, :1025].any() and not got[-1, 1025:].any()
        got = check(gpu, None, out_s16, STRIDE_OUT, rows=n, nsamples=2000, seed=seed, sigma=0.2)
        assert got[:, 1039].any()
        check(gpu, None, out_s16, STRIDE_OUT, rows=n, nsamples=500, seed=seed, sigma=0.2, gain=gain)


def test_an_output_narrower_than_the_input(gpu):
    """W = min(nsamples, stream_stride, out_stride): the output's stride cuts the rows; one vector of each kind"""
    rng = np.random.default_rng(8)
    for in_s16, out_s16 in KIND_PAIRS:
        x = rows_of(rng, 3, 264, in_s16)
        for out_stride in (8, 136):
            got = check(gpu, x, out_s16, out_stride, seed=5, sigma=0.1)
            assert got[:, -1].any()
    check(gpu, rows_of(rng, 3, 12, False), False, 4, seed=5, sigma=0.1)
    check(gpu, rows_of(rng, 3, 12, False), False, 20, seed=5, sigma=0.1)        # f32 -> f32: stride % 8 == 4
    # a thread of 8 samples whose second float vector lies behind the row's stride: on the output, on the input
    got = check(gpu, rows_of(rng, 3, 264, True), False, 132, seed=5, sigma=0.1)
    assert got[:, -1].any()
    got = check(gpu, rows_of(rng, 3, 260, False), True, 264, seed=5, sigma=0.1)
    assert got[:, 259].any() and not got[:, 260:].any()


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_in_place_equals_out_of_place(gpu, s16):
    rng = np.random.default_rng(21)
    lens = (1032, 1000, 9, 0, 517)
    x = rows_of(rng, len(lens), STRIDE_IN, s16)
    kw = dict(lens=lens, seed=99, gain=0.9, sigma=0.2, dc=0.01)
    apart = check(gpu, x, s16, STRIDE_IN, **kw)
    assert_same(check(gpu, x, s16, STRIDE_IN, in_place=True, **kw), apart)


# ---------------------------------------------------------------------------
# field positions
# ---------------------------------------------------------------------------
def test_field_positions(gpu):
    rng = np.random.default_rng(31)
    x = rows_of(rng, 3, 64, False)
    for first_stream in (0, (1 << 32) - 2, 1 << 63):                # three rows cross the low word
        for first_sample in (4, (1 << 32) - 4, 1 << 32, (1 << 40) + 8):
            check(gpu, x, False, 64, seed=0x0123456789ABCDEF, sigma=1.0, first_stream=first_stream,
                  first_sample=first_sample)
    # the known answers of the definition: seed 0, stream 0, samples 0 .. 3 and the second set
    got = check(gpu, None, False, 4, rows=1, seed=0, sigma=1.0, gain=0.0)
    assert same_bits(got[0], np.array([float.fromhex(v) for v in (
        "0x1.fb7665db1b649p-1", "-0x1.d96d5ff0aec98p-1", "-0x1.3c373dd6d9558p-1", "-0x1.eda3633cd971p-2")]).astype(F32))
    got = check(gpu, None, False, 4, rows=1, seed=0x01234567DEADBEEF, sigma=1.0, first_stream=5, first_sample=0x500000000)
    assert same_bits(got[0], np.array([float.fromhex(v) for v in (
        "-0x1.2869a07130971p+1", "0x1.09bcef4090687p+1", "0x1.7c6ae00e54393p-1", "0x1.11cf48b0be383p+1")]).astype(F32))


@pytest.mark.parametrize("in_s16,out_s16", [(False, False), (True, True)], ids=["f32", "s16"])
def test_pieces_and_shards_get_the_noise_of_the_whole_batch(gpu, in_s16, out_s16):
    M, torch, ctx = gpu
    rng = np.random.default_rng(41)
    x = rows_of(rng, 4, 4096, in_s16)
    kw = dict(seed=4242, sigma=0.3, gain=0.8, dc=-0.02)
    whole = check(gpu, x, out_s16, 4096, first_stream=10, first_sample=1 << 20, **kw)
    # four pieces of 1024 columns: views of the one input, 4096 elements apart
    d = torch.from_numpy(x).cuda()
    pieces = [M.impair(ctx, d[:, 1024 * k:1024 * (k + 1)], first_stream=10, first_sample=(1 << 20) + 1024 * k, **kw)
              for k in range(4)]
    torch.cuda.synchronize()
    assert all(p.shape == (4, 1024) for p in pieces)
    assert_same(np.concatenate([p.cpu().numpy() for p in pieces], axis=1), whole)
    # two shards of rows
    shards = [M.impair(ctx, d[2 * k:2 * k + 2], first_stream=10 + 2 * k, first_sample=1 << 20, **kw) for k in range(2)]
    torch.cuda.synchronize()
    assert_same(np.concatenate([s.cpu().numpy() for s in shards], axis=0), whole)
    # per-row parameters shard with the rows
    sg = rng.uniform(0.0, 0.5, 4).astype(F32)
    whole = check(gpu, x, out_s16, 4096, seed=7, sigma=sg)
    dsg = torch.from_numpy(sg).cuda()
    shards = [M.impair(ctx, d[2 * k:2 * k + 2], seed=7, sigma=dsg[2 * k:2 * k + 2].contiguous(), first_stream=2 * k)
              for k in range(2)]
    torch.cuda.synchronize()
    assert_same(np.concatenate([s.cpu().numpy() for s in shards], axis=0), whole)


# ---------------------------------------------------------------------------
# row blocks
# ---------------------------------------------------------------------------
def test_more_rows_than_one_launch_holds(gpu):
    """65 537 rows of 8 samples: a second block of rows, with per-row lengths and parameters"""
    rng = np.random.default_rng(51)
    n = 65537
    x = rows_of(rng, n, 8, False)
    lens = np.full(n, 8, np.int32)
    lens[[3, 65535]] = 5
    sigma = (0.1 + 0.01 * (np.arange(n) % 7)).astype(F32)
    dc = (0.001 * (np.arange(n) % 5)).astype(F32)
    got = impair(gpu, x, False, 8, lens=lens, seed=65537, sigma=sigma, dc=dc, first_stream=3)
    for s in (0, 3, 65534, 65535, 65536):
        want = Im.ref_impair(x[s:s + 1], lens[s:s + 1], False, 8, seed=65537, sigma=sigma[s:s + 1], dc=dc[s:s + 1],
                             first_stream=3 + s)
        assert_same(got[s:s + 1], want)
    assert not got[65535, 5:].any() and got[65536].all() and got[65534].all()


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def test_parameters_and_samples_are_data(gpu):
    """NaN, +-Inf and -0.0 samples; sigma 0, negative and infinite; a gain that overflows the float; PCM16
    output that clamps on both sides; a NaN into PCM16 gives 0."""
    rng = np.random.default_rng(61)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 2.0], F32)
    cases = [(1.0, 0.0, 0.0), (1.0, -0.5, 0.0), (1.0, np.inf, 0.0), (3e38, 0.1, 0.0), (1.0, 2.0, 0.0),
             (np.nan, 0.0, 0.0), (0.0, 0.0, -0.0), (-1.0, 0.0, np.inf), (1.0, np.nan, 0.0), (np.inf, 0.0, 0.0)]
    x = np.tile(np.concatenate([special, (rng.standard_normal(248) * 0.3).astype(F32)]), (len(cases), 1))
    gain, sigma, dc = (np.array([c[i] for c in cases], F32) for i in range(3))
    f = check(gpu, x, False, 256, seed=6, gain=gain, sigma=sigma, dc=dc)
    s = check(gpu, x, True, 256, seed=6, gain=gain, sigma=sigma, dc=dc)
    # sigma 0, gain 1: the samples themselves, except that fma(1, -0.0, 0) = +0.0
    assert same_bits(f[0, 4:], x[0, 4:]) and np.isnan(f[0, 0]) and f[0, 1] == np.inf and f[0, 2] == -np.inf
    assert f[0, 3] == 0.0 and not np.signbit(f[0, 3])
    assert s[0, 0] == 0 and s[0, 1] == 32767 and s[0, 2] == -32768          # NaN -> 0; the clamp
    assert np.isinf(f[3, 7]) and np.isfinite(f[3, 5])                       # 3e38 * 2 overflows the float, 3e38 * 1 does not
    assert (s[4] == 32767).any() and (s[4] == -32768).any()                 # sigma 2.0 clamps on both sides
    assert np.isnan(f[5]).all() and not s[5].any()                          # a NaN gain
    assert np.isnan(f[8]).all() and np.isnan(f[9, 4])                       # a NaN sigma; inf * 0.0
    # noise rows with an infinite gain: fma(inf, 0.0, d) is a NaN, nothing is skipped for x = 0
    got = check(gpu, None, False, 8, rows=2, seed=6, gain=np.array([np.inf, 2.0], F32), sigma=0.1)
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()
    # PCM16 samples at the ends of their range
    x16 = np.tile(np.array([-32768, 32767, 0, -1, 1, 16384, -16384, 12345], np.int16), (2, 4))
    check(gpu, x16, False, 32, seed=6, sigma=np.array([0.0, 0.01], F32))
    got = check(gpu, x16, True, 32, seed=6, sigma=np.array([0.0, 0.01], F32))
    assert got[0, 0] == -32767 and got[0, 1] == 32766                       # / 32768, * 32767: not the identity


# ---------------------------------------------------------------------------
# round trip through the receiver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_round_trip_through_the_receiver(gpu, s16):
    """16 Bell-202 streams of 24 bytes at amplitude 0.5, per-row sigma for no noise, 20, 12 and 6 dB: one
    impair call, then demod_batch.  The clean rows go to the host, the restatement makes the noisy ones
    there, and the oracle's frames, episodes and bytes of every stream equal the device's: the noisy batch
    itself is never copied back."""
    M, torch, ctx = gpu
    rng = np.random.default_rng(71)
    cfg, ocfg = M.rx_config("1200"), O.oracle_config("1200")
    n = 16
    words = rng.integers(0x20, 0x7F, size=(n, 24), dtype=np.uint8)
    lead = torch.from_numpy(rng.integers(0, 60, n).astype(np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, cfg, torch.from_numpy(words).cuda(), amplitude=0.5, leading_silence=lead)
    stride = (clean.shape[1] + 7) // 8 * 8
    snr = [float("inf"), 20.0, 12.0, 6.0]
    sigma = np.array([M.snr_sigma(0.5, snr[i % 4]) for i in range(n)], F32)
    assert sigma[0] == 0.0 and abs(sigma[3] - np.sqrt(0.125 / 10 ** 0.6)) < 1e-6
    dsigma = torch.from_numpy(sigma).cuda()
    seed = 0x5EED00000000ABCD
    host_clean, host_lens = clean.cpu().numpy(), lens.cpu().numpy()
    if s16:
        pcm = M.impair(ctx, clean, nsamples=lens, s16_out=True, out=torch.empty((n, stride), dtype=torch.int16, device="cuda"))
        host_pcm = Im.ref_impair(host_clean, host_lens, True, stride)
        assert_same(pcm.cpu().numpy(), host_pcm)
        noisy = M.ingest_s16(ctx, M.impair(ctx, pcm, nsamples=lens, seed=seed, sigma=dsigma), nsamples=lens)
        want16 = Im.ref_impair(host_pcm, host_lens, True, stride, seed=seed, sigma=sigma)
        want = want16.astype(F32) / F32(32768.0)
    else:
        noisy = M.impair(ctx, clean, nsamples=lens, seed=seed, sigma=dsigma)
        want = Im.ref_impair(host_clean, host_lens, False, noisy.shape[1], seed=seed, sigma=sigma)
    out = M.demod_batch(ctx, cfg, noisy, nsamples=lens, want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, want, host_lens, res, threads=4)
    assert bad == []
    for i in range(0, n, 4):                                    # without noise the payload is there
        assert words[i].tobytes() in res["bytes"][i, :int(res["nbytes"][i])].tobytes(), i
    assert int(res["nframes"].sum()) >= 24 * 8
