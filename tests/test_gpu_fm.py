"""mifsk_fm_demod_batch, mifsk_fm_modulate_batch and mifsk_selftest_turn (include/mifsk.h,
minimodem_amd/csrc/mifsk_fm.hip, mifsk_angle.h) against the host restatement tools/fm_ref.c: every output
element of every case bit for bit, no tolerance (a NaN equals a NaN).  Rows are a few thousand samples (one
case of 65 537 rows of 4, one row longer than 64 of the modulator's tiles); every array a call reads or
writes lies inside a larger pool whose cells around it the call must leave alone."""
import numpy as np
import pytest

import _fm as Fm
import _impair as Im
import _oracle as O
from _fm import F32, same_bits

pytestmark = pytest.mark.gpu

GUARD = 512                         # scalars either side: the rows stay 16-byte aligned
GUARDS = {np.dtype(np.float32): F32(7.25), np.dtype(np.int16): np.int16(12345), np.dtype(np.int64): np.int64(-77)}
TILE = 2048                         # the modulator's samples per workgroup: 256 threads x 8
DEV, GAIN = 3000.0 / 48000.0, 48000.0 / 3000.0
KINDS = pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _pool(torch, shape, dtype, fill=None):
    """an array of `shape` inside a pool of guard cells -> (pool, the array's view)"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    pool = torch.full((n + 2 * GUARD,), GUARDS[dtype].item(), dtype=getattr(torch, dtype.name), device="cuda")
    view = pool[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype)).cuda())
    return pool, view


def _inside(pool, shape):
    """the array inside the pool as numpy, the guard cells checked"""
    host = pool.cpu().numpy()
    guard = GUARDS[host.dtype]
    assert np.all(host[:GUARD] == guard) and np.all(host[-GUARD:] == guard), "the guard cells were written"
    return host[GUARD:-GUARD].reshape(shape)


def assert_same(got, want):
    if not same_bits(got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
        diff = got != want
        if got.dtype.kind == "f":
            diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        bad = np.argwhere(diff)
        raise AssertionError("%d elements differ, first at %s: %r != %r" % (
            len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def _dev_lens(torch, lens):
    return None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()


def demod(gpu, iq, out_stride, lens=None, nsamples=None, gain=GAIN, prev=None):
    """One discriminator call between guard cells -> (out [rows, out_stride], last [rows, 2]) as numpy"""
    M, torch, ctx = gpu
    rows = iq.shape[0]
    pin, d = _pool(torch, iq.shape, iq.dtype, iq)
    pout, o = _pool(torch, (rows, out_stride), F32)
    plast, dlast = _pool(torch, (rows, 2), F32)
    pprev, dprev = (None, None) if prev is None else _pool(torch, (rows, 2), F32, prev)
    dl = _dev_lens(torch, lens)
    torch.cuda.synchronize()
    res = M.fm_demod(ctx, d, nsamples=dl if dl is not None else nsamples, gain=gain, prev=dprev, last=dlast, out=o)
    torch.cuda.synchronize()
    assert res is o
    assert same_bits(_inside(pin, iq.shape), iq), "the input rows were written"
    if prev is not None:
        assert same_bits(_inside(pprev, (rows, 2)), np.asarray(prev, F32)), "prev was written"
    return _inside(pout, (rows, out_stride)), _inside(plast, (rows, 2))


def check_demod(gpu, iq, out_stride, lens=None, nsamples=None, gain=GAIN, prev=None):
    got, last = demod(gpu, iq, out_stride, lens=lens, nsamples=nsamples, gain=gain, prev=prev)
    want, want_last = Fm.ref_demod(iq, lens, out_stride, gain=gain, prev=prev, nsamples=nsamples)
    assert_same(got, want)
    assert_same(last, want_last)
    return got, last


def modulate(gpu, x, s16, out_stride, lens=None, nsamples=None, phase0=None, **params):
    """One modulator call between guard cells -> (out [rows, out_stride, 2], phase_out uint64 [rows]) as numpy"""
    M, torch, ctx = gpu
    rows = x.shape[0]
    pin, d = _pool(torch, x.shape, F32, x)
    pout, o = _pool(torch, (rows, out_stride, 2), np.int16 if s16 else F32)
    pph, dph = _pool(torch, (rows,), np.int64)
    pp0, dp0 = (None, None) if phase0 is None else _pool(torch, (rows,), np.int64, np.asarray(phase0, np.uint64).view(np.int64))
    dl = _dev_lens(torch, lens)
    torch.cuda.synchronize()
    res = M.fm_modulate(ctx, d, nsamples=dl if dl is not None else nsamples, phase0=dp0, phase_out=dph, out=o, **params)
    torch.cuda.synchronize()
    assert res is o
    assert same_bits(_inside(pin, x.shape), x), "the input rows were written"
    if phase0 is not None:
        assert np.array_equal(_inside(pp0, (rows,)).view(np.uint64), np.asarray(phase0, np.uint64)), "phase0 was written"
    return _inside(pout, (rows, out_stride, 2)), _inside(pph, (rows,)).view(np.uint64)


def check_modulate(gpu, x, s16, out_stride, lens=None, nsamples=None, phase0=None, **params):
    got, phase = modulate(gpu, x, s16, out_stride, lens=lens, nsamples=nsamples, phase0=phase0, **params)
    want, want_phase = Fm.ref_modulate(x, lens, s16, out_stride, phase0=phase0, nsamples=nsamples, **params)
    assert_same(got, want)
    assert np.array_equal(phase, want_phase), (phase, want_phase)
    return got, phase


def iq_rows(rng, rows, stride, s16):
    if s16:
        return rng.integers(-32768, 32768, size=(rows, stride, 2)).astype(np.int16)
    return (rng.standard_normal((rows, stride, 2)) * 0.5).astype(F32)


# ---------------------------------------------------------------------------
# the angle
# ---------------------------------------------------------------------------
def test_the_angle_at_its_corners_and_on_random_pairs(gpu):
    _M, _torch, ctx = gpu
    cy, cx = Fm.corner_pairs()
    rng = np.random.default_rng(2017)
    pick = rng.permutation(cy.size)[:256]                       # the corner set crossed with itself would repeat
    vals = np.unique(np.concatenate([cy, cx]).view(np.uint64)).view(np.float64)     # ... so: every value with every value
    y = np.concatenate([cy, np.repeat(vals, vals.size), cy[pick], rng.standard_normal(1 << 16),
                        rng.standard_normal(1 << 15) * 10.0 ** rng.uniform(-300, 300, 1 << 15)])
    x = np.concatenate([cx, np.tile(vals, vals.size), cx[pick][::-1], rng.standard_normal(1 << 16),
                        rng.standard_normal(1 << 15) * 10.0 ** rng.uniform(-300, 300, 1 << 15)])
    want = Fm.ref_turns(y, x)
    got = ctx.selftest_turn(y, x)
    if not same_bits(got, want):
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
        i = int(bad[0])
        raise AssertionError("%d angles differ, first for (y, x) = (%s, %s): %s != %s" % (
            len(bad), float(y[i]).hex(), float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()))
    assert np.isnan(got).any() and (got == 0.5).any() and (got == -0.5).any()
    assert ctx.selftest_turn(np.empty(0), np.empty(0)).shape == (0,)


# ---------------------------------------------------------------------------
# the discriminator
# ---------------------------------------------------------------------------
# a thread owns 4 outputs, a wave 256, a workgroup 1024
RAGGED = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1027)
STRIDE_IN, STRIDE_OUT = 1028, 1032


@KINDS
def test_ragged_rows(gpu, s16):
    """13 rows of ragged lengths in one call, 1028 elements apart in and 1032 floats out: the tails are zero up
    to the output's stride, d_last holds every row's last valid sample -- d_prev's, or (0, 0), for the empty row
    -- and no pool's guard cells are touched."""
    rng = np.random.default_rng(17 + s16)
    n = len(RAGGED)
    iq = iq_rows(rng, n, STRIDE_IN, s16)
    prev = (rng.standard_normal((n, 2)) * 0.5).astype(F32)
    got, last = check_demod(gpu, iq, STRIDE_OUT, lens=RAGGED)
    for s, ln in enumerate(RAGGED):
        assert not got[s, ln:].any(), s
    assert not got[:, 0].any() and got[-1, 1:1027].all()        # no sample before the first: 0.0
    assert not last[0].any()
    scale = F32(32768.0) if s16 else F32(1.0)
    assert same_bits(last[3], iq[3, 2].astype(F32) / scale) and same_bits(last[-1], iq[-1, 1026].astype(F32) / scale)
    got, last = check_demod(gpu, iq, STRIDE_OUT, lens=RAGGED, prev=prev)
    assert got[1:, 0].all() and same_bits(last[0], prev[0])
    # uniform lengths: above the strides, and below them
    got, _last = check_demod(gpu, iq, STRIDE_OUT, nsamples=2000, prev=prev)
    assert got[:, 1027].all() and not got[:, 1028:].any()
    got, _last = check_demod(gpu, iq, STRIDE_OUT, nsamples=500, gain=1.0)
    assert got[:, 499].all() and not got[:, 500:].any()
    got, last = check_demod(gpu, iq, STRIDE_OUT, nsamples=0, prev=prev)
    assert not got.any() and same_bits(last, prev)


def test_an_output_narrower_than_the_input_and_odd_strides(gpu):
    """W = min(nsamples, stream_stride, out_stride): the output's stride cuts the rows; float32 rows an odd number
    of 16-byte vectors apart, whose last thread holds one vector only"""
    rng = np.random.default_rng(9)
    for s16 in (False, True):
        iq = iq_rows(rng, 3, 264, s16)
        for out_stride in (4, 8, 136):
            got, last = check_demod(gpu, iq, out_stride)
            assert got[:, -1].all()
    iq = iq_rows(rng, 3, 262, False)
    got, last = check_demod(gpu, iq, 264)
    assert got[:, 261].all() and not got[:, 262:].any() and same_bits(last, iq[:, 261])
    got, last = check_demod(gpu, iq, 264, lens=(261, 259, 258))
    assert same_bits(last[0], iq[0, 260]) and same_bits(last[1], iq[1, 258]) and same_bits(last[2], iq[2, 257])
    check_demod(gpu, iq_rows(rng, 2, 2, False), 4)
    check_demod(gpu, iq_rows(rng, 2, 4, True), 4, lens=(3, 1))


def test_samples_are_data(gpu):
    """rows holding NaN, Inf and nothing but zeros; PCM16 at the ends of its range; any gain"""
    rng = np.random.default_rng(19)
    iq = iq_rows(rng, 6, 64, False)
    iq[0, 5] = (np.nan, 0.25)
    iq[0, 9] = (0.5, np.inf)
    iq[1, 7] = (-np.inf, np.inf)
    iq[1, 20:24] = 0.0
    iq[2] = 0.0
    iq[3] = -0.0
    iq[4, :, 1] = 0.0                                           # the real axis: turns of 0 and 0.5
    iq[5, :, 0] = 0.0
    got, _last = check_demod(gpu, iq, 64)
    assert np.isnan(got[0, 5:7]).all() and np.isnan(got[0, 9:11]).all() and np.isfinite(got[0, 11:]).all()
    assert np.isnan(got[1, 7:9]).all() and not got[1, 20:25].any() and got[1, 25] != 0
    assert not got[2].any() and not got[3].any()
    assert set(np.unique(np.abs(got[4, 1:]))) <= {F32(0.0), F32(0.5 * GAIN)}
    assert set(np.unique(np.abs(got[5, 1:]))) <= {F32(0.0), F32(0.5 * GAIN)}
    for gain in (0.0, -1.0, np.inf, np.nan, 3e38):
        check_demod(gpu, iq, 64, gain=gain)
    x16 = np.tile(np.array([[-32768, 32767], [0, -1], [1, 0], [32767, -32768], [0, 0], [-1, -1], [16384, 3], [-3, -16384]],
                           np.int16), (2, 4, 1))
    got, last = check_demod(gpu, x16, 32, prev=np.array([[1.0, 0.0], [0.0, -1.0]], F32))
    assert not got[:, 4].any() and not got[:, 5].any()


def test_more_rows_than_one_launch_holds(gpu):
    """65 537 rows of 4 samples: a second block of rows, with per-row lengths and previous samples"""
    rng = np.random.default_rng(53)
    n = 65537
    iq = iq_rows(rng, n, 4, False)
    lens = np.full(n, 4, np.int32)
    lens[[3, 65535]] = 2
    lens[65534] = 0
    prev = (rng.standard_normal((n, 2)) * 0.5).astype(F32)
    got, last = check_demod(gpu, iq, 4, lens=lens, prev=prev)
    assert got[65536].all() and not got[65535, 2:].any() and got[65535, :2].all() and not got[65534].any()
    assert same_bits(last[65534], prev[65534]) and same_bits(last[65536], iq[65536, 3])


@KINDS
def test_pieces_through_last_and_prev_equal_the_whole(gpu, s16):
    """two rows of 4 099 samples, in one call and in pieces of 4 k samples, each piece's d_last the next one's
    d_prev: the same floats"""
    M, torch, ctx = gpu
    rng = np.random.default_rng(23 + s16)
    iq = iq_rows(rng, 2, 4100, s16)
    whole, last = check_demod(gpu, iq, 4100, nsamples=4099)
    d = torch.from_numpy(iq).cuda()
    a, prev, parts = 0, None, []
    for b in (4, 1028, 1032, 3080, 4099):
        nxt = torch.empty((2, 2), dtype=torch.float32, device="cuda")
        parts.append(M.fm_demod(ctx, d[:, a:b], gain=GAIN, prev=prev, last=nxt))
        a, prev = b, nxt
    torch.cuda.synchronize()
    assert parts[-1].shape == (2, 1020)                         # 1019 samples, rounded up: the tail is zero
    pieces = np.concatenate([p.cpu().numpy() for p in parts], axis=1)
    assert_same(pieces, whole)
    assert_same(prev.cpu().numpy(), last)


# ---------------------------------------------------------------------------
# the modulator
# ---------------------------------------------------------------------------
MOD_LENS = (0, 1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 5 * TILE + 1, 7, 8, 9, 511, 513)
MOD_STRIDE = 5 * TILE + 4


def audio_rows(rng, rows, stride):
    return rng.uniform(-1.0, 1.0, (rows, stride)).astype(F32)


def phases(rng, rows):
    p = rng.integers(0, 1 << 64, rows, dtype=np.uint64)
    p[0], p[1 % rows] = 0, (1 << 64) - 1
    return p


@KINDS
def test_modulated_rows_of_every_length(gpu, s16):
    """rows that end before, on and behind a tile's border, and inside a thread, a wave and a tile, in one call:
    random start phases with 0 and 2^64 - 1 among them, either sign of the centre, the last phase of every row"""
    rng = np.random.default_rng(29 + s16)
    n = len(MOD_LENS)
    x = audio_rows(rng, n, MOD_STRIDE)
    p0 = phases(rng, n)
    got, phase = check_modulate(gpu, x, s16, MOD_STRIDE, lens=MOD_LENS, phase0=p0, deviation=DEV, centre=-0.013,
                                amplitude=0.8)
    for s, ln in enumerate(MOD_LENS):
        assert not got[s, ln:].any(), s
    assert phase[0] == p0[0] and phase[1] != p0[1]              # the empty row's phase is where it was
    assert got[10, :5 * TILE + 1].any(axis=1).all()
    check_modulate(gpu, x, s16, MOD_STRIDE, lens=MOD_LENS, phase0=p0, deviation=DEV, centre=0.21)
    got, phase = check_modulate(gpu, x, s16, MOD_STRIDE, lens=MOD_LENS, deviation=DEV)         # no start phase: 0
    assert phase[0] == 0
    # uniform lengths: above the strides, and below them
    got, _phase = check_modulate(gpu, x, s16, MOD_STRIDE, nsamples=1 << 20, phase0=p0, deviation=DEV)
    assert got[:, -1].any(axis=1).all()
    got, _phase = check_modulate(gpu, x, s16, MOD_STRIDE, nsamples=TILE + 9, phase0=p0, deviation=-DEV, centre=0.001)
    assert got[:, TILE + 8].any(axis=1).all() and not got[:, TILE + 9:].any()
    # an output narrower than the input, and one vector of it
    got, _phase = check_modulate(gpu, x, s16, TILE + 4, phase0=p0, deviation=DEV)
    assert got[:, -1].any(axis=1).all()
    check_modulate(gpu, x, s16, 4, phase0=p0, deviation=DEV)
    if not s16:
        check_modulate(gpu, x, s16, 2, phase0=p0, deviation=DEV)
        check_modulate(gpu, x, s16, TILE + 2, phase0=p0, deviation=DEV)     # float32: stride % 4 == 2


def test_a_row_of_more_tiles_than_a_wave_scans_at_once(gpu):
    """65 tiles and one sample: the row scan takes its tiles 64 at a time"""
    rng = np.random.default_rng(31)
    n = 65 * TILE + 1
    x = audio_rows(rng, 2, n + 3)
    got, phase = check_modulate(gpu, x, False, n + 3, lens=(n, 64 * TILE), phase0=phases(rng, 2), deviation=DEV,
                                centre=0.03)
    assert got[0, n - 1].any() and not got[0, n:].any() and not got[1, 64 * TILE:].any()


def test_steps_outside_the_range_hold_the_phase(gpu):
    """NaN, Inf and huge samples, a deviation and a centre that put every step outside +-16384 turns: q = 0"""
    rng = np.random.default_rng(37)
    x = audio_rows(rng, 4, 2 * TILE + 8)
    x[0, [0, 5, 6, 7, 8, 2047, 2048, 4000]] = (np.nan, np.inf, -np.inf, 3e38, -3e38, np.nan, np.inf, np.nan)
    x[1, ::3] = np.nan
    x[2] = np.inf
    for s16 in (False, True):
        got, phase = check_modulate(gpu, x, s16, 2 * TILE + 8, phase0=phases(rng, 4), deviation=DEV, centre=0.01)
        assert np.isfinite(got.astype(np.float64)).all()
        assert same_bits(got[0, 5], got[0, 4]) and same_bits(got[0, 8], got[0, 4]) and same_bits(got[2, 100], got[2, 0])
    p0 = phases(rng, 4)
    for params in (dict(deviation=1e9), dict(deviation=DEV, centre=16384.0), dict(deviation=np.nan),
                   dict(deviation=DEV, centre=-np.inf), dict(deviation=16385.0, centre=0.0)):
        got, phase = check_modulate(gpu, x, False, 2 * TILE + 8, phase0=p0, **params)
    got, phase = check_modulate(gpu, np.ones((4, 8), F32), False, 8, phase0=p0, deviation=16384.0)
    assert np.array_equal(phase, p0)
    got, phase = check_modulate(gpu, np.ones((4, 8), F32), False, 8, phase0=p0, deviation=16383.0, amplitude=np.inf)
    assert not np.array_equal(phase, p0)


def test_more_modulated_rows_than_one_launch_holds(gpu):
    """65 537 rows of 4 samples: a second block of rows in both tile launches, every row's phases"""
    rng = np.random.default_rng(59)
    n = 65537
    x = audio_rows(rng, n, 4)
    lens = np.full(n, 4, np.int32)
    lens[[3, 65535]] = 2
    lens[65534] = 0
    got, phase = check_modulate(gpu, x, False, 4, lens=lens, phase0=phases(rng, n), deviation=DEV, centre=-0.1)
    assert got[65536].any(axis=1).all() and not got[65535, 2:].any() and not got[65534].any()


@KINDS
def test_pieces_through_phase_out_and_phase0_equal_the_whole(gpu, s16):
    """two rows of 3 tiles and 3 samples, in one call and in pieces, the phase array handed on in place"""
    M, torch, ctx = gpu
    rng = np.random.default_rng(41 + s16)
    n = 3 * TILE + 3
    x = audio_rows(rng, 2, n + 1)
    p0 = phases(rng, 2)
    whole, end = check_modulate(gpu, x, s16, n + 1, nsamples=n, phase0=p0, deviation=DEV, centre=0.002, amplitude=0.6)
    d = torch.from_numpy(x).cuda()
    phase = torch.from_numpy(p0.view(np.int64).copy()).cuda()
    a, parts = 0, []
    for b in (4, TILE, TILE + 4, 3 * TILE - 4, n):
        parts.append(M.fm_modulate(ctx, d[:, a:b], deviation=DEV, centre=0.002, amplitude=0.6, phase0=phase,
                                   phase_out=phase, s16=s16))
        a = b
    torch.cuda.synchronize()
    pieces = np.concatenate([p.cpu().numpy() for p in parts], axis=1)
    assert_same(pieces[:, :n], whole[:, :n])
    assert not pieces[:, n:].any()
    assert np.array_equal(phase.cpu().numpy().view(np.uint64), end)


# ---------------------------------------------------------------------------
# end to end: transmitter -> FM modulator -> channel -> discriminator -> receiver
# ---------------------------------------------------------------------------
CNR_DB = 14.0                       # carrier to noise over the whole sample rate; the restated chain decodes at 10 dB


@pytest.mark.parametrize("cnr_db", [None, CNR_DB], ids=["clean", "cnr14"])
def test_bell_202_through_an_fm_channel(gpu, cnr_db):
    """8 Bell-202 streams of 16 bytes at full deviation (3 kHz at 48 kHz): synthesize_batch -> fm_modulate ->
    impair over the I/Q rows as real rows of twice the length -> fm_demod with fm_gain -> demod_batch.  The
    transmitted audio goes to the host, the restatements (fm_ref.c, impair_ref.c) make the received audio there
    and the oracle decodes it: every stream's bytes must be the message BEFORE anything of the device's is looked
    at.  Then the device's audio equals the host's bit for bit, its frames and episodes the oracle's, and its
    bytes the message, in every stream."""
    M, torch, ctx = gpu
    rng = np.random.default_rng(81)
    cfg, ocfg = M.rx_config("1200"), O.oracle_config("1200")
    n = 8
    words = rng.integers(0x20, 0x7F, size=(n, 16), dtype=np.uint8)
    lead = torch.from_numpy(rng.integers(0, 60, n).astype(np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, cfg, torch.from_numpy(words).cuda(), amplitude=1.0, leading_silence=lead)
    stride = clean.shape[1]
    assert stride % 4 == 0 and stride < 20000
    sigma = 0.0 if cnr_db is None else M.snr_sigma(1.0, cnr_db)       # carrier power 1, noise power 2 sigma^2
    seed = 0xF00D00000000CAFE
    dev, gain = M.fm_step(3000.0, 48000.0), M.fm_gain(48000.0, 3000.0)
    assert (dev, gain) == (DEV, GAIN)

    host_clean, host_lens = clean.cpu().numpy(), lens.cpu().numpy().astype(np.uint32)
    ref_iq, _phase = Fm.ref_modulate(host_clean, host_lens, False, stride, dev)
    ref_noisy = Im.ref_impair(ref_iq.reshape(n, 2 * stride), 2 * host_lens, False, 2 * stride, seed=seed, sigma=sigma)
    ref_audio, _last = Fm.ref_demod(ref_noisy.reshape(n, stride, 2), host_lens, stride, gain=gain)
    for i in range(n):                                          # the precondition: this noise leaves the oracle whole
        assert O.oracle_rx_stream(ocfg, ref_audio[i, :host_lens[i]])["bytes"] == words[i].tobytes(), i

    iq = M.fm_modulate(ctx, clean, nsamples=lens, deviation=dev)
    lens2 = (lens * 2).to(torch.int32)
    noisy = M.impair(ctx, iq.view(n, 2 * stride), nsamples=lens2, seed=seed, sigma=sigma)
    audio = M.fm_demod(ctx, noisy.view(n, stride, 2), nsamples=lens, gain=gain)
    out = M.demod_batch(ctx, cfg, audio, nsamples=lens, want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    assert_same(iq.cpu().numpy(), ref_iq)
    assert_same(noisy.cpu().numpy(), ref_noisy)
    assert_same(audio.cpu().numpy(), ref_audio)
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, ref_audio, host_lens, res, threads=4)
    assert bad == []
    for i in range(n):
        assert res["bytes"][i, :int(res["nbytes"][i])].tobytes() == words[i].tobytes(), i
    if cnr_db is None:
        err = np.abs(ref_audio[:, 1:].astype(np.float64) - host_clean[:, 1:])
        assert err.max() <= GAIN * (2.0 * np.sqrt(2.0) * 2.0 ** -24 / (2.0 * np.pi) + 2.0 ** -31) + 2.0 ** -23
