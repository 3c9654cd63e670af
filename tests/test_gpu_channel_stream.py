"""The channel stream (include/mifsk/channel_stream.h, minimodem_amd/csrc/mifsk_channel_stream.hip) on the device:
a capture fed in pieces gives, concatenated, what channelize gives on the whole capture and what the host
restatement gives (tools/channel_ref.c), bit for bit on the float patterns, counts included.  Pieces are
padded with NaN (PCM16: full scale) behind their lengths, both output arrays of every feed lie between guard
cells, and every row is zero from its count to out_stride.  Rows are a few of the kernel's chunks long (a chunk
is 32 to 2048 outputs, by the number of channels)."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _channel_iq as Iq
import _channel_stream as Cs
from _abi import EINVAL
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
ROW_GUARD_BITS, NOUT_GUARD = 0x7FC0BEEF, -77            # a NaN pattern


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def vec_of(kind):
    return 16 // ((2 if kind & Cs.S16 else 4) * (2 if kind & Cs.COMPLEX else 1))


def make_plan(gpu, kind, P, taps, D, centres, r):
    M, _torch, ctx = gpu
    return M.ChannelPlan(ctx, taps, D, centres, r, P, complex_input=bool(kind & Cs.COMPLEX), s16=bool(kind & Cs.S16))


def chunk_of(K):
    """OB of the kernel: the outputs of one workgroup"""
    nc = 2 if K > 1 else 1
    ncl, shift = (K + nc - 1) // nc, 0
    while (1 << shift) < ncl and shift < 6:
        shift += 1
    return 4 * (64 >> shift) * 8


def default_stride(width, D, iq):
    vec = 2 if iq else 4
    return max(vec, (-(-width // D) + vec - 1) // vec * vec)


def guarded(torch, nrows, out_stride, iq):
    """both outputs with guard cells around them -> (the rows' buffer, the counts' buffer, out=)"""
    per = 2 if iq else 1
    fr = torch.full((nrows * out_stride * per + 2 * GUARD,), ROW_GUARD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    fn = torch.full((nrows + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device="cuda")
    rows = fr[GUARD:GUARD + nrows * out_stride * per]
    out = {"rows": rows.view(nrows, out_stride, 2) if iq else rows.view(nrows, out_stride), "nsamples": fn[GUARD:GUARD + nrows]}
    return fr, fn, out


def padded_piece(kind, pieces, width=None):
    """the feed's tensor from one piece per stream: whole vectors wide, NaN (PCM16: +full scale) behind each
    piece's length -> (numpy [ns, width(, 2)], lengths)"""
    vec = vec_of(kind)
    lens = [p.shape[0] for p in pieces]
    if width is None:
        width = max(vec, (max(lens) + vec - 1) // vec * vec)
    shape = (len(pieces), width) + ((2,) if kind & Cs.COMPLEX else ())
    buf = np.full(shape, 32767, np.int16) if kind & Cs.S16 else np.full(shape, np.nan, F32)
    for s, p in enumerate(pieces):
        buf[s, :lens[s]] = p
    return buf, lens


def feed_all(gpu, cs, kind, xs, cuts, iq, use_lens=True):
    """Feeds stream s the pieces cuts[s] of row xs[s] (every stream as many pieces), every feed between guard
    cells, one synchronisation at the end -> (per stream the concatenated outputs [K, total(, 2)], the counts
    [feeds, ns]).  Checks the guards, the zero tails and the counts against the host's books."""
    M, torch, _ctx = gpu
    plan = cs.plan
    T, D, K = plan.ntaps, plan.decim, plan.nchannels
    ns, nfeeds = len(xs), len(cuts[0])
    assert all(len(c) == nfeeds for c in cuts)
    at = [0] * ns
    kept = []
    for i in range(nfeeds):
        pieces = [xs[s][at[s]:at[s] + cuts[s][i]] for s in range(ns)]
        buf, lens = padded_piece(kind, pieces)
        d = torch.from_numpy(buf).cuda()
        dl = torch.from_numpy(np.asarray(lens, np.int32)).cuda() if use_lens else None
        assert use_lens or all(k == buf.shape[1] for k in lens)
        out_stride = default_stride(buf.shape[1], D, iq)
        fr, fn, out = guarded(torch, ns * K, out_stride, iq)
        res = cs.feed(d, nsamples=dl, out=out, iq=iq)
        assert res is out
        want = [M.channel_stream_outputs(T, D, at[s], cuts[s][i]) for s in range(ns)]
        kept.append((fr, fn, out_stride, want))
        at = [a + c[i] for a, c in zip(at, cuts)]
    torch.cuda.synchronize()
    got = [[] for _ in range(ns)]
    counts = np.zeros((nfeeds, ns), np.int64)
    for i, (fr, fn, out_stride, want) in enumerate(kept):
        fr, fn = fr.cpu().numpy(), fn.cpu().numpy()
        for guard in (fr[:GUARD], fr[-GUARD:]):
            assert np.all(guard.view(np.uint32) == ROW_GUARD_BITS), "feed %d: the guard cells around the rows were written" % i
        for guard in (fn[:GUARD], fn[-GUARD:]):
            assert np.all(guard == NOUT_GUARD), "feed %d: the guard cells around the counts were written" % i
        rows = fr[GUARD:-GUARD].reshape((ns, K, out_stride) + ((2,) if iq else ()))
        nout = fn[GUARD:-GUARD].reshape(ns, K)
        for s in range(ns):
            assert np.all(nout[s] == want[s]), ("feed", i, "stream", s, nout[s], want[s])
            assert not np.any(rows[s][:, want[s]:].view(np.uint32)), "feed %d: row %d is not zero behind its count" % (i, s)
            got[s].append(rows[s][:, :want[s]])
            counts[i, s] = want[s]
    return [np.concatenate(g, axis=1) for g in got], counts


def whole_on_device(gpu, plan, kind, xs, iq):
    """channelize on the whole rows, padded to one stride -> per stream [K, M_s(, 2)]"""
    M, torch, _ctx = gpu
    buf, lens = padded_piece(kind, xs)
    res = M.channelize(plan, torch.from_numpy(buf).cuda(), nsamples=torch.from_numpy(np.asarray(lens, np.int32)).cuda(), iq=iq)
    torch.cuda.synchronize()
    rows, nout = res["rows"].cpu().numpy(), res["nsamples"].cpu().numpy()
    K = plan.nchannels
    out = []
    for s in range(len(xs)):
        assert len(set(nout[s * K:(s + 1) * K])) == 1
        out.append(rows[s * K:(s + 1) * K, :nout[s * K]])
    return out


def ref_whole(x, kind, P, taps, D, centres, r, iq):
    return (Iq.ref_channelize_iq if iq else Ch.ref_channelize)(x, kind, P, taps, D, centres, r)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not Ch.same_f32(got, want):
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError("%s: %d values differ, first at %s: %r != %r" % (
            what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def even_feeds(cuts):
    """every stream as many pieces: the shorter lists get pieces of 0 at their ends"""
    n = max(len(c) for c in cuts)
    return [c + [0] * (n - len(c)) for c in cuts]


# ---------------------------------------------------------------------------
# 1: pieces == whole == restatement
# ---------------------------------------------------------------------------
def size_cases():
    return [pytest.param(*c, id="%s-T%d-D%d-K%d-P%d" % c) for c in Cs.size_cases()]


def sized_case(M, name, T, D, K, P):
    """Two rows of about 3.3 and 2.2 chunks of outputs, each cut its own way.  Every cut list holds pieces of
    0, 1, D - 1, D, T - 1 and T, a run of three pieces shorter than T, one piece of more than two chunks of outputs
    (so a feed runs several workgroups per channel block) and odd lengths; stream 1 gets nothing in the middle
    feed.  With D < T every seam lies T - D .. T - 1 elements into the virtual row: inside a tile of taps but
    for T = 385, D = 1, where the tail's 384 elements put it on the first output of a later chunk (K = 65: 32
    outputs a chunk)."""
    kind = Cs.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + D)
    OB = chunk_of(K)
    big = (2 * OB + 3) * D + T                              # more than 2 OB outputs wherever it falls
    n = [T + int(3.3 * OB) * D + 5 * T + 3, T + int(2.2 * OB) * D + 5 * T + 2 * D + 1]
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
    xs = [Cs.random_rows(rng, kind, 1, k)[0] for k in n]
    cuts = [Cs.cut_points(rng, k, T, D, extra=(big,) if s == 0 else (OB * D + 1,)) for s, k in enumerate(n)]
    cuts = even_feeds(cuts)
    mid = len(cuts[1]) // 2
    cuts[1].insert(mid, 0)
    cuts[0].insert(mid, 7)                                  # (stream 0 goes on while stream 1 waits)
    xs[0] = np.concatenate([xs[0], Cs.random_rows(rng, kind, 1, 7)[0]])
    return kind, taps, Cs.centres_of(rng, K, P), xs, cuts


@pytest.mark.parametrize("name,T,D,K,P", size_cases())
def test_pieces_equal_the_whole_and_the_restatement(gpu, name, T, D, K, P):
    M = gpu[0]
    kind, taps, centres, xs, cuts = sized_case(M, name, T, D, K, P)
    r = int(centres[-1])
    plan = make_plan(gpu, kind, P, taps, D, centres, r)
    cs = M.ChannelStream(plan, 2)
    for iq in (False, True):
        cs.seek(None)
        got, counts = feed_all(gpu, cs, kind, xs, cuts, iq)
        assert np.array_equal(cs.seen(), [x.shape[0] for x in xs])
        assert counts.max() > 2 * chunk_of(K) and (counts == 0).any()
        whole = whole_on_device(gpu, plan, kind, xs, iq)
        for s in range(2):
            assert_same(got[s], whole[s], (name, "iq" if iq else "real", "stream", s, "device"))
            assert_same(got[s], ref_whole(xs[s], kind, P, taps, D, centres, r, iq), (name, iq, s, "restatement"))
    cs.close()
    plan.close()


def test_a_decimation_beyond_the_taps(gpu):
    """D > T: elements between the windows are read by nobody, a cut may fall among them, and the tail is empty
    more often than not"""
    M = gpu[0]
    rng = np.random.default_rng(513)
    T, D, P, K = 5, 13, 4799, 3
    taps, centres = rng.standard_normal(T).astype(F32), Cs.centres_of(rng, K, P)
    n = 3000 * D + 7
    xs = [Cs.random_rows(rng, 0, 1, n)[0], Cs.random_rows(rng, 0, 1, n - 400)[0]]
    cuts = even_feeds([Cs.cut_points(rng, x.shape[0], T, D, extra=(6, 7, 8, 2 * D, 2100 * D)) for x in xs])
    plan = make_plan(gpu, 0, P, taps, D, centres, 5)
    cs = M.ChannelStream(plan, 2)
    for iq in (False, True):
        cs.seek(None)
        got, _counts = feed_all(gpu, cs, 0, xs, cuts, iq)
        for s in range(2):
            assert_same(got[s], ref_whole(xs[s], 0, P, taps, D, centres, 5, iq), ("D > T", iq, s))
    cs.close()
    plan.close()


def test_whole_rows_without_lengths(gpu):
    """without d_nsamples every row's length is the feed's width"""
    M = gpu[0]
    rng = np.random.default_rng(12)
    T, D, P = 63, 7, 4800
    taps, centres = M.channel_taps(T, 400.0, 48000.0, 2.0), Cs.centres_of(rng, 3, P)
    xs = [Cs.random_rows(rng, 0, 1, 1200)[0] for _ in range(2)]
    plan = make_plan(gpu, 0, P, taps, D, centres, 30)
    cs = M.ChannelStream(plan, 2)
    got, _counts = feed_all(gpu, cs, 0, xs, [[400, 4, 796]] * 2, False, use_lens=False)
    for s in range(2):
        assert_same(got[s], ref_whole(xs[s], 0, P, taps, D, centres, 30, False), s)
    cs.close()
    plan.close()


# ---------------------------------------------------------------------------
# 2: special values cross the seam through the tail
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True])
def test_special_values_cross_the_seam(gpu, cx):
    M = gpu[0]
    kind = Cs.COMPLEX if cx else 0
    rng = np.random.default_rng(9)
    T, D, P, n, cut = 64, 7, 65536, 2000, 1000
    taps = M.channel_taps(T, 3000.0, 48000.0, 2.0)
    centres = np.array([0, 1000, -20000, P // 2], np.int32)
    x = Cs.random_rows(rng, kind, 4, n)
    flat = x.reshape(4, n, -1)
    flat[0, cut - 5] = np.nan                               # in the last T - 1 elements of the first piece
    flat[1, cut - 20], flat[1, cut - 2] = np.inf, -np.inf
    flat[2, cut - T + 1:cut] = np.uint32(12345).view(F32)   # subnormals: the whole tail
    flat[3, cut - 9] = -0.0
    plan = make_plan(gpu, kind, P, taps, D, centres, 1000)
    cs = M.ChannelStream(plan, 4)
    for iq in (False, True):
        cs.seek(None)
        got, _counts = feed_all(gpu, cs, kind, list(x), [[cut, n - cut]] * 4, iq)
        whole = whole_on_device(gpu, plan, kind, list(x), iq)
        first = M.channel_stream_outputs(T, D, 0, cut)
        for s in range(4):
            assert_same(got[s], whole[s], ("special", cx, iq, s))
            assert_same(got[s], ref_whole(x[s], kind, P, taps, D, centres, 1000, iq), ("special", cx, iq, s, "restatement"))
        assert np.isnan(got[0][:, first:first + 8]).any() and not np.isnan(got[0][:, first + 12:]).any()
        assert not np.isfinite(got[1][:, first:first + 8]).all()
    cs.close()
    plan.close()


# ---------------------------------------------------------------------------
# 3: beyond 2^32
# ---------------------------------------------------------------------------
def test_a_capture_joined_beyond_two_to_the_32(gpu):
    M = gpu[0]
    rng = np.random.default_rng(32)
    T, D, P, r = 65, 4, 4800, 117
    taps, centres = M.channel_taps(T, 400.0, 48000.0, 2.0), Cs.centres_of(rng, 3, P)
    n0 = D * P * -(-2 ** 32 // (D * P))                     # phase index 0 there
    assert n0 > 2 ** 32 and n0 % (D * P) == 0
    xs = [Cs.random_rows(rng, 0, 1, 3000)[0], Cs.random_rows(rng, 0, 1, 2500)[0]]
    cuts = even_feeds([[1000, 3, 61, 1936], [17, 2000, 483]])
    plan = make_plan(gpu, 0, P, taps, D, centres, r)
    cs = M.ChannelStream(plan, 2)
    first, _counts = feed_all(gpu, cs, 0, xs, cuts, False)                     # from 0
    want = [ref_whole(x, 0, P, taps, D, centres, r, False) for x in xs]
    for s in range(2):
        assert_same(first[s], want[s], ("from 0", s))
    # joined where the phase index is 0 again: the row's outputs from 0
    cs.seek([n0, n0])
    assert np.array_equal(cs.seen(), np.array([n0, n0], np.uint64))
    got, _counts = feed_all_from(gpu, cs, 0, xs, cuts, [n0, n0], [n0 // D] * 2)
    for s in range(2):
        assert_same(got[s], want[s], ("joined at n0", s))
    seen = cs.seen()
    assert seen.dtype == np.uint64 and [int(v) for v in seen] == [n0 + 3000, n0 + 2500] and int(seen.min()) > 2 ** 32
    # joined a elements later: the outputs m >= ceil(a / D) = 1 of the row with a ignored elements in front
    for a in (1, 3):
        cs.seek([n0 + a, n0 + a])
        got, _counts = feed_all_from(gpu, cs, 0, xs, cuts, [n0 + a] * 2, [n0 // D + 1] * 2)
        for s in range(2):
            shifted = ref_whole(np.concatenate([np.zeros(a, F32), xs[s]]), 0, P, taps, D, centres, r, False)
            assert_same(got[s], shifted[:, 1:], ("joined at n0 +", a, s))
        assert [int(v) for v in cs.seen()] == [n0 + a + 3000, n0 + a + 2500]
    # the restatement says the same at that index (the host model, joined there)
    hs = Cs.HostStream(0, P, taps, D, centres, r, seen=n0 + 3)
    assert_same(np.concatenate([hs.feed(xs[0][:1000]), hs.feed(xs[0][1000:])], axis=1), got[0], "host model")
    # the reset: the same pieces again give the first run's outputs
    cs.seek(None)
    assert not cs.seen().any()
    again, _counts = feed_all(gpu, cs, 0, xs, cuts, False)
    for s in range(2):
        assert_same(again[s], first[s], ("after the reset", s))
    with pytest.raises(ValueError):
        cs.seek([2 ** 63 + 1, 0])
    cs.close()
    plan.close()


def feed_all_from(gpu, cs, kind, xs, cuts, seen0, next0):
    """feed_all behind a seek: the host's books start at seen0 with next0 the first output (the counts of the
    first feeds are M(seen + k) less next0, not less M(seen)) -> as feed_all, the books checked here"""
    M, torch, _ctx = gpu
    plan = cs.plan
    T, D, K = plan.ntaps, plan.decim, plan.nchannels
    ns, nfeeds = len(xs), len(cuts[0])
    at, nxt = [0] * ns, list(next0)
    outs = []
    for i in range(nfeeds):
        buf, lens = padded_piece(kind, [xs[s][at[s]:at[s] + cuts[s][i]] for s in range(ns)])
        res = cs.feed(torch.from_numpy(buf).cuda(), nsamples=torch.from_numpy(np.asarray(lens, np.int32)).cuda())
        outs.append(res)
        at = [a + c[i] for a, c in zip(at, cuts)]
    torch.cuda.synchronize()
    got = [[] for _ in range(ns)]
    at = [0] * ns
    counts = np.zeros((nfeeds, ns), np.int64)
    for i, res in enumerate(outs):
        rows = res["rows"].cpu().numpy().reshape(ns, K, -1)
        nout = res["nsamples"].cpu().numpy().reshape(ns, K)
        for s in range(ns):
            at[s] += cuts[s][i]
            upto = Cs.outputs_upto(T, D, seen0[s] + at[s])
            want = max(0, upto - nxt[s])
            nxt[s] = max(nxt[s], upto)
            assert np.all(nout[s] == want), (i, s, nout[s], want)
            assert not np.any(rows[s][:, want:].view(np.uint32))
            got[s].append(rows[s][:, :want])
            counts[i, s] = want
    return [np.concatenate(g, axis=1) for g in got], counts


# ---------------------------------------------------------------------------
# 4: more streams than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_more_streams_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    ns, cut = 65537, 65535
    x = rng.standard_normal((ns, 8)).astype(F32)
    P, taps, D, centres, r = 7, np.array([0.75, -0.5], F32), 1, np.array([3], np.int32), 1
    plan = make_plan(gpu, 0, P, taps, D, centres, r)
    d = torch.from_numpy(x).cuda()
    one, a, b = M.ChannelStream(plan, ns), M.ChannelStream(plan, cut), M.ChannelStream(plan, ns - cut)
    res = []
    for piece in (slice(0, 4), slice(4, 8)):
        p = d[:, piece].contiguous()
        res.append((one.feed(p), a.feed(p[:cut]), b.feed(p[cut:])))
    torch.cuda.synchronize()
    assert np.all(one.seen() == 8) and np.all(a.seen() == 8) and np.all(b.seen() == 8)
    rows = []
    for i, (w, pa, pb) in enumerate(res):
        wr, wn = w["rows"].cpu().numpy(), w["nsamples"].cpu().numpy()
        assert wr.shape == (ns, 4) and np.all(wn == (3, 4)[i])
        assert Ch.same_f32(wr, np.concatenate([pa["rows"].cpu().numpy(), pb["rows"].cpu().numpy()]))
        assert np.array_equal(wn, np.concatenate([pa["nsamples"].cpu().numpy(), pb["nsamples"].cpu().numpy()]))
        rows.append(wr[:, :wn[0]])
    got = np.concatenate(rows, axis=1)
    for s in (0, 1, 65534, 65535, 65536):
        assert_same(got[s][None], Ch.ref_channelize(x[s], 0, P, taps, D, centres, r), s)
    for o in (one, a, b):
        o.close()
    plan.close()


# ---------------------------------------------------------------------------
# 5: refusals with a live object
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_what_a_feed_refuses_leaves_the_object_as_it_was(gpu, iq):
    M, torch, _ctx = gpu
    lib = _lib.load()
    rng = np.random.default_rng(3)
    T, D, P = 65, 4, 4800
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0)
    plan = make_plan(gpu, 0, P, taps, D, [117, -60], 117)
    cs = M.ChannelStream(plan, 2)
    x = Cs.random_rows(rng, 0, 2, 600)
    d = torch.from_numpy(x).cuda()
    cs.feed(d[:, :200].contiguous(), iq=iq)
    n = 400                                                 # the piece under test: ceil(400 / 4) = 100 outputs at most
    piece = d[:, 200:].contiguous()
    need = 100
    fr, fn, out = guarded(torch, 4, need, iq)
    before = (fr.cpu().numpy().copy(), fn.cpu().numpy().copy())
    samples, rows, nout = piece.data_ptr(), out["rows"].data_ptr(), out["nsamples"].data_ptr()
    flag = _lib.CHANNEL_STREAM_IQ if iq else 0
    vec = 2 if iq else 4

    def rc(obj=cs.handle, flags=flag, **kw):
        io = _lib.ChannelIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
        io.d_rows, io.out_stride, io.nout_cap, io.d_nout = rows, need, need, nout
        for k, v in kw.items():
            setattr(io, k, v)
        got = lib.mifsk_channel_stream_feed(obj, C.byref(io), flags, None)
        torch.cuda.synchronize()
        assert np.array_equal(fr.cpu().numpy().view(np.uint32), before[0].view(np.uint32)), kw
        assert np.array_equal(fn.cpu().numpy(), before[1]), kw
        assert np.array_equal(cs.seen(), [200, 200]), kw
        return got

    assert lib.mifsk_channel_stream_feed(cs.handle, None, flag, None) == EINVAL
    assert rc(obj=None) == EINVAL
    for field in ("d_samples", "d_rows", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (4, 8):                                      # misaligned bases
        assert rc(d_samples=samples + off) == EINVAL and rc(d_rows=rows + off) == EINVAL, off
    assert rc(stream_stride=n + 1) == EINVAL and rc(stream_stride=n + 2) == EINVAL
    assert rc(out_stride=need + 1, nout_cap=need) == EINVAL
    assert rc(nout_cap=need + 1) == EINVAL
    for nstreams in (1, 3):                                 # not the object's
        assert rc(nstreams=nstreams) == EINVAL, nstreams
    for bit in (2, 4, 1 << 31):                             # unknown flag bits
        assert rc(flags=flag | bit) == EINVAL, bit
    assert rc(out_stride=need - vec, nout_cap=need - vec) == EINVAL          # one vector below ceil(kmax / D)
    assert rc(nout_cap=need - 1) == EINVAL                  # one below it
    cs.close()
    plan.close()


def test_the_room_a_feed_needs(gpu):
    """the two capacity rules at their edges: kmax is min(nsamples, stream_stride) without d_nsamples and
    stream_stride with it, whatever the lengths say; what passes runs and moves the counters"""
    M, torch, _ctx = gpu
    lib = _lib.load()
    T, D, P = 65, 4, 4800
    plan = make_plan(gpu, 0, P, M.channel_taps(T, 400.0, 48000.0, 2.0), D, [117, -60], 117)
    cs = M.ChannelStream(plan, 2)
    d = torch.from_numpy(Cs.random_rows(np.random.default_rng(4), 0, 2, 400)).cuda()
    lens = torch.from_numpy(np.array([8, 0], np.int32)).cuda()
    fr, fn, out = guarded(torch, 4, 100, False)

    def rc(nsamples, d_nsamples, out_stride, nout_cap):
        io = _lib.ChannelIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = d.data_ptr(), 400, d_nsamples, nsamples, 2
        io.d_rows, io.out_stride, io.nout_cap, io.d_nout = out["rows"].data_ptr(), out_stride, nout_cap, out["nsamples"].data_ptr()
        got = lib.mifsk_channel_stream_feed(cs.handle, C.byref(io), 0, None)
        torch.cuda.synchronize()
        return got

    assert rc(400, None, 96, 96) == EINVAL and rc(400, None, 100, 99) == EINVAL
    assert rc(397, None, 96, 96) == EINVAL                  # ceil(397 / 4) = 100
    assert rc(9999, None, 96, 96) == EINVAL                 # beyond the stride: the stride counts
    assert rc(4, lens.data_ptr(), 96, 96) == EINVAL         # per-row lengths: any may be the stride
    assert rc(4, lens.data_ptr(), 100, 99) == EINVAL
    assert np.array_equal(cs.seen(), [0, 0])
    assert rc(384, None, 96, 96) == 0                       # ceil(384 / 4) = 96
    assert np.array_equal(cs.seen(), [384, 384])
    assert np.all(out["nsamples"].cpu().numpy() == 80)      # (384 - 65) // 4 + 1
    assert rc(4, lens.data_ptr(), 100, 100) == 0
    assert np.array_equal(cs.seen(), [392, 384])
    assert np.array_equal(out["nsamples"].cpu().numpy(), [2, 2, 0, 0])
    got = fr.cpu().numpy()
    assert np.all(got[:GUARD].view(np.uint32) == ROW_GUARD_BITS) and np.all(got[-GUARD:].view(np.uint32) == ROW_GUARD_BITS)
    cs.close()
    plan.close()


# ---------------------------------------------------------------------------
# 6: a side stream
# ---------------------------------------------------------------------------
def test_three_feeds_on_a_side_stream(gpu):
    """tests/test_gpu_row_streams.py's pattern: the outputs are dropped at once and memory of their size is
    refilled on the current stream before anybody waits for the side stream"""
    M, torch, _ctx = gpu
    rng = np.random.default_rng(77)
    T, D, P = 63, 4, 4800
    taps, centres = M.channel_taps(T, 400.0, 48000.0, 1.0), Cs.centres_of(rng, 3, P)
    x = torch.from_numpy(Cs.random_rows(rng, Cs.COMPLEX, 2, 6000)).cuda()
    pieces = [x[:, :2000].contiguous(), x[:, 2000:2050].contiguous(), x[:, 2050:].contiguous()]
    plan = make_plan(gpu, Cs.COMPLEX, P, taps, D, centres, 0)
    cs = M.ChannelStream(plan, 2)
    want = [cs.feed(p, iq=True) for p in pieces]
    want = [{k: t.cpu().numpy().tobytes() for k, t in w.items()} for w in want]
    torch.cuda.synchronize()
    cs.seek(None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = [cs.feed(p, stream=side, iq=True) for p in pieces]
    shapes = [(tuple(t.shape), t.dtype) for r in res for t in r.values()]
    with torch.cuda.stream(side):
        kept = [{k: t.clone() for k, t in r.items()} for r in res]              # behind the kernels
    del res
    again = [torch.full(shape, 85, dtype=dtype, device="cuda") for shape, dtype in shapes]
    side.synchronize()
    torch.cuda.synchronize()
    del again
    for i, (k, w) in enumerate(zip(kept, want)):
        for name in ("rows", "nsamples"):
            assert k[name].cpu().numpy().tobytes() == w[name], "feed %d: %s differs on a side stream" % (i, name)
    assert np.array_equal(cs.seen(side), [6000, 6000])
    cs.close()
    plan.close()


# ---------------------------------------------------------------------------
# 7: end to end
# ---------------------------------------------------------------------------
def unequal_pieces(rng, n, count, vec):
    """about `count` unequal lengths that sum to n, whole vectors but for the last"""
    edges = np.sort(rng.choice(np.arange(1, n // vec), count - 1, replace=False)) * vec
    edges = [0] + [int(e) for e in edges] + [n]
    return [b - a for a, b in zip(edges, edges[1:])]


def test_three_signals_of_a_capture_in_pieces_decode_through_a_resident_session(gpu):
    """ChannelStream.feed -> Session(resident=True).feed, the counts from the host's books: the bytes of every
    channel, concatenated, are demod_batch's on channelize(whole)'s rows"""
    M, torch, ctx = gpu
    c = Ch.three_bell202_iq()
    x, T, D = c["x"], len(c["taps"]), c["D"]
    plan = make_plan(gpu, c["kind"], c["P"], c["taps"], D, c["centres"], c["r"])
    cfg = M.rx_config(c["mode"])
    whole = M.channelize(plan, torch.from_numpy(x).cuda())
    ref = M.results_to_host(M.demod_batch(ctx, cfg, whole["rows"], nsamples=whole["nsamples"], want=("bytes",)))
    cs = M.ChannelStream(plan, 1)
    sess = M.Session(ctx, cfg, 3, resident=True)
    cuts = unequal_pieces(np.random.default_rng(202), x.shape[0], 10, 2)
    assert len(cuts) == 10 and len(set(cuts)) > 5
    got, at, rows = [b"", b"", b""], 0, []
    for i, k in enumerate(cuts):
        buf, _lens = padded_piece(c["kind"], [x[at:at + k]])
        out = cs.feed(torch.from_numpy(buf).cuda(), nsamples=torch.tensor([k], dtype=torch.int32, device="cuda"))
        count = M.channel_stream_outputs(T, D, at, k)      # the host's books: d_nout is not read back to go on
        res = sess.feed(out["rows"], final=(i == len(cuts) - 1), nsamples=[count] * 3)
        assert np.all(out["nsamples"].cpu().numpy() == count)
        rows.append(out["rows"].cpu().numpy()[:, :count])
        for ch in range(3):
            got[ch] += res[ch]["bytes"]
        at += k
    sess.close()
    cs.close()
    plan.close()
    n = int(whole["nsamples"][0])
    assert_same(np.concatenate(rows, axis=1), whole["rows"].cpu().numpy()[:, :n], "rows")
    for ch, payload in enumerate(c["payloads"]):
        assert got[ch] == ref["bytes"][ch, :int(ref["nbytes"][ch])].tobytes(), ch
        assert Ch.payload_condition(got[ch], payload), (ch, got[ch], payload)


def test_three_fm_channels_of_a_capture_in_pieces(gpu):
    """feed(iq=True) -> fm_demod(prev, last): the concatenated audio is fm_demod(channelize(whole, iq=True)),
    bit for bit.  The capture is tests/test_gpu_channel_iq.py's: three Bell-202 messages FM-modulated at their
    centres of a 192 kHz complex capture, summed, with noise."""
    M, torch, ctx = gpu
    words = Iq.fm_messages()
    tx_cfg = M.rx_config("1200", sample_rate=Iq.FS)
    lead = torch.from_numpy(np.array(Iq.LEAD, np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, tx_cfg, torch.from_numpy(words).cuda(), amplitude=1.0, leading_silence=lead)
    n = clean.shape[1]
    dev = M.fm_step(Iq.DEVIATION_HZ, Iq.FS)
    parts = [M.fm_modulate(ctx, clean[k:k + 1], nsamples=lens[k:k + 1], deviation=dev, centre=M.fm_step(off, Iq.FS),
                           amplitude=Iq.CARRIER) for k, off in enumerate(Iq.OFFSETS)]
    capture = (parts[0] + parts[1]) + parts[2]
    noisy = M.impair(ctx, capture.view(1, 2 * n), seed=Iq.SEED, sigma=Iq.fm_sigma(M, 14.0)).view(1, n, 2)
    taps = M.channel_taps(Iq.NTAPS, Iq.CUTOFF, float(Iq.FS), 1.0)
    gain = M.fm_gain(Iq.FS / Iq.D_FM, Iq.DEVIATION_HZ)
    plan = M.ChannelPlan(ctx, taps, Iq.D_FM, Iq.CENTRES, 0, Iq.P_FM, complex_input=True)
    whole = M.channelize(plan, noisy, iq=True)
    want = M.fm_demod(ctx, whole["rows"], nsamples=whole["nsamples"], gain=gain)
    nout = int(whole["nsamples"][0])
    cs = M.ChannelStream(plan, 1)
    state = [torch.zeros((3, 2), dtype=torch.float32, device="cuda") for _ in range(2)]     # prev / last, in turns
    cuts = unequal_pieces(np.random.default_rng(355), n, 9, 2) + [0]
    audio, at = [], 0
    x = noisy[0].cpu().numpy()
    for i, k in enumerate(cuts):
        buf, _lens = padded_piece(Cs.COMPLEX, [x[at:at + k]])
        out = cs.feed(torch.from_numpy(buf).cuda(), nsamples=torch.tensor([k], dtype=torch.int32, device="cuda"), iq=True)
        a = M.fm_demod(ctx, out["rows"], nsamples=out["nsamples"], gain=gain, prev=state[i & 1], last=state[(i & 1) ^ 1])
        count = M.channel_stream_outputs(Iq.NTAPS, Iq.D_FM, at, k)
        assert np.all(out["nsamples"].cpu().numpy() == count)
        audio.append(a.cpu().numpy()[:, :count])
        at += k
    cs.close()
    plan.close()
    got = np.concatenate(audio, axis=1)
    assert got.shape == (3, nout) and nout > 1000
    assert_same(got, want.cpu().numpy()[:, :nout], "audio")
