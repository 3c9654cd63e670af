"""The multiplexer stream (include/mifsk/mux_stream.h, minimodem_amd/csrc/mifsk_mux_stream.hip) on the device: rows
fed in pieces give, concatenated, what multiplex gives on the whole rows and what the host restatement gives
(tools/mux_ref.c), bit for bit, counts included.  Pieces are padded with NaN behind their lengths, both output
arrays of every feed lie between guard cells, and every row is zero from its count to out_stride.  Rows are a few
of the kernel's workgroups long (a workgroup is 2048 outputs)."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _channel_iq as Iq
import _mux as Mx
import _mux_iq as Mq
import _mux_stream as Ms
from _abi import EINVAL
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64                                              # 32-bit words: the bases stay 16-byte aligned
ROW_GUARD_BITS, NOUT_GUARD = 0x7FC0BEEF, -77            # a NaN pattern (PCM16: two odd values)
CHUNK = 256 * 8                                         # outputs of one workgroup of the kernel


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def make_plan(gpu, kind, P, taps, L, centres, r, gains=None):
    M, _torch, ctx = gpu
    return M.MuxPlan(ctx, taps, L, centres, r, P, complex_output=bool(kind & Ms.COMPLEX), s16=bool(kind & Ms.S16),
                     gains=gains)


def kind_of(plan):
    return (Ms.COMPLEX if plan.complex_output else 0) | (Ms.S16 if plan.s16 else 0)


def default_stride(kind, width, L):
    v = Ms.vec_of(kind)
    return max(v, (width * L + v - 1) // v * v)


def guarded(torch, kind, ns, out_stride):
    """both outputs with guard cells around them -> (the rows' buffer, the counts' buffer, out=)"""
    per = 2 if kind & Ms.COMPLEX else 1
    esz = 2 if kind & Ms.S16 else 4
    words = ns * out_stride * per * esz // 4
    fr = torch.full((words + 2 * GUARD,), ROW_GUARD_BITS, dtype=torch.int32, device="cuda")
    fn = torch.full((ns + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device="cuda")
    rows = fr[GUARD:GUARD + words].view(torch.int16 if kind & Ms.S16 else torch.float32)
    out = {"rows": rows.view((ns, out_stride, 2) if per == 2 else (ns, out_stride)), "nsamples": fn[GUARD:GUARD + ns]}
    return fr, fn, out


def read_guarded(kind, ns, fr, fn, what):
    """the guards checked -> (rows [ns, out_stride(, 2)], counts [ns]) as numpy"""
    fr, fn = fr.cpu().numpy(), fn.cpu().numpy()
    for guard in (fr[:GUARD], fr[-GUARD:]):
        assert np.all(guard.view(np.uint32) == ROW_GUARD_BITS), "%s: the guard cells around the rows were written" % (what,)
    for guard in (fn[:GUARD], fn[-GUARD:]):
        assert np.all(guard == NOUT_GUARD), "%s: the guard cells around the counts were written" % (what,)
    rows = fr[GUARD:-GUARD].view(np.int16 if kind & Ms.S16 else F32)
    return rows.reshape((ns, -1, 2) if kind & Ms.COMPLEX else (ns, -1)), fn[GUARD:-GUARD]


def padded_piece(iq, pieces, width=None):
    """the feed's tensor from one piece per row: whole vectors wide, NaN behind each piece's length ->
    (numpy [rows, width(, 2)], lengths)"""
    vec = 2 if iq else 4
    lens = [p.shape[0] for p in pieces]
    if width is None:
        width = max(vec, (max(lens) + vec - 1) // vec * vec)
    buf = np.full((len(pieces), width) + ((2,) if iq else ()), np.nan, F32)
    for row, p in enumerate(pieces):
        buf[row, :lens[row]] = p
    return buf, lens


def pieces_of(xs, ends, at, cuts, i):
    """feed i's piece of every row of every stream: row k of stream s from at[s] on, cuts[s][i] long, cut at the
    row's end ends[s][k]"""
    out = []
    for s, x in enumerate(xs):
        for k in range(x.shape[0]):
            e = x.shape[1] if ends is None else ends[s][k]
            out.append(x[k, min(at[s], e):min(at[s] + cuts[s][i], e)])
    return out


def feed_all(gpu, ms, xs, cuts, ends=None, use_lens=True):
    """Feeds stream s the pieces cuts[s] of its rows xs[s] ([K, n_s(, 2)]; every stream as many pieces), every
    feed between guard cells, one synchronisation at the end -> per stream the concatenated outputs [total(, 2)].
    Checks the guards, the zero tails and the counts against the host's k L."""
    M, torch, _ctx = gpu
    plan, iq = ms.plan, ms.iq
    kind, L, K = kind_of(plan), plan.interp, plan.nchannels
    ns, nfeeds = len(xs), len(cuts[0])
    assert all(len(c) == nfeeds for c in cuts) and ns == ms.nstreams
    at = [0] * ns
    kept = []
    for i in range(nfeeds):
        pieces = pieces_of(xs, ends, at, cuts, i)
        buf, lens = padded_piece(iq, pieces)
        d = torch.from_numpy(buf).cuda()
        dl = torch.from_numpy(np.asarray(lens, np.int32)).cuda() if use_lens else None
        assert use_lens or all(k == buf.shape[1] for k in lens)
        out_stride = default_stride(kind, buf.shape[1], L)
        fr, fn, out = guarded(torch, kind, ns, out_stride)
        res = ms.feed(d, nsamples=dl, out=out)
        assert res is out
        want = [max(lens[s * K:(s + 1) * K]) * L for s in range(ns)]
        kept.append((fr, fn, want))
        at = [a + c[i] for a, c in zip(at, cuts)]
    torch.cuda.synchronize()
    got = [[] for _ in range(ns)]
    for i, (fr, fn, want) in enumerate(kept):
        rows, nout = read_guarded(kind, ns, fr, fn, "feed %d" % i)
        for s in range(ns):
            assert nout[s] == want[s], ("feed", i, "stream", s, nout[s], want[s])
            assert not np.any(rows[s][want[s]:].view(np.uint16)), "feed %d: row %d is not zero behind its count" % (i, s)
            got[s].append(rows[s][:want[s]])
    return [np.concatenate(g, axis=0) for g in got]


def whole_on_device(gpu, plan, iq, xs, ends=None, extra=0):
    """multiplex on the whole rows, padded with NaN to one stride, room for `extra` more outputs than the longest
    row's N L -> per stream (the row [out_stride(, 2)], the count)"""
    M, torch, _ctx = gpu
    K, L = plan.nchannels, plan.interp
    rows = [x[k, :(x.shape[1] if ends is None else ends[s][k])] for s, x in enumerate(xs) for k in range(x.shape[0])]
    buf, lens = padded_piece(iq, rows)
    cap = max(Mx.full_outputs(max(lens), L, plan.ntaps), max(lens) * L + extra)
    res = M.multiplex(plan, torch.from_numpy(buf).cuda(), nsamples=torch.from_numpy(np.asarray(lens, np.int32)).cuda(),
                      nout_cap=cap, iq=iq)
    torch.cuda.synchronize()
    out, nout = res["rows"].cpu().numpy(), res["nsamples"].cpu().numpy()
    return [(out[s], int(nout[s])) for s in range(len(xs))]


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not Ms.same_bits(got, want):
        diff = got != want
        if got.dtype != np.int16:
            diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        bad = np.argwhere(diff)
        raise AssertionError("%s: %d values differ, first at %s: %r != %r" % (
            what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def centres_of(rng, K, P):
    fixed = [q for q in (0, -1, P // 2, -(P - 1), 1, -(P // 2)) if abs(q) < P] or [0]
    more = rng.integers(-(P - 1), P, max(0, K - len(fixed))) if P > 1 else np.zeros(max(0, K - len(fixed)), int)
    return np.array((fixed + [int(v) for v in more])[:K] + [0] * max(0, K - len(fixed) - len(more)), np.int32)


def taps_of(M, rng, T, L):
    return M.channel_taps(T, 1200.0, 192000.0, 2.0 * L) if T > 2 else rng.standard_normal(T).astype(F32)


def zeros_piece(iq, n):
    return np.zeros((n, 2) if iq else (n,), F32)


def drain(gpu, ms, H):
    """H samples of +0.0 to every row -> per stream the H L outputs"""
    K, ns = ms.plan.nchannels, ms.nstreams
    xs = [np.zeros((K, H, 2) if ms.iq else (K, H), F32) for _ in range(ns)]
    return feed_all(gpu, ms, xs, [[H]] * ns)


# ---------------------------------------------------------------------------
# 1: pieces == whole == restatement, then the drain
# ---------------------------------------------------------------------------
def size_cases():
    return [pytest.param(*c, id="%s-L%d-T%d-K%d-P%d" % c) for c in Ms.size_cases()]


def sized_case(M, L, T, K, P, iq, seed=0):
    """Two streams, each cut its own way.  Every cut list holds pieces of 0, 1, 7, 8, 9, H - 1, H and H + 1, a run
    of three pieces shorter than H and odd lengths; stream 0 has one piece of more than two workgroups of outputs,
    stream 1 one of more than one; stream 1 gets nothing in the middle feed."""
    rng = np.random.default_rng(1000 * T + 10 * K + L + seed)
    H = Ms.drain_of(T, L)
    big = -(-(2 * CHUNK + 400) // L) + 3
    assert big * L > 2 * CHUNK
    n = [big + 26 + 5 * H + 61, -(-(CHUNK + 200) // L) + 26 + 5 * H + 50]
    cuts = [Ms.cut_points(rng, n[0], H, extra=(big,)), Ms.cut_points(rng, n[1], H, extra=(-(-(CHUNK + 200) // L),))]
    cuts = Ms.even_feeds(cuts)
    mid = len(cuts[1]) // 2
    cuts[1].insert(mid, 0)
    cuts[0].insert(mid, 7)                                  # (stream 0 goes on while stream 1 waits)
    n[0] += 7
    xs = [Ms.random_rows(rng, iq, K, k, 0.05) for k in n]
    taps = taps_of(M, rng, T, L)
    centres = centres_of(rng, K, P)
    gains = (rng.standard_normal(K) + 1.5).astype(F32) if (L + K) % 2 else None
    return H, taps, centres, gains, xs, cuts


def check_case(gpu, kind, L, T, K, P, iq, seed=0):
    M = gpu[0]
    H, taps, centres, gains, xs, cuts = sized_case(M, L, T, K, P, iq, seed)
    r = int(centres[-1])
    plan = make_plan(gpu, kind, P, taps, L, centres, r, gains)
    ms = M.MuxStream(plan, 2, iq=iq)
    got = feed_all(gpu, ms, xs, cuts)
    assert np.array_equal(ms.seen(), [x.shape[1] for x in xs])
    rest = drain(gpu, ms, H)
    assert np.array_equal(ms.seen(), [x.shape[1] + H for x in xs])
    whole = whole_on_device(gpu, plan, iq, xs, extra=H * L)
    for s in range(2):
        N = xs[s].shape[1]
        row, count = whole[s]
        assert count == (N - 1) * L + T and got[s].shape[0] == N * L
        assert_same(got[s], row[:N * L], (kind, iq, "stream", s, "device"))
        ref, rcount = Ms.ref_whole(xs[s], None, kind, P, taps, L, centres, r, gains=gains, iq=iq, out_stride=(N + H) * L)
        assert rcount == count
        both = np.concatenate([got[s], rest[s]], axis=0)
        assert_same(both, ref, (kind, iq, "stream", s, "restatement"))
        assert_same(rest[s], row[N * L:(N + H) * L], (kind, iq, "stream", s, "the drain on the device"))
    ms.close()
    plan.close()


@pytest.mark.parametrize("name,L,T,K,P", size_cases())
def test_pieces_equal_the_whole_and_the_restatement(gpu, name, L, T, K, P):
    for iq in (False, True):
        check_case(gpu, Ms.KINDS[name], L, T, K, P, iq)


# ---------------------------------------------------------------------------
# 2: channels staged several at a time and one at a time; small shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,T,K,iq", [("complex-f32", 2, 9, 64, False), ("complex-f32", 2, 9, 64, True),
                                           ("real-s16", 1, 2000, 5, True), ("real-f32", 1, 4096, 2, False)],
                         ids=["5-channels-at-a-time", "5-channels-at-a-time-iq", "1-at-a-time-68KB-iq", "1-at-a-time-119KB"])
def test_channels_staged_in_several_batches(gpu, name, L, T, K, iq):
    """tests/test_gpu_mux.py's large-LDS shapes at piece size: the tail of up to 4095 samples is staged in front of
    the piece, and a piece shorter than the tail leaves a tail made of two pieces"""
    M = gpu[0]
    kind = Ms.KINDS[name]
    rng = np.random.default_rng(T + K)
    H = Ms.drain_of(T, L)
    big = (2 * CHUNK + 400) // L + 4
    cuts = [[H + 1, 9, big, 0, max(1, H // 2), 701], [333, big // 2, H, 1, 8, H + 7]]
    xs = [Ms.random_rows(rng, iq, K, sum(c), 0.05) for c in cuts]
    taps = taps_of(M, rng, T, max(L, 4))
    centres = centres_of(rng, K, 4800)
    r = int(centres[-1])
    plan = make_plan(gpu, kind, 4800, taps, L, centres, r)
    ms = M.MuxStream(plan, 2, iq=iq)
    got = feed_all(gpu, ms, xs, cuts)
    whole = whole_on_device(gpu, plan, iq, xs)
    for s in range(2):
        N = xs[s].shape[1]
        assert_same(got[s], whole[s][0][:N * L], (name, s, "device"))
        ref, _ = Ms.ref_whole(xs[s], None, kind, 4800, taps, L, centres, r, iq=iq, out_stride=N * L)
        assert_same(got[s], ref, (name, s, "restatement"))
    ms.close()
    plan.close()


@pytest.mark.parametrize("name,L,T,K,P", [("real-f32", 40, 17, 3, 4800), ("complex-f32", 300, 700, 3, 7),
                                          ("real-s16", 300, 299, 2, 4800), ("complex-s16", 5, 33, 65, 4800)],
                         ids=["T-below-L", "L300-a-group-spans-workgroups", "L300-T-below-L", "K65"])
def test_small_shapes(gpu, name, L, T, K, P):
    """T < L: the phases phi >= T are exact zeros and there is no tail, the phase alone continues.  L = 300: a group
    of 8 L outputs spans several workgroups.  K = 65: more channels than a wave has lanes."""
    for iq in (False, True):
        check_case(gpu, Ms.KINDS[name], L, T, K, P, iq, seed=5)


# ---------------------------------------------------------------------------
# 3: special values cross a seam through the tail
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_special_values_cross_the_seam(gpu, iq):
    """non-finite samples, taps and gains and a tail full of subnormals, rows equally long: the pieces are the
    whole, bit for bit, on [0, N L)"""
    M = gpu[0]
    rng = np.random.default_rng(9)
    L, T, K, P, n, cut = 4, 100, 4, 65536, 1400, 700
    H = Ms.drain_of(T, L)
    centres = np.array([0, 1000, -20000, P // 2], np.int32)
    x = Ms.random_rows(rng, iq, K, n, 0.3)
    flat = x.reshape(K, n, -1)
    flat[0, cut - 5] = np.nan                               # in the last H samples of the first piece
    flat[1, cut - 20], flat[1, cut - 2] = np.inf, -np.inf
    flat[2, cut - H:cut] = np.uint32(12345).view(F32)       # subnormals: the whole tail
    flat[3, cut - 9] = -0.0
    for bad_taps in (False, True):
        taps = M.channel_taps(T, 3000.0, 192000.0, 2.0 * L)
        gains = np.array([1.0, -0.5, 2.0, 1.0], F32)
        if bad_taps:
            taps[5], taps[50], taps[97] = np.inf, np.nan, -np.inf
            gains[3] = np.inf
        for kind in (0, Ms.COMPLEX | Ms.S16):
            plan = make_plan(gpu, kind, P, taps, L, centres, 1000, gains)
            ms = M.MuxStream(plan, 1, iq=iq)
            got = feed_all(gpu, ms, [x], [[cut, 3, n - cut - 3]])[0]
            whole = whole_on_device(gpu, plan, iq, [x])[0][0]
            assert_same(got, whole[:n * L], ("special", iq, bad_taps, kind, "device"))
            ref, _ = Ms.ref_whole(x, None, kind, P, taps, L, centres, 1000, gains=gains, iq=iq, out_stride=n * L)
            assert_same(got, ref, ("special", iq, bad_taps, kind, "restatement"))
            if kind == 0:
                assert np.isnan(got[cut * L:(cut + 8) * L]).any()
                assert bad_taps or not np.isnan(got[(cut + H + 1) * L:]).any()
            ms.close()
            plan.close()


# ---------------------------------------------------------------------------
# 4: ragged rows inside a feed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_ragged_rows_equal_the_restatement_and_the_batch(gpu, iq):
    """rows of a stream that end at different lengths, one of them empty from the start and one that ends in the
    middle of a feed: the host model feed by feed, and (finite taps) the batch on the rows, drain included"""
    M = gpu[0]
    rng = np.random.default_rng(44)
    L, T, K, P = 3, 200, 5, 4800
    H = Ms.drain_of(T, L)
    taps, centres = taps_of(M, rng, T, L), centres_of(rng, K, P)
    gains = (rng.standard_normal(K) + 1.5).astype(F32)
    r = int(centres[2])
    ends = [[1500, 0, 1499, 777, 64], [40, 900, 1200, 1200, 3]]
    xs = [Ms.random_rows(rng, iq, K, 1500, 0.3), Ms.random_rows(rng, iq, K, 1200, 0.3)]
    cuts = Ms.even_feeds([[700, 70, 9, 721, H], [1000, 0, 199, 1, H]])
    for s in range(2):                                      # the drain: +0.0 behind the longest row
        xs[s] = np.concatenate([xs[s], np.zeros_like(xs[s][:, :H])], axis=1)
        ends[s] = [e if e < xs[s].shape[1] - H else e + H for e in ends[s]]
    for kind in (Ms.COMPLEX, Ms.S16):
        plan = make_plan(gpu, kind, P, taps, L, centres, r, gains)
        ms = M.MuxStream(plan, 2, iq=iq)
        got = feed_all(gpu, ms, xs, cuts, ends=ends)
        for s in range(2):
            N = xs[s].shape[1] - H
            hs = Ms.HostMuxStream(kind, P, taps, L, centres, r, gains=gains, iq=iq)
            at, model = 0, []
            for c in cuts[s]:
                model.append(hs.feed([xs[s][k, min(at, e):min(at + c, e)] for k, e in enumerate(ends[s])]))
                at += c
            assert_same(got[s], np.concatenate(model, axis=0), (kind, s, "host model"))
            real_ends = [min(e, N) for e in ends[s]]
            ref, count = Ms.ref_whole(xs[s][:, :N], real_ends, kind, P, taps, L, centres, r, gains=gains, iq=iq,
                                      out_stride=(N + H) * L)
            assert count == (N - 1) * L + T
            assert_same(got[s], ref, (kind, s, "the batch's restatement"))
        whole = whole_on_device(gpu, plan, iq, [x[:, :x.shape[1] - H] for x in xs],
                                ends=[[min(e, x.shape[1] - H) for e in en] for en, x in zip(ends, xs)], extra=H * L)
        for s in range(2):
            assert_same(got[s], whole[s][0][:got[s].shape[0]], (kind, s, "the batch on the device"))
        ms.close()
        plan.close()


def test_whole_rows_without_lengths(gpu):
    """without d_nsamples every row's length is the feed's width"""
    M = gpu[0]
    rng = np.random.default_rng(12)
    L, T, K, P = 4, 63, 3, 4800
    taps, centres = taps_of(M, rng, T, L), centres_of(rng, K, P)
    xs = [Ms.random_rows(rng, False, K, 1200, 0.3) for _ in range(2)]
    plan = make_plan(gpu, 0, P, taps, L, centres, 30)
    ms = M.MuxStream(plan, 2)
    got = feed_all(gpu, ms, xs, [[400, 4, 796]] * 2, use_lens=False)
    for s in range(2):
        ref, _ = Ms.ref_whole(xs[s], None, 0, P, taps, L, centres, 30, out_stride=1200 * L)
        assert_same(got[s], ref, s)
    ms.close()
    plan.close()


# ---------------------------------------------------------------------------
# 5: seeks, beyond 2^32, and the reset
# ---------------------------------------------------------------------------
def test_a_stream_joined_beyond_two_to_the_32(gpu):
    M = gpu[0]
    rng = np.random.default_rng(32)
    L, T, K, P, r = 4, 100, 3, 4800, 117
    H = Ms.drain_of(T, L)
    taps, centres = taps_of(M, rng, T, L), centres_of(rng, K, P)
    gains = np.array([1.0, 0.25, -1.0], F32)
    n0 = P * -(-2 ** 32 // P)                               # phase index 0 there
    assert n0 > 2 ** 32 and n0 % P == 0
    xs = [Ms.random_rows(rng, False, K, 900, 0.3), Ms.random_rows(rng, False, K, 640, 0.3)]
    cuts = Ms.even_feeds([[600, 3, 17, 280], [5, 600, 35]])
    plan = make_plan(gpu, 0, P, taps, L, centres, r, gains)
    ms = M.MuxStream(plan, 2)
    first = feed_all(gpu, ms, xs, cuts)                                        # from 0
    want = [Ms.ref_whole(x, None, 0, P, taps, L, centres, r, gains=gains, out_stride=x.shape[1] * L)[0] for x in xs]
    for s in range(2):
        assert_same(first[s], want[s], ("from 0", s))
    # joined where the phase index is 0 again: the rows' outputs from 0 (the tails still hold the first run's
    # samples: the index compare excludes them)
    ms.seek([n0, n0])
    assert np.array_equal(ms.seen(), np.array([n0, n0], np.uint64))
    got = feed_all(gpu, ms, xs, cuts)
    for s in range(2):
        assert_same(got[s], want[s], ("joined at n0", s))
    seen = ms.seen()
    assert seen.dtype == np.uint64 and [int(v) for v in seen] == [n0 + 900, n0 + 640] and int(seen.min()) > 2 ** 32
    # joined one sample later: the outputs from L on of the rows with one +0.0 in front
    ms.seek([n0 + 1, n0 + 1])
    got = feed_all(gpu, ms, xs, cuts)
    for s in range(2):
        N = xs[s].shape[1]
        shifted, _ = Ms.ref_whole(np.concatenate([np.zeros((K, 1), F32), xs[s]], axis=1), None, 0, P, taps, L, centres, r,
                                  gains=gains, out_stride=(N + 1) * L)
        assert_same(got[s], shifted[L:], ("joined at n0 + 1", s))
        assert not Ms.same_bits(got[s][:40 * L], want[s][:40 * L])              # (the phase does matter)
    assert [int(v) for v in ms.seen()] == [n0 + 901, n0 + 641]
    # the restatement says the same at that index (the host model, joined there)
    hs = Ms.HostMuxStream(0, P, taps, L, centres, r, gains=gains, seen=n0 + 1)
    model = np.concatenate([hs.feed(list(xs[0][:, :600])), hs.feed(list(xs[0][:, 600:]))], axis=0)
    assert_same(model, got[0], "host model")
    # the reset: the same pieces again give the first run's outputs
    ms.seek(None)
    assert not ms.seen().any()
    again = feed_all(gpu, ms, xs, cuts)
    for s in range(2):
        assert_same(again[s], first[s], ("after the reset", s))
    with pytest.raises(ValueError):
        ms.seek([2 ** 46 + 1, 0])
    ms.seek([2 ** 46, 0])
    assert [int(v) for v in ms.seen()] == [2 ** 46, 0]
    ms.close()
    plan.close()


# ---------------------------------------------------------------------------
# 6: more streams than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_more_streams_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    ns, cut = 65537, 65535
    x = rng.standard_normal((ns, 8)).astype(F32)
    P, taps, L, centres, r = 7, np.array([0.75, -0.5, 0.25], F32), 1, np.array([3], np.int32), 1
    plan = make_plan(gpu, 0, P, taps, L, centres, r)
    d = torch.from_numpy(x).cuda()
    one, a, b = M.MuxStream(plan, ns), M.MuxStream(plan, cut), M.MuxStream(plan, ns - cut)
    res = []
    for piece in (slice(0, 4), slice(4, 8)):
        p = d[:, piece].contiguous()
        res.append((one.feed(p), a.feed(p[:cut]), b.feed(p[cut:])))
    torch.cuda.synchronize()
    assert np.all(one.seen() == 8) and np.all(a.seen() == 8) and np.all(b.seen() == 8)
    rows = []
    for w, pa, pb in res:
        wr, wn = w["rows"].cpu().numpy(), w["nsamples"].cpu().numpy()
        assert wr.shape == (ns, 4) and np.all(wn == 4)
        assert Ms.same_bits(wr, np.concatenate([pa["rows"].cpu().numpy(), pb["rows"].cpu().numpy()]))
        assert np.array_equal(wn, np.concatenate([pa["nsamples"].cpu().numpy(), pb["nsamples"].cpu().numpy()]))
        rows.append(wr)
    got = np.concatenate(rows, axis=1)
    for s in (0, 1, 65534, 65535, 65536):
        want, _cnt = Mx.ref_multiplex(x[s:s + 1], None, 0, P, taps, L, centres, r, out_stride=8)
        assert_same(got[s], want, s)
    for o in (one, a, b):
        o.close()
    plan.close()


# ---------------------------------------------------------------------------
# 7: refusals with a live object
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_what_a_feed_refuses_leaves_the_object_as_it_was(gpu, iq):
    M, torch, _ctx = gpu
    lib = _lib.load()
    rng = np.random.default_rng(3)
    L, T, P = 4, 65, 4800
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0 * L)
    plan = make_plan(gpu, 0, P, taps, L, [117, -60], 117)
    ms = M.MuxStream(plan, 2, iq=iq)
    x = Ms.random_rows(rng, iq, 4, 300, 0.3)
    d = torch.from_numpy(x).cuda()
    ms.feed(d[:, :200].contiguous())
    n = 100                                                 # the piece under test: 400 outputs
    piece = d[:, 200:].contiguous()
    need = n * L
    fr, fn, out = guarded(torch, 0, 2, need)
    before = (fr.cpu().numpy().copy(), fn.cpu().numpy().copy())
    samples, rows, nout = piece.data_ptr(), out["rows"].data_ptr(), out["nsamples"].data_ptr()

    def rc(obj=ms.handle, **kw):
        io = _lib.MuxIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
        io.d_out, io.out_stride, io.nout_cap, io.d_nout = rows, need, need, nout
        for k, v in kw.items():
            setattr(io, k, v)
        got = lib.mifsk_mux_stream_feed(obj, C.byref(io), None)
        torch.cuda.synchronize()
        assert np.array_equal(fr.cpu().numpy().view(np.uint32), before[0].view(np.uint32)), kw
        assert np.array_equal(fn.cpu().numpy(), before[1]), kw
        assert np.array_equal(ms.seen(), [200, 200]), kw
        return got

    assert lib.mifsk_mux_stream_feed(ms.handle, None, None) == EINVAL
    assert rc(obj=None) == EINVAL
    for field in ("d_samples", "d_out", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (4, 8):                                      # misaligned bases
        assert rc(d_samples=samples + off) == EINVAL and rc(d_out=rows + off) == EINVAL, off
    for stride in ((n + 1,) if iq else (n + 1, n + 2)):    # not whole 16-byte vectors (pairs lie in twos)
        assert rc(stream_stride=stride) == EINVAL, stride
    assert rc(out_stride=need + 1, nout_cap=need) == EINVAL
    assert rc(out_stride=need + 2, nout_cap=need) == EINVAL
    assert rc(nout_cap=need + 1) == EINVAL
    for nstreams in (1, 3):                                 # not the object's
        assert rc(nstreams=nstreams) == EINVAL, nstreams
    assert rc(out_stride=need - 4, nout_cap=need - 4) == EINVAL              # one vector below kmax L
    assert rc(nout_cap=need - 1) == EINVAL                  # one below it
    # the earlier refusal wins: each of these with the capacity violation behind it
    for early in ({"d_nout": None}, {"stream_stride": n + 1}, {"out_stride": need - 3}, {"nstreams": 3}):
        assert rc(**dict({"nout_cap": need - 1}, **early)) == EINVAL, early
    # what passes runs: the piece goes through and the counters move
    io = _lib.MuxIO()
    io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
    io.d_out, io.out_stride, io.nout_cap, io.d_nout = rows, need, need, nout
    assert lib.mifsk_mux_stream_feed(ms.handle, C.byref(io), None) == 0
    assert np.array_equal(ms.seen(), [300, 300])
    got, counts = read_guarded(0, 2, fr, fn, "the feed that passes")
    assert np.all(counts == need) and np.isfinite(got).all() and got.any()
    ms.close()
    plan.close()


def test_the_room_a_feed_needs(gpu):
    """the two capacity rules at their edges, kmax L and kmax L - 1: kmax is min(nsamples, stream_stride) without
    d_nsamples and stream_stride with it, whatever the lengths say; what passes runs and moves the counters"""
    M, torch, _ctx = gpu
    lib = _lib.load()
    L, T, P = 4, 65, 4800
    plan = make_plan(gpu, 0, P, M.channel_taps(T, 400.0, 48000.0, 2.0 * L), L, [117, -60], 117)
    ms = M.MuxStream(plan, 2)
    d = torch.from_numpy(Ms.random_rows(np.random.default_rng(4), False, 4, 100)).cuda()
    lens = torch.from_numpy(np.array([8, 0, 0, 0], np.int32)).cuda()
    fr, fn, out = guarded(torch, 0, 2, 400)

    def rc(nsamples, d_nsamples, out_stride, nout_cap):
        io = _lib.MuxIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = d.data_ptr(), 100, d_nsamples, nsamples, 2
        io.d_out, io.out_stride, io.nout_cap, io.d_nout = out["rows"].data_ptr(), out_stride, nout_cap, out["nsamples"].data_ptr()
        got = lib.mifsk_mux_stream_feed(ms.handle, C.byref(io), None)
        torch.cuda.synchronize()
        return got

    assert rc(100, None, 396, 396) == EINVAL and rc(100, None, 400, 399) == EINVAL
    assert rc(9999, None, 396, 396) == EINVAL               # beyond the stride: the stride counts
    assert rc(4, lens.data_ptr(), 396, 396) == EINVAL       # per-row lengths: any may be the stride
    assert rc(4, lens.data_ptr(), 400, 399) == EINVAL
    assert np.array_equal(ms.seen(), [0, 0])
    assert rc(99, None, 396, 396) == 0                      # 99 x 4 = 396
    assert np.array_equal(ms.seen(), [99, 99])
    assert np.all(out["nsamples"].cpu().numpy() == 396)
    assert rc(4, lens.data_ptr(), 400, 400) == 0
    assert np.array_equal(ms.seen(), [107, 99])
    assert np.array_equal(out["nsamples"].cpu().numpy(), [32, 0])
    rows, _n = read_guarded(0, 2, fr, fn, "the room")
    assert not np.any(rows[0][32:].view(np.uint32)) and not np.any(rows[1].view(np.uint32))
    ms.close()
    plan.close()


# ---------------------------------------------------------------------------
# 8: a side stream
# ---------------------------------------------------------------------------
def test_three_feeds_on_a_side_stream(gpu):
    """tests/test_gpu_row_streams.py's pattern: the outputs are dropped at once and memory of their size is
    refilled on the current stream before anybody waits for the side stream"""
    M, torch, _ctx = gpu
    rng = np.random.default_rng(77)
    L, T, K, P = 4, 63, 3, 4800
    taps, centres = taps_of(M, rng, T, L), centres_of(rng, K, P)
    x = torch.from_numpy(Ms.random_rows(rng, True, 2 * K, 3000, 0.3)).cuda()
    pieces = [x[:, :1000].contiguous(), x[:, 1000:1050].contiguous(), x[:, 1050:].contiguous()]
    plan = make_plan(gpu, Ms.COMPLEX, P, taps, L, centres, 0)
    ms = M.MuxStream(plan, 2, iq=True)
    want = [ms.feed(p) for p in pieces]
    want = [{k: t.cpu().numpy().tobytes() for k, t in w.items()} for w in want]
    torch.cuda.synchronize()
    ms.seek(None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = [ms.feed(p, stream=side) for p in pieces]
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
    assert np.array_equal(ms.seen(side), [3000, 3000])
    ms.close()
    plan.close()


# ---------------------------------------------------------------------------
# 9: end to end
# ---------------------------------------------------------------------------
def unequal_pieces(rng, n, count, vec):
    """about `count` unequal lengths that sum to n, whole vectors but for the last"""
    edges = np.sort(rng.choice(np.arange(1, n // vec), count - 1, replace=False)) * vec
    edges = [0] + [int(e) for e in edges] + [n]
    return [b - a for a, b in zip(edges, edges[1:])]


def test_three_signals_in_pieces_through_both_streams_and_a_resident_session(gpu):
    """MuxStream.feed -> ChannelStream.feed -> Session(resident=True).feed, ten unequal pieces, one of them empty,
    and the drain: the capture and the channel rows are the whole-row chain's, bit for bit, the bytes of every
    channel demod_batch's on that chain's rows, and they are the payloads"""
    M, torch, ctx = gpu
    c = Mx.three_bell202_rows()
    x, lens, L, T = c["x"], [int(v) for v in c["lens"]], c["L"], len(c["taps"])
    H, D, rxT = Ms.drain_of(T, L), c["rx_D"], len(c["rx_taps"][False])
    N = max(lens)
    cfg = M.rx_config(c["mode"], sample_rate=Mx.MUX_FS_IN)
    mplan = make_plan(gpu, 0, c["P"], c["taps"], L, c["centres"], c["r"], c["gains"])
    cplan = M.ChannelPlan(ctx, c["rx_taps"][False], D, c["centres"], c["r"], c["P"])
    # the whole-row chain, the capture with room for the drain's outputs (zeros behind its count)
    wbuf, _l = padded_piece(False, [x[k, :lens[k]] for k in range(3)])
    cap = M.multiplex(mplan, torch.from_numpy(wbuf).cuda(), nsamples=torch.from_numpy(c["lens"]).cuda(), nout_cap=(N + H) * L)
    assert int(cap["nsamples"][0]) == (N - 1) * L + T <= (N + H) * L
    total = torch.tensor([(N + H) * L], dtype=torch.int32, device="cuda")
    ch = M.channelize(cplan, cap["rows"], nsamples=total)
    ref = M.results_to_host(M.demod_batch(ctx, cfg, ch["rows"], nsamples=ch["nsamples"], want=("bytes",)))
    # in pieces
    ms, cs = M.MuxStream(mplan, 1), M.ChannelStream(cplan, 1)
    sess = M.Session(ctx, cfg, 3, resident=True)
    cuts = unequal_pieces(np.random.default_rng(202), N, 9, 1)
    cuts.insert(4, 0)
    cuts.append(H)                                          # the drain
    assert len(cuts) == 11 and len(set(cuts)) > 6
    xz = np.concatenate([x[:, :N], np.zeros((3, H), F32)], axis=1)
    ends = [e if e < N else N + H for e in lens]
    got, at, seen_out, capture, rows = [b"", b"", b""], 0, 0, [], []
    for i, k in enumerate(cuts):
        buf, plens = padded_piece(False, [xz[row, min(at, e):min(at + k, e)] for row, e in enumerate(ends)])
        m = ms.feed(torch.from_numpy(buf).cuda(), nsamples=torch.from_numpy(np.asarray(plens, np.int32)).cuda())
        out = cs.feed(m["rows"], nsamples=m["nsamples"])
        count = M.channel_stream_outputs(rxT, D, seen_out, k * L)          # the host's books: nothing is read back to go on
        res = sess.feed(out["rows"], final=(i == len(cuts) - 1), nsamples=[count] * 3)
        assert int(m["nsamples"][0]) == k * L and np.all(out["nsamples"].cpu().numpy() == count)
        capture.append(m["rows"].cpu().numpy()[0, :k * L])
        rows.append(out["rows"].cpu().numpy()[:, :count])
        for chn in range(3):
            got[chn] += res[chn]["bytes"]
        at += k
        seen_out += k * L
    sess.close()
    cs.close()
    ms.close()
    assert_same(np.concatenate(capture), cap["rows"].cpu().numpy()[0, :(N + H) * L], "capture")
    n = int(ch["nsamples"][0])
    assert_same(np.concatenate(rows, axis=1), ch["rows"].cpu().numpy()[:, :n], "channel rows")
    cplan.close()
    mplan.close()
    for chn, payload in enumerate(c["payloads"]):
        assert got[chn] == ref["bytes"][chn, :int(ref["nbytes"][chn])].tobytes(), chn
        assert Ch.payload_condition(got[chn], payload), (chn, got[chn], payload)


def test_fm_modulate_in_pieces_into_an_iq_stream(gpu):
    """fm_modulate in pieces with phase0 / phase_out -> MuxStream(iq=True).feed equals
    multiplex(fm_modulate(whole), iq=True) on [0, N L), bit for bit"""
    M, torch, ctx = gpu
    words = Iq.fm_messages()
    tx_cfg = M.rx_config("1200", sample_rate=Mq.FS_IN)
    lead = torch.from_numpy(np.array(Mq.TX_LEAD, np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, tx_cfg, torch.from_numpy(words).cuda(), amplitude=1.0, leading_silence=lead)
    n, L = clean.shape[1], Mq.L_FM
    dev = M.fm_step(Iq.DEVIATION_HZ, Mq.FS_IN)
    taps = Mq.fm_tx_taps(M)
    plan = M.MuxPlan(ctx, taps, L, Iq.CENTRES, 0, Iq.P_FM, complex_output=True)
    iq = M.fm_modulate(ctx, clean, nsamples=lens, deviation=dev, centre=0.0, amplitude=Iq.CARRIER)
    whole = M.multiplex(plan, iq, iq=True)                  # every row the full width: zeros behind a message
    ms = M.MuxStream(plan, 1, iq=True)
    phase = torch.zeros(3, dtype=torch.int64, device="cuda")
    hl = lens.cpu().numpy().astype(np.int64)
    cuts = unequal_pieces(np.random.default_rng(355), n, 9, 4) + [0]
    got, at = [], 0
    for k in cuts:
        width = max(4, (k + 3) // 4 * 4)
        piece = torch.zeros((3, width), dtype=torch.float32, device="cuda")
        piece[:, :k] = clean[:, at:at + k]
        plens = torch.from_numpy(np.clip(hl - at, 0, k).astype(np.int32)).cuda()
        part = M.fm_modulate(ctx, piece, nsamples=plens, deviation=dev, centre=0.0, amplitude=Iq.CARRIER,
                             phase0=phase, phase_out=phase)
        out = ms.feed(part, nsamples=torch.full((3,), k, dtype=torch.int32, device="cuda"))
        assert int(out["nsamples"][0]) == k * L
        got.append(out["rows"].cpu().numpy()[0, :k * L])
        at += k
    assert np.array_equal(ms.seen(), [n])
    ms.close()
    got = np.concatenate(got, axis=0)
    assert got.shape == (n * L, 2) and n * L > 10000
    assert_same(got, whole["rows"].cpu().numpy()[0, :n * L], "capture")
    plan.close()
