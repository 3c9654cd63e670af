"""mifsk_multiplex_batch (include/mifsk.h, minimodem_amd/csrc/mifsk_mux.hip) against the host
restatement tools/mux_ref.c: every output element and every count of every case bit for bit, no
tolerance (a NaN equals a NaN).  Rows are a few thousand outputs (one case just over 2^20, one of 65 537 streams of 8 samples); both
output arrays are made with guard cells around them, which every call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _mux as Mx
import _oracle as O
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
F32_GUARD, S16_GUARD, NOUT_GUARD = F32(7.25), 12345, -77
EINVAL = -22
CHUNK = 256 * 8                     # outputs of one workgroup of the kernel


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
    return M.MuxPlan(ctx, taps, L, centres, r, P, complex_output=bool(kind & Mx.COMPLEX), s16=bool(kind & Mx.S16),
                     gains=gains)


def default_stride(kind, width, L, T):
    v = Mx.vec_of(kind)
    return max(v, (Mx.full_outputs(width, L, T) + v - 1) // v * v)


def multiplex(gpu, plan, x, lens=None, nout_cap=None, out_stride=None, stream=None):
    """One call with guard cells around both outputs -> (rows [nstreams, out_stride(, 2)], nout) as numpy."""
    M, torch, _ctx = gpu
    d = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nrows, width = d.shape
    ns = nrows // plan.nchannels
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32).reshape(-1)).cuda()
    kind = (Mx.COMPLEX if plan.complex_output else 0) | (Mx.S16 if plan.s16 else 0)
    if out_stride is None:
        out_stride = default_stride(kind, width, plan.interp, plan.ntaps) if nout_cap is None else \
            max(Mx.vec_of(kind), (nout_cap + Mx.vec_of(kind) - 1) // Mx.vec_of(kind) * Mx.vec_of(kind))
    per = 2 if plan.complex_output else 1
    g = GUARD * 8                                   # scalars: the base stays 16-byte aligned
    guard = S16_GUARD if plan.s16 else float(F32_GUARD)
    fr = torch.full((ns * out_stride * per + 2 * g,), guard, dtype=torch.int16 if plan.s16 else torch.float32,
                    device=d.device)
    fn = torch.full((ns + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device=d.device)
    shape = (ns, out_stride, 2) if plan.complex_output else (ns, out_stride)
    out = {"rows": fr[g:g + ns * out_stride * per].view(shape), "nsamples": fn[GUARD:GUARD + ns]}
    torch.cuda.synchronize()                        # the fills, before a launch on another stream
    res = M.multiplex(plan, d, nsamples=dl, nout_cap=nout_cap, stream=stream, out=out)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert res is out
    fr, fn = fr.cpu().numpy(), fn.cpu().numpy()
    for cells in (fr[:g], fr[-g:]):
        assert np.all(cells == fr.dtype.type(guard)), "the guard cells around the rows were written"
    for cells in (fn[:GUARD], fn[-GUARD:]):
        assert np.all(cells == NOUT_GUARD), "the guard cells around the counts were written"
    return fr[g:-g].reshape(shape), fn[GUARD:-GUARD]


def expect(x, kind, P, taps, L, centres, r, gains, lens, nout_cap, out_stride):
    """what the call must leave: the restatement's rows and counts, stream by stream"""
    K = len(centres)
    x = np.asarray(x)
    ns = x.shape[0] // K
    lens = None if lens is None else np.asarray(lens).reshape(ns, K)
    rows, nout = [], []
    for s in range(ns):
        row, cnt = Mx.ref_multiplex(x[s * K:(s + 1) * K], None if lens is None else lens[s], kind, P, taps, L,
                                    centres, r, gains, out_stride, nout_cap)
        rows.append(row)
        nout.append(cnt)
    return np.stack(rows), np.array(nout, np.int32)


def assert_same(rows, want_rows, nout, want_nout):
    assert np.array_equal(nout, want_nout), (nout, want_nout)
    if not Mx.same_bits(rows, want_rows):
        assert rows.shape == want_rows.shape and rows.dtype == want_rows.dtype
        diff = rows != want_rows
        if rows.dtype != np.int16:
            diff = (rows.view(np.uint32) != want_rows.view(np.uint32)) & ~(np.isnan(rows) & np.isnan(want_rows))
        bad = np.argwhere(diff)
        raise AssertionError("%d elements differ, first at %s: %r != %r" % (
            len(bad), bad[0], rows[tuple(bad[0])], want_rows[tuple(bad[0])]))


def check(gpu, x, kind, P, taps, L, centres, r, gains=None, lens=None, nout_cap=None, out_stride=None, plan=None):
    own = plan is None
    plan = plan or make_plan(gpu, kind, P, taps, L, centres, r, gains)
    rows, nout = multiplex(gpu, plan, x, lens, nout_cap, out_stride)
    if own:
        plan.close()
    want_rows, want_nout = expect(x, kind, P, taps, L, centres, r, gains, lens, nout_cap, rows.shape[1])
    assert_same(rows, want_rows, nout, want_nout)
    return rows, nout


def centres_of(rng, K, P):
    fixed = [q for q in (0, -1, P // 2, -(P - 1), 1, -(P // 2)) if abs(q) < P] or [0]
    more = rng.integers(-(P - 1), P, max(0, K - len(fixed))) if P > 1 else np.zeros(max(0, K - len(fixed)), int)
    return np.array((fixed + [int(v) for v in more])[:K] + [0] * max(0, K - len(fixed) - len(more)), np.int32)


def taps_of(M, rng, T, L):
    return M.channel_taps(T, 1200.0, 192000.0, 2.0 * L) if T > 2 else rng.standard_normal(T).astype(F32)


# ---------------------------------------------------------------------------
# kinds and sizes
# ---------------------------------------------------------------------------
def size_cases():
    """_mux.size_cases() (whose coverage tests/test_mux_args.py asserts) as pytest parameters"""
    return [pytest.param(*c, id="%s-L%d-T%d-K%d-P%d" % c) for c in Mx.size_cases()]


@pytest.mark.parametrize("name,L,T,K,P", size_cases())
def test_kinds_and_sizes(gpu, name, L, T, K, P):
    """Two streams of more than two workgroups' outputs each; the second one ragged, its longest row not
    channel 0 and, from three channels on, a row of length zero in it.  q - r is negative for some
    channels of every case with P > 1; every other case has gains."""
    M = gpu[0]
    kind = Mx.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + L)
    n = max(12, -(-(2 * CHUNK + 400) // L) + 3)
    stride = (n + 3) // 4 * 4
    assert Mx.full_outputs(n, L, T) > 2 * CHUNK
    taps = taps_of(M, rng, T, L)
    centres = centres_of(rng, K, P)
    gains = (rng.standard_normal(K) + 1.5).astype(F32) if (L + K) % 2 else None
    scale = 0.05 if kind & Mx.S16 else 1.0
    x = (rng.standard_normal((2 * K, stride)) * scale).astype(F32)
    lens = np.full((2, K), n, np.int32)
    lens[1] = rng.integers(1, n, K)
    lens[1, K - 1] = n - 1                      # the longest of stream 1 (K > 1: not channel 0)
    if K >= 3:
        lens[1, 1] = 0
    for r in sorted({0, int(centres[-1]), int(centres[K // 2])})[:2] if P > 1 else (0,):
        check(gpu, x, kind, P, taps, L, centres, r, gains, lens=lens)


@pytest.mark.parametrize("name,L,T,K", [("complex-f32", 2, 9, 64), ("real-s16", 1, 2000, 5), ("real-f32", 1, 4096, 2)],
                         ids=["5-channels-at-a-time", "1-at-a-time-68KB", "1-at-a-time-119KB"])
def test_channels_staged_in_several_batches(gpu, name, L, T, K):
    """Small L makes a workgroup's span of samples long (2048 / L + T / L per channel): the channels are
    staged 5 at a time with a last batch of 4, and one at a time with more than 64 KiB of LDS (the
    largest the entry can ask for: L = 1, T = 4096)."""
    M = gpu[0]
    kind = Mx.KINDS[name]
    rng = np.random.default_rng(T + K)
    n = (2 * CHUNK + 400) // L + 4
    n = (n + 3) // 4 * 4
    taps = taps_of(M, rng, T, max(L, 4))
    centres = centres_of(rng, K, 4800)
    x = (rng.standard_normal((2 * K, n)) * (0.05 if kind & Mx.S16 else 1.0)).astype(F32)
    lens = np.full((2, K), n, np.int32)
    lens[1] = rng.integers(0, n, K)
    check(gpu, x, kind, 4800, taps, L, centres, int(centres[-1]), lens=lens)


def test_a_row_of_just_over_2_to_the_20_outputs_with_2_to_the_20_phase_steps(gpu):
    """n mod P wraps inside the row and dq * (n mod P) needs 40 bits"""
    M = gpu[0]
    rng = np.random.default_rng(20)
    P, L, T, K = 1 << 20, 64, 65, 2
    n = P // L + 2
    assert Mx.full_outputs(n, L, T) > P
    x = rng.standard_normal((K, (n + 3) // 4 * 4)).astype(F32)
    centres = np.array([P - 1, -(P - 3)], np.int32)
    check(gpu, x, 0, P, taps_of(M, rng, T, L), L, centres, -5, lens=[n, n - 77])


# ---------------------------------------------------------------------------
# ragged batches, capacity, alignment, special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Mx.KINDS))
def test_ragged_batches_and_capacity(gpu, name):
    M = gpu[0]
    kind = Mx.KINDS[name]
    rng = np.random.default_rng(7)
    L, T, P, n = 4, 65, 4800, 700
    taps = taps_of(M, rng, T, L)
    centres = np.array([117, -60, 2400], np.int32)
    gains = np.array([1.0, 0.5, -2.0], F32)
    lens = np.array([[0, 10, n], [n + 1000, 0, 17], [0, 0, 0], [1, 0, 0], [n, n, n]], np.int32)
    x = (rng.standard_normal((lens.size, n)) * (0.05 if kind & Mx.S16 else 1.0)).astype(F32)
    full = Mx.full_outputs(n, L, T)
    assert full > CHUNK + 200
    plan = make_plan(gpu, kind, P, taps, L, centres, 170, gains)
    for nout_cap in (None, CHUNK + 123, 0, T - 5, 1, full + 9):        # inside a chunk, nothing, below T, beyond
        rows, nout = check(gpu, x, kind, P, taps, L, centres, 170, gains, lens=lens, nout_cap=nout_cap, plan=plan)
        cap = rows.shape[1] if nout_cap is None else nout_cap
        assert list(nout) == [min(cap, c) for c in (full, full, 0, T, full)]
        for s, c in enumerate(nout):
            assert not np.any(rows[s, c:].view(np.uint32 if rows.dtype == F32 else np.uint16)), "tail of row %d" % s
    plan.close()


@pytest.mark.parametrize("name", ["real-f32", "complex-s16"])
def test_input_rows_at_every_alignment_the_stride_rule_allows(gpu, name):
    M, torch, _ctx = gpu
    kind = Mx.KINDS[name]
    rng = np.random.default_rng(5)
    L, T, P, K = 3, 10, 4799, 2
    taps = taps_of(M, rng, T, L)
    centres = np.array([5, -700], np.int32)
    n, stride = 37 * 4 - 1, 37 * 4                            # 37 vectors: the rows walk through every alignment
    pool = torch.from_numpy((rng.standard_normal(8 * 4 + 4 * stride) * 0.05).astype(F32)).cuda()
    plan = make_plan(gpu, kind, P, taps, L, centres, 5)
    for j in range(8):                                        # the base at each 16-byte step of a 128-byte line
        x = pool[j * 4:j * 4 + 4 * stride].view(4, stride)[:, :n]
        assert x.data_ptr() % 16 == 0 and x.data_ptr() % 128 == (pool.data_ptr() + 16 * j) % 128
        rows, nout = multiplex(gpu, plan, x)
        want, wn = expect(x.cpu().numpy(), kind, P, taps, L, centres, 5, None, None, None, rows.shape[1])
        assert_same(rows, want, nout, wn)
    plan.close()


@pytest.mark.parametrize("cx", [False, True])
def test_special_values(gpu, cx):
    M = gpu[0]
    kind = Mx.COMPLEX if cx else 0
    rng = np.random.default_rng(9)
    L, T, P, n, K = 3, 20, 65536, 900, 2
    taps = taps_of(M, rng, T, L)
    centres = np.array([1000, -20000], np.int32)
    x = rng.standard_normal((5 * K, n)).astype(F32)
    x[0, 100:400], x[1, 100:400] = 0.0, -0.0                  # windows of zeros of both signs
    x[2] = (rng.integers(1, 1 << 22, n).astype(np.uint32)).view(F32)        # subnormals
    x[3] *= F32(1e30)
    x[4, 333], x[5, 700] = np.inf, -np.inf
    x[6, 444] = np.nan
    x[8:10] *= 0.01
    rows, _nout = check(gpu, x, kind, P, taps, L, centres, 1000)
    flat = rows.reshape(5, rows.shape[1], -1)
    assert np.isnan(flat[3]).any() and not np.isnan(flat[3]).all()          # the NaN stays inside its tail
    assert (np.isinf(flat[2]) | np.isnan(flat[2])).any() and np.isfinite(flat[2]).any()
    assert not np.any(flat[0, 110 * L:390 * L].view(np.uint32) & 0x7FFFFFFF)      # zeros in, zeros out
    # a NaN gain poisons every output its channel reaches, an infinite one the non-zero ones
    rows, nout = check(gpu, x[8:10], kind, P, taps, L, centres, 1000, gains=np.array([1.0, np.nan], F32),
                       lens=[n, n // 2])
    # (behind the short row too: its re = 0.0 there, and 0.0 * NaN is a NaN)
    assert nout[0] == Mx.full_outputs(n, L, T) and np.isnan(rows.reshape(rows.shape[1], -1)[:nout[0]]).all()
    check(gpu, x[8:10], kind, P, taps, L, centres, 1000, gains=np.array([-np.inf, 0.0], F32))
    # taps that are not finite: a term outside the row is skipped, not multiplied by zero.  Outputs 0
    # and 2 have one term inside the row (taps 0 and 2); taps 3 and 11 would meet samples -1 and -3.
    bad = taps.copy()
    bad[3], bad[11] = np.nan, np.inf
    rows, _ = check(gpu, x[8:10], kind, P, bad, L, centres, 1000)
    flat = rows.reshape(rows.shape[1], -1)
    assert np.isfinite(flat[0]).all() and np.isfinite(flat[2]).all() and not np.isfinite(flat[3 * L]).any()


def lrintf_ties():
    """float32 values whose float32 product with 32767.0f is an integer plus one half"""
    k = np.arange(-300, 300, dtype=np.float64)
    v = ((k + 0.5) / 32767.0).astype(F32)
    t = v * F32(32767.0)
    return v[t.astype(np.float64) == k + 0.5]


@pytest.mark.parametrize("cx", [False, True])
def test_pcm16_clamps_ties_and_nan(gpu, cx):
    """One tap of 1.0, L = 1, one channel, P = 1: o is the finite sample itself (oi is 0.0)"""
    kind = Mx.S16 | (Mx.COMPLEX if cx else 0)
    ties = lrintf_ties()
    assert ties.size >= 8 and {int(np.floor(v * 32767.0)) & 1 for v in ties.astype(np.float64)} == {0, 1}
    vals = np.concatenate([ties, F32([0.5, -0.5, 1.0, -1.0, 1.00002, -1.00002, -1.00004, 2.0, -2.0, 1e30, -1e30,
                                      np.nan, 0.0, -0.0, 3e-5, -3e-5])]).astype(F32)
    x = np.zeros((1, (vals.size + 3) // 4 * 4), F32)
    x[0, :vals.size] = vals
    rows, nout = check(gpu, x, kind, 1, np.ones(1, F32), 1, [0], 0, lens=[vals.size])
    got = rows.reshape(rows.shape[1], -1)[:vals.size, 0]
    assert nout[0] == vals.size and np.array_equal(got, Mx.numpy_s16(vals))
    assert got.max() == 32767 and got.min() == -32768 and got[list(vals).index(F32(0.5))] == 16384


@pytest.mark.parametrize("cx", [False, True])
def test_pcm16_rows_are_the_float_rows_through_the_conversion(gpu, cx):
    M = gpu[0]
    rng = np.random.default_rng(16)
    L, T, P, K, n = 40, 401, 4800, 5, 80
    taps = taps_of(M, rng, T, L)
    centres = centres_of(rng, K, P)
    x = (rng.standard_normal((2 * K, n)) * 1.5).astype(F32)            # the sum clamps now and then
    x[3, 40] = np.nan
    base = Mx.COMPLEX if cx else 0
    stride = (Mx.full_outputs(n, L, T) + 7) // 8 * 8           # a whole number of vectors of either kind
    f, nf = check(gpu, x, base, P, taps, L, centres, 170, out_stride=stride)
    s, ns = check(gpu, x, base | Mx.S16, P, taps, L, centres, 170, out_stride=stride)
    assert np.array_equal(nf, ns)
    assert np.array_equal(s, Mx.numpy_s16(f))
    assert (s == 32767).any() and (s == -32768).any()


# ---------------------------------------------------------------------------
# reuse, plans, streams, refusals
# ---------------------------------------------------------------------------
def test_reuse_of_a_plan_and_of_its_outputs_and_two_plans_at_once(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(21)
    P, n = 4800, 600
    ta, tb = taps_of(M, rng, 65, 4), taps_of(M, rng, 401, 40)
    ca, cb = np.array([117, 237, -57], np.int32), centres_of(rng, 5, P)
    x1, x2 = rng.standard_normal((6, n)).astype(F32), rng.standard_normal((6, n)).astype(F32)
    xb = rng.standard_normal((5, 60)).astype(F32)
    pa = make_plan(gpu, 0, P, ta, 4, ca, 170)
    alone1 = multiplex(gpu, pa, x1)
    pb = make_plan(gpu, Mx.COMPLEX, P, tb, 40, cb, 170)         # two plans alive at once
    both_b = multiplex(gpu, pb, xb)
    both_a2 = multiplex(gpu, pa, x2)                            # a second call on the same plan, other rows
    both_a1 = multiplex(gpu, pa, x1)
    pa.close()
    alone_b = multiplex(gpu, pb, xb)
    pb.close()
    assert Mx.same_bits(alone1[0], both_a1[0]) and Mx.same_bits(both_b[0], alone_b[0])
    for got, x, kind, taps, L, c in ((alone1, x1, 0, ta, 4, ca), (both_a2, x2, 0, ta, 4, ca),
                                     (both_b, xb, Mx.COMPLEX, tb, 40, cb)):
        want, wn = expect(x, kind, P, taps, L, c, 170, None, None, None, got[0].shape[1])
        assert_same(got[0], want, got[1], wn)
    # out= reuse on a stream of its own: the same as fresh calls, shorter rows leave no old outputs behind
    pa = make_plan(gpu, 0, P, ta, 4, ca, 170)
    side = torch.cuda.Stream()
    d1, d2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    short = torch.from_numpy(np.array([n, 150, 70, 0, 0, 3], np.int32)).cuda()
    torch.cuda.synchronize()
    out = M.multiplex(pa, d1, stream=side)
    side.synchronize()
    assert out["rows"].dtype == torch.float32 and out["rows"].shape == (2, default_stride(0, n, 4, 65))
    assert out["nsamples"].dtype == torch.int32 and out["nsamples"].shape == (2,)
    first = out["rows"].cpu().numpy().copy()
    again = M.multiplex(pa, d2, nsamples=short, stream=side, out=out)
    side.synchronize()
    assert again is out and Mx.same_bits(first, alone1[0])
    want, wn = expect(x2, 0, P, ta, 4, ca, 170, None, [n, 150, 70, 0, 0, 3], None, first.shape[1])
    assert_same(out["rows"].cpu().numpy(), want, out["nsamples"].cpu().numpy(), wn)
    # and through the guarded helper on the side stream
    rows, nout = multiplex(gpu, pa, d2, lens=[n, 150, 70, 0, 0, 3], stream=side)
    assert_same(rows, want, nout, wn)
    pa.close()
    # the shapes and types of the other kinds
    pc = make_plan(gpu, Mx.COMPLEX | Mx.S16, P, ta, 4, ca, 170)
    out = M.multiplex(pc, d1[:3])
    torch.cuda.synchronize()
    assert out["rows"].dtype == torch.int16 and out["rows"].shape == (1, default_stride(3, n, 4, 65), 2)
    pc.close()


@pytest.mark.parametrize("name", list(Mx.KINDS))
def test_what_multiplex_refuses_of_the_io(gpu, name):
    """with a plan of each kind: every refusal comes back before a launch (the pointers are numbers)"""
    M, _torch, _ctx = gpu
    lib = _lib.load()
    kind = Mx.KINDS[name]
    vec = Mx.vec_of(kind)
    plan = make_plan(gpu, kind, 4800, M.channel_taps(65, 1200.0, 192000.0, 8.0), 4, [117, -60], 170)
    base = 1 << 20

    def rc(**kw):
        io = _lib.MuxIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = base, 4000, None, 4000, 2
        io.d_out, io.out_stride, io.nout_cap, io.d_nout = base + (1 << 24), 16000, 16000, base + (1 << 26)
        for k, v in kw.items():
            setattr(io, k, v)
        return lib.mifsk_multiplex_batch(plan.handle, C.byref(io), None)

    assert lib.mifsk_multiplex_batch(plan.handle, None, None) == EINVAL
    for field in ("d_samples", "d_out", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (4, 8, 12):
        assert rc(d_samples=base + off) == EINVAL, off
    for stride in (4001, 4002, 4003):
        assert rc(stream_stride=stride) == EINVAL, stride
    for off in (2, 4, 8):
        assert rc(d_out=base + (1 << 24) + off) == EINVAL, off
    assert rc(out_stride=0, nout_cap=0) == EINVAL
    for out_stride in range(16000 + 1, 16000 + vec):            # not a whole number of 16-byte vectors
        assert rc(out_stride=out_stride) == EINVAL, out_stride
    assert rc(out_stride=(1 << 32) - 8 + vec, nout_cap=0) == EINVAL and rc(out_stride=1 << 40, nout_cap=0) == EINVAL
    assert rc(nout_cap=16001) == EINVAL and rc(nout_cap=0xFFFFFFFF) == EINVAL
    assert rc(nstreams=(1 << 30) + 1) == EINVAL                 # nstreams * nchannels
    assert rc(stream_stride=4001, d_out=None) == EINVAL
    plan.close()


# ---------------------------------------------------------------------------
# end to end: synthesize_batch -> multiplex -> channelize -> demod_batch on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [True, False], ids=["complex", "real"])
def test_the_four_step_chain_on_the_device(gpu, cx):
    M, torch, ctx = gpu
    c = Mx.three_bell202_rows()
    kind = Mx.COMPLEX if cx else 0
    cfg = M.rx_config(c["mode"], sample_rate=Mx.MUX_FS_IN)
    words = torch.from_numpy(np.stack([np.frombuffer(p, np.uint8) for p in c["payloads"]])).cuda()
    lead = torch.from_numpy(np.array([16, 75, 37], np.int32)).cuda()
    tx, txlen = M.synthesize_batch(ctx, cfg, words, amplitude=0.3, leading_silence=lead, stride=c["x"].shape[1])
    mplan = make_plan(gpu, kind, c["P"], c["taps"], c["L"], c["centres"], c["r"], c["gains"])
    cap = M.multiplex(mplan, tx, nsamples=txlen)
    cplan = M.ChannelPlan(ctx, c["rx_taps"][cx], c["rx_D"], c["centres"], c["r"], c["P"], complex_input=cx)
    ch = M.channelize(cplan, cap["rows"], nsamples=cap["nsamples"])
    out = M.demod_batch(ctx, cfg, ch["rows"], nsamples=ch["nsamples"], want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    mplan.close()
    cplan.close()
    # the inputs are the ones the CPU test proved
    assert np.array_equal(tx.cpu().numpy(), c["x"]) and np.array_equal(txlen.cpu().numpy(), c["lens"])
    want, wn = expect(c["x"], kind, c["P"], c["taps"], c["L"], c["centres"], c["r"], c["gains"], c["lens"], None,
                      cap["rows"].shape[1])
    assert_same(cap["rows"].cpu().numpy(), want, cap["nsamples"].cpu().numpy(), wn)
    assert cap["rows"].shape[1] <= 40000
    rows, lens = ch["rows"].cpu().numpy(), ch["nsamples"].cpu().numpy()
    wrows = Ch.ref_channelize(want[0], Ch.COMPLEX if cx else 0, c["P"], c["rx_taps"][cx], c["rx_D"], c["centres"],
                              c["r"], n=int(wn[0]))
    assert np.all(lens == wrows.shape[1]) and Ch.same_f32(rows[:, :wrows.shape[1]], wrows)
    res = M.results_to_host(out)
    ocfg = O.oracle_config(c["mode"], sample_rate=Mx.MUX_FS_IN)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, rows, lens, res, threads=3)
    assert bad == []                                           # frames, bytes and episodes of the device-made rows
    for k, payload in enumerate(c["payloads"]):
        decoded = res["bytes"][k, :int(res["nbytes"][k])].tobytes()
        assert Ch.payload_condition(decoded, payload), (k, decoded, payload)


# ---------------------------------------------------------------------------
# more streams than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_a_batch_of_more_streams_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    ns, n, cut = 65537, 8, 40000
    x = rng.standard_normal((ns, n)).astype(F32)
    P, taps, L, centres, r = 7, np.array([0.75, -0.5, 0.25], F32), 2, np.array([3], np.int32), 1
    full = Mx.full_outputs(n, L, taps.size)
    plan = make_plan(gpu, 0, P, taps, L, centres, r)
    d = torch.from_numpy(x).cuda()
    whole = M.multiplex(plan, d)
    parts = [M.multiplex(plan, d[:cut]), M.multiplex(plan, d[cut:])]
    torch.cuda.synchronize()
    plan.close()
    rows, nout = whole["rows"].cpu().numpy(), whole["nsamples"].cpu().numpy()
    assert rows.shape == (ns, default_stride(0, n, L, taps.size)) and np.all(nout == full)
    assert Mx.same_bits(rows, np.concatenate([p["rows"].cpu().numpy() for p in parts]))
    assert np.array_equal(nout, np.concatenate([p["nsamples"].cpu().numpy() for p in parts]))
    for s in (0, 65534, 65535, 65536):
        want, cnt = Mx.ref_multiplex(x[s:s + 1], None, 0, P, taps, L, centres, r)
        assert cnt == full and Mx.same_bits(rows[s], want), s
