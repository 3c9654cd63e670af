"""mifsk_multiplex_iq_batch (include/mifsk/mux_iq.h, minimodem_amd/csrc/mifsk_mux.hip) against the host
restatement mux_ref_iq (tools/mux_ref.c): every output element, every tail and every count of every case bit
for bit, no tolerance (a NaN equals a NaN).  Rows are a few thousand outputs (one case of 65 537 streams of 8
elements); both output arrays are made with guard cells around them, which every call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import _channel_iq as Iq
import _mux as Mx
import _mux_iq as Mq
import _oracle as O
from _abi import EINVAL, ladder
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
F32_GUARD, S16_GUARD, NOUT_GUARD = F32(7.25), 12345, -77
CHUNK = 256 * 8                     # outputs of one workgroup of the kernel


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def kind_of(plan):
    return (Mq.COMPLEX if plan.complex_output else 0) | (Mq.S16 if plan.s16 else 0)


def make_plan(gpu, kind, P, taps, L, centres, r, gains=None):
    M, _torch, ctx = gpu
    return M.MuxPlan(ctx, taps, L, centres, r, P, complex_output=bool(kind & Mq.COMPLEX), s16=bool(kind & Mq.S16),
                     gains=gains)


def default_stride(kind, width, L, T):
    v = Mq.vec_of(kind)
    return max(v, (Mq.full_outputs(width, L, T) + v - 1) // v * v)


def guarded(torch, plan, ns, out_stride, device):
    """both outputs with guard cells around them -> (the rows' buffer, the counts' buffer, out=, guard value)"""
    per = 2 if plan.complex_output else 1
    g = GUARD * 8                                   # scalars: the base stays 16-byte aligned
    guard = S16_GUARD if plan.s16 else float(F32_GUARD)
    fr = torch.full((ns * out_stride * per + 2 * g,), guard, dtype=torch.int16 if plan.s16 else torch.float32,
                    device=device)
    fn = torch.full((ns + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device=device)
    shape = (ns, out_stride, 2) if plan.complex_output else (ns, out_stride)
    out = {"rows": fr[g:g + ns * out_stride * per].view(shape), "nsamples": fn[GUARD:GUARD + ns]}
    return fr, fn, out, guard


def multiplex(gpu, plan, x, lens=None, nout_cap=None, out_stride=None, stream=None, iq=True):
    """One call with guard cells around both outputs -> (rows [nstreams, out_stride(, 2)], nout) as numpy."""
    M, torch, _ctx = gpu
    d = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    nrows, width = d.shape[0], d.shape[1]
    ns = nrows // plan.nchannels
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32).reshape(-1)).cuda()
    kind = kind_of(plan)
    if out_stride is None:
        v = Mq.vec_of(kind)
        out_stride = default_stride(kind, width, plan.interp, plan.ntaps) if nout_cap is None else \
            max(v, (nout_cap + v - 1) // v * v)
    fr, fn, out, guard = guarded(torch, plan, ns, out_stride, d.device)
    g = GUARD * 8
    torch.cuda.synchronize()                        # the fills, before a launch on another stream
    res = M.multiplex(plan, d, nsamples=dl, nout_cap=nout_cap, stream=stream, out=out, iq=iq)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert res is out
    shape = tuple(out["rows"].shape)
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
        row, cnt = Mq.ref_multiplex_iq(x[s * K:(s + 1) * K], None if lens is None else lens[s], kind, P, taps, L,
                                       centres, r, gains, out_stride, nout_cap)
        rows.append(row)
        nout.append(cnt)
    return np.stack(rows), np.array(nout, np.int32)


def assert_same(rows, want_rows, nout, want_nout):
    assert np.array_equal(nout, want_nout), (nout, want_nout)
    if not Mq.same_bits(rows, want_rows):
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
    return M.channel_taps(T, 1200.0, 192000.0, float(L)) if T > 2 else rng.standard_normal(T).astype(F32)


# ---------------------------------------------------------------------------
# kinds and sizes
# ---------------------------------------------------------------------------
def size_cases():
    """_mux.size_cases() (whose coverage tests/test_mux_args.py asserts) as pytest parameters"""
    return [pytest.param(*c, id="%s-L%d-T%d-K%d-P%d" % c) for c in Mq.size_cases()]


@pytest.mark.parametrize("name,L,T,K,P", size_cases())
def test_kinds_and_sizes(gpu, name, L, T, K, P):
    """Two streams of more than two workgroups' outputs each; the second one ragged, its longest row not
    channel 0 and, from three channels on, a row of length zero in it.  Centres 0, +-(P - 1) and P / 2 and
    random ones; every other case has gains."""
    M = gpu[0]
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + L)
    n = max(12, -(-(2 * CHUNK + 400) // L) + 3)
    stride = (n + 1) // 2 * 2
    assert Mq.full_outputs(n, L, T) > 2 * CHUNK
    taps = taps_of(M, rng, T, L)
    centres = centres_of(rng, K, P)
    gains = (rng.standard_normal(K) + 1.5).astype(F32) if (L + K) % 2 else None
    x = Mq.iq_rows(rng, 2 * K, stride, 0.05 if kind & Mq.S16 else 1.0)
    lens = np.full((2, K), n, np.int32)
    lens[1] = rng.integers(1, n, K)
    lens[1, K - 1] = n - 1                      # the longest of stream 1 (K > 1: not channel 0)
    if K >= 3:
        lens[1, 1] = 0
    for r in sorted({0, int(centres[-1]), int(centres[K // 2])})[:2] if P > 1 else (0,):
        check(gpu, x, kind, P, taps, L, centres, r, gains, lens=lens)


@pytest.mark.parametrize("name", list(Mq.KINDS))
def test_ragged_streams_and_capacity(gpu, name):
    """row lengths 0, 1, ceil(T / L) - 1, one that ends inside a workgroup's span and one above the stride; a
    stream of empty rows; nout_cap nothing, below T, inside a workgroup and above the row"""
    M = gpu[0]
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(7)
    L, T, P, n = 4, 65, 4800, 700
    J = -(-T // L)
    taps = taps_of(M, rng, T, L)
    centres = np.array([117, -60, 2400], np.int32)
    gains = np.array([1.0, 0.5, -2.0], F32)
    inside = CHUNK // L + 37                    # its last sample lies in the second workgroup's span
    lens = np.array([[0, 10, n], [n + 1000, 0, J - 1], [0, 0, 0], [1, 0, 0], [inside, J - 1, 1], [n, n, n]], np.int32)
    x = Mq.iq_rows(rng, lens.size, n, 0.05 if kind & Mq.S16 else 1.0)
    full = Mq.full_outputs(n, L, T)
    assert full > CHUNK + 200 and CHUNK < Mq.full_outputs(inside, L, T) < 2 * CHUNK
    plan = make_plan(gpu, kind, P, taps, L, centres, 170, gains)
    for nout_cap in (None, CHUNK + 123, 0, T - 5, 1, full + 9):        # inside a chunk, nothing, below T, beyond
        rows, nout = check(gpu, x, kind, P, taps, L, centres, 170, gains, lens=lens, nout_cap=nout_cap, plan=plan)
        cap = rows.shape[1] if nout_cap is None else nout_cap
        assert list(nout) == [min(cap, c) for c in (full, full, 0, T, Mq.full_outputs(inside, L, T), full)]
        for s, c in enumerate(nout):
            assert not np.any(rows[s, c:].view(np.uint32 if rows.dtype == F32 else np.uint16)), "tail of row %d" % s
    plan.close()


# ---------------------------------------------------------------------------
# the shapes of the LDS staging
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,T,K", [("complex-f32", 2, 9, 64), ("real-s16", 1, 2000, 5), ("real-f32", 1, 4096, 2),
                                        ("complex-s16", 300, 7, 3), ("real-f32", 300, 901, 2)],
                         ids=["5-channels-at-a-time", "1-at-a-time-68KB", "1-at-a-time-119KB", "L-above-T",
                              "a-group-over-several-workgroups"])
def test_the_shapes_of_the_staging(gpu, name, L, T, K):
    """Small L makes a workgroup's span long: the channels are staged 5 at a time with a last batch of 4, and one
    at a time with the largest LDS the entry can ask for (L = 1, T = 4096: 64 KiB of table, 6920 cells of 8
    bytes).  L > T: the phases from T on have no tap and are exact zeros.  L = 300: a group of 8 L outputs spans
    several workgroups."""
    M = gpu[0]
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(T + K)
    n = (2 * CHUNK + 400) // L + 4
    n = (n + 1) // 2 * 2
    taps = taps_of(M, rng, T, max(L, 4))
    centres = centres_of(rng, K, 4800)
    x = Mq.iq_rows(rng, 2 * K, n, 0.05 if kind & Mq.S16 else 1.0)
    lens = np.full((2, K), n, np.int32)
    lens[1] = rng.integers(0, n, K)
    rows, nout = check(gpu, x, kind, 4800, taps, L, centres, int(centres[-1]), lens=lens)
    if L > T:
        flat = rows.reshape(2, rows.shape[1], -1)
        phase = np.arange(nout[0]) % L
        assert not np.any(flat[0, :nout[0]][phase >= T]) and np.any(flat[0, :nout[0]][phase < T])


# ---------------------------------------------------------------------------
# Q = +0.0: the real entry's output
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Mq.KINDS))
def test_with_q_zero_the_output_is_the_real_entrys(gpu, name):
    """one plan, one input: multiplex(iq=True) of (I, +0.0) == multiplex of I, bit for bit (the reason is
    tests/test_mux_iq_args.py's)"""
    M, torch, _ctx = gpu
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(kind + 5)
    L, T, P, K = 4, 129, 1920, 3
    n = (2 * CHUNK + 400) // L + 4
    taps = taps_of(M, rng, T, L)
    centres = np.array([-300, 30, 410], np.int32)
    gains = np.array([1.0, -0.5, 2.0], F32)
    x = np.zeros((2 * K, n, 2), F32)
    x[..., 0] = rng.standard_normal((2 * K, n)) * (0.05 if kind & Mq.S16 else 1.0)
    x[0, 5:9, 0] = [0.0, -0.0, 1e-40, -1e-40]
    lens = np.array([n, n - 5, 300, 17, n, 0], np.int32)
    plan = make_plan(gpu, kind, P, taps, L, centres, 170, gains)
    iq, niq = multiplex(gpu, plan, x, lens)
    real, nreal = multiplex(gpu, plan, np.ascontiguousarray(x[..., 0]), lens, iq=False)
    plan.close()
    assert_same(iq, real, niq, nreal)
    assert niq[0] == Mq.full_outputs(n, L, T) and np.any(iq)


# ---------------------------------------------------------------------------
# special values, PCM16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True])
def test_special_values(gpu, cx):
    M = gpu[0]
    kind = Mq.COMPLEX if cx else 0
    rng = np.random.default_rng(9)
    L, T, P, n, K = 3, 20, 65536, 900, 2
    taps = taps_of(M, rng, T, L)
    centres = np.array([1000, -20000], np.int32)
    x = Mq.iq_rows(rng, 7 * K, n)
    x[0, 100:400, 0], x[0, 100:400, 1] = 0.0, -0.0            # windows of zeros of both signs, in both planes
    x[1, 100:400, 0], x[1, 100:400, 1] = -0.0, 0.0
    x[2, :, 0] = (rng.integers(1, 1 << 22, n).astype(np.uint32)).view(F32)          # subnormals in I
    x[3, :, 1] = (rng.integers(1, 1 << 22, n).astype(np.uint32)).view(F32)          # ... in Q
    x[4] *= F32(1e30)                                         # in both
    x[5, :, 0] *= F32(1e30)
    x[6, 333, 0], x[7, 700, 1] = np.inf, -np.inf              # I; Q
    x[8, 444, 0], x[9, 555, 1] = np.nan, np.nan
    x[10, 222], x[11, 223] = (np.inf, -np.inf), (np.nan, np.nan)            # both
    x[12:14] *= 0.01
    rows, nout = check(gpu, x, kind, P, taps, L, centres, 1000)
    flat = rows.reshape(7, rows.shape[1], -1)
    for s in (4, 5):
        assert np.isnan(flat[s]).any() and not np.isnan(flat[s, :nout[s]]).all(), s  # it stays inside its tail
    assert (np.isinf(flat[3]) | np.isnan(flat[3])).any() and np.isfinite(flat[3]).any()
    assert np.isfinite(flat[1]).all() and np.isfinite(flat[2]).all() and np.any(flat[2])
    assert not np.any(flat[0, 110 * L:390 * L].view(np.uint32) & 0x7FFFFFFF)          # zeros in, zeros out
    # a NaN gain poisons every output its channel reaches, an infinite one the non-zero ones
    rows, nout = check(gpu, x[12:14], kind, P, taps, L, centres, 1000, gains=np.array([1.0, np.nan], F32),
                       lens=[n, n // 2])
    assert nout[0] == Mq.full_outputs(n, L, T) and np.isnan(rows.reshape(rows.shape[1], -1)[:nout[0]]).all()
    check(gpu, x[12:14], kind, P, taps, L, centres, 1000, gains=np.array([-np.inf, 0.0], F32))
    # taps that are not finite: a term outside the row is skipped, not multiplied by zero.  Outputs 0
    # and 2 have one term inside the row (taps 0 and 2); taps 3 and 11 would meet samples -1 and -3.
    bad = taps.copy()
    bad[3], bad[11] = np.nan, np.inf
    rows, _ = check(gpu, x[12:14], kind, P, bad, L, centres, 1000)
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
    """One tap of 1.0, L = 1, one channel, P = 1: (o, oi) is the finite sample (I, Q) itself.  I holds the
    values, Q holds them in reverse order."""
    kind = Mq.S16 | (Mq.COMPLEX if cx else 0)
    ties = lrintf_ties()
    assert ties.size >= 8 and {int(np.floor(v * 32767.0)) & 1 for v in ties.astype(np.float64)} == {0, 1}
    vals = np.concatenate([ties, F32([0.5, -0.5, 1.0, -1.0, 1.00002, -1.00002, -1.00004, 2.0, -2.0, 1e30, -1e30,
                                      0.0, -0.0, 3e-5, -3e-5])]).astype(F32)
    x = np.zeros((1, (vals.size + 1) // 2 * 2, 2), F32)
    x[0, :vals.size, 0], x[0, :vals.size, 1] = vals, vals[::-1]
    rows, nout = check(gpu, x, kind, 1, np.ones(1, F32), 1, [0], 0, lens=[vals.size])
    got = rows.reshape(rows.shape[1], -1)[:vals.size]
    assert nout[0] == vals.size and np.array_equal(got[:, 0], Mq.numpy_s16(vals))
    if cx:
        assert np.array_equal(got[:, 1], Mq.numpy_s16(vals[::-1]))
    assert got.max() == 32767 and got.min() == -32768 and got[list(vals).index(F32(0.5)), 0] == 16384
    # a NaN in either half gives 0 in every scalar it reaches
    x[0, 3, 1] = np.nan
    rows, _ = check(gpu, x, kind, 1, np.ones(1, F32), 1, [0], 0, lens=[vals.size])
    assert not np.any(rows.reshape(rows.shape[1], -1)[3])


@pytest.mark.parametrize("cx", [False, True])
def test_pcm16_rows_are_the_float_rows_through_the_conversion(gpu, cx):
    M = gpu[0]
    rng = np.random.default_rng(16)
    L, T, P, K, n = 40, 401, 4800, 5, 80
    taps = taps_of(M, rng, T, L)
    centres = centres_of(rng, K, P)
    x = Mq.iq_rows(rng, 2 * K, n, 1.5)                          # the sum clamps now and then
    x[3, 40, 1] = np.nan
    base = Mq.COMPLEX if cx else 0
    stride = (Mq.full_outputs(n, L, T) + 7) // 8 * 8           # a whole number of vectors of either kind
    f, nf = check(gpu, x, base, P, taps, L, centres, 170, out_stride=stride)
    s, ns = check(gpu, x, base | Mq.S16, P, taps, L, centres, 170, out_stride=stride)
    assert np.array_equal(nf, ns)
    assert np.array_equal(s, Mq.numpy_s16(f))
    assert (s == 32767).any() and (s == -32768).any()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Mq.KINDS))
def test_what_the_entry_refuses_of_the_io(gpu, name):
    """with a plan of each kind and real arrays: every refusal comes back in the real entry's order, and after
    each one both outputs and their guard cells hold what they held"""
    M, torch, _ctx = gpu
    lib = _lib.load()
    kind = Mq.KINDS[name]
    vec = Mq.vec_of(kind)
    L, T = 4, 65
    plan = make_plan(gpu, kind, 4800, M.channel_taps(T, 1200.0, 192000.0, 4.0), L, [117, -60], 170)
    n, out_stride = 40, 256
    assert out_stride % vec == 0 and out_stride > Mq.full_outputs(n, L, T)
    d = torch.from_numpy(Mq.iq_rows(np.random.default_rng(3), 4, n)).cuda()
    fr, fn, out, guard = guarded(torch, plan, 2, out_stride, d.device)
    before = (fr.cpu().numpy().copy(), fn.cpu().numpy().copy())
    samples, rows, nout = d.data_ptr(), out["rows"].data_ptr(), out["nsamples"].data_ptr()
    assert samples % 16 == 0 and rows % 16 == 0

    def io_of(**kw):
        io = _lib.MuxIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
        io.d_out, io.out_stride, io.nout_cap, io.d_nout = rows, out_stride, out_stride, nout
        for k, v in kw.items():
            setattr(io, k, v)
        return io

    def rc(ctx=plan.handle, **kw):
        got = lib.mifsk_multiplex_iq_batch(ctx, C.byref(io_of(**kw)), None)
        torch.cuda.synchronize()
        assert np.array_equal(fr.cpu().numpy(), before[0]) and np.array_equal(fn.cpu().numpy(), before[1]), kw
        return got

    assert lib.mifsk_multiplex_iq_batch(plan.handle, None, None) == EINVAL
    for field in ("d_samples", "d_out", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (4, 8, 12):                                      # 8: a whole element, not 16 bytes
        assert rc(d_samples=samples + off) == EINVAL, off
    for stride in (n + 1, n + 3, 1, 4001):                      # odd: not a whole number of 16-byte vectors
        assert rc(stream_stride=stride) == EINVAL, stride
    for off in (2, 4, 8):
        assert rc(d_out=rows + off) == EINVAL, off
    assert rc(out_stride=0, nout_cap=0) == EINVAL
    for stride in range(out_stride + 1, out_stride + vec):      # not a whole number of 16-byte vectors
        assert rc(out_stride=stride) == EINVAL, stride
    assert rc(out_stride=(1 << 32) - 8 + vec, nout_cap=0) == EINVAL and rc(out_stride=1 << 40, nout_cap=0) == EINVAL
    assert rc(nout_cap=out_stride + 1) == EINVAL and rc(nout_cap=0xFFFFFFFF) == EINVAL
    assert rc(nstreams=(1 << 30) + 1) == EINVAL                 # nstreams * nchannels
    ladder(rc, dict(nstreams=(1 << 30) + 1),
           [dict(d_nout=None), dict(nstreams=0), dict(d_samples=samples + 8), dict(stream_stride=n + 1),
            dict(d_out=rows + 8), dict(out_stride=0, nout_cap=0), dict(out_stride=out_stride + vec - 1),
            dict(out_stride=1 << 40, nout_cap=0), dict(nout_cap=out_stride + 1)])
    # what passes the checks runs: the same io, nothing replaced
    assert lib.mifsk_multiplex_iq_batch(plan.handle, C.byref(io_of()), None) == 0
    torch.cuda.synchronize()
    plan.close()
    assert np.all(out["nsamples"].cpu().numpy() == Mq.full_outputs(n, L, T))
    got = fr.cpu().numpy()
    g = GUARD * 8
    assert np.all(got[:g] == got.dtype.type(guard)) and np.all(got[-g:] == got.dtype.type(guard))
    want, _wn = expect(d.cpu().numpy(), kind, 4800, M.channel_taps(T, 1200.0, 192000.0, 4.0), L,
                       np.array([117, -60], np.int32), 170, None, None, None, out_stride)
    assert Mq.same_bits(out["rows"].cpu().numpy(), want)


# ---------------------------------------------------------------------------
# more streams than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_a_batch_of_more_streams_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    ns, n, cut = 65537, 8, 40000
    x = Mq.iq_rows(rng, ns, n)
    P, taps, L, centres, r = 7, np.array([0.75, -0.5, 0.25], F32), 2, np.array([3], np.int32), 1
    full = Mq.full_outputs(n, L, taps.size)
    plan = make_plan(gpu, 0, P, taps, L, centres, r)
    d = torch.from_numpy(x).cuda()
    whole = M.multiplex(plan, d, iq=True)
    parts = [M.multiplex(plan, d[:cut], iq=True), M.multiplex(plan, d[cut:], iq=True)]
    torch.cuda.synchronize()
    plan.close()
    rows, nout = whole["rows"].cpu().numpy(), whole["nsamples"].cpu().numpy()
    assert rows.shape == (ns, default_stride(0, n, L, taps.size)) and np.all(nout == full)
    assert Mq.same_bits(rows, np.concatenate([p["rows"].cpu().numpy() for p in parts]))
    assert np.array_equal(nout, np.concatenate([p["nsamples"].cpu().numpy() for p in parts]))
    for s in (0, 65534, 65535, 65536):
        want, cnt = Mq.ref_multiplex_iq(x[s:s + 1], None, 0, P, taps, L, centres, r)
        assert cnt == full and Mq.same_bits(rows[s], want), s


# ---------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------
def test_the_python_surface(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(21)
    P, n = 4800, 600
    ta, tb = taps_of(M, rng, 65, 4), taps_of(M, rng, 401, 40)
    ca, cb = np.array([117, 237, -57], np.int32), centres_of(rng, 5, P)
    x1, x2 = Mq.iq_rows(rng, 6, n), Mq.iq_rows(rng, 6, n)
    xb = Mq.iq_rows(rng, 5, 60)
    pa = make_plan(gpu, 0, P, ta, 4, ca, 170)
    pb = make_plan(gpu, Mq.COMPLEX, P, tb, 40, cb, 170)
    d1, d2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    # shapes and types; complex64 is the same rows
    a = M.multiplex(pa, d1, iq=True)
    b = M.multiplex(pa, torch.view_as_complex(d1), iq=True)
    capped = M.multiplex(pa, d1, nout_cap=100, iq=True)
    torch.cuda.synchronize()
    assert a["rows"].dtype == torch.float32 and a["rows"].shape == (2, default_stride(0, n, 4, 65))
    assert a["nsamples"].dtype == torch.int32 and a["nsamples"].shape == (2,)
    assert capped["rows"].shape == (2, 100) and np.all(capped["nsamples"].cpu().numpy() == 100)
    want, wn = expect(x1, 0, P, ta, 4, ca, 170, None, None, None, a["rows"].shape[1])
    assert_same(a["rows"].cpu().numpy(), want, a["nsamples"].cpu().numpy(), wn)
    assert_same(b["rows"].cpu().numpy(), want, b["nsamples"].cpu().numpy(), wn)
    assert Mq.same_bits(capped["rows"].cpu().numpy(), want[:, :100])
    # out= reuse on a stream of its own: shorter rows leave no old outputs behind
    side = torch.cuda.Stream()
    short = [n, 150, 70, 0, 0, 3]
    torch.cuda.synchronize()
    again = M.multiplex(pa, d2, nsamples=torch.from_numpy(np.array(short, np.int32)).cuda(), stream=side, out=a, iq=True)
    side.synchronize()
    assert again is a
    want2, wn2 = expect(x2, 0, P, ta, 4, ca, 170, None, short, None, a["rows"].shape[1])
    assert_same(a["rows"].cpu().numpy(), want2, a["nsamples"].cpu().numpy(), wn2)
    # rows that are not I/Q rows are refused, and I/Q rows without the switch
    with pytest.raises(AssertionError):
        M.multiplex(pa, d1[..., 0].contiguous(), iq=True)
    with pytest.raises(AssertionError):
        M.multiplex(pa, d1)
    # iq=False on the same plan is the path it was
    real_in = np.ascontiguousarray(x1[..., 0])
    rows, nout = multiplex(gpu, pa, real_in, iq=False)
    wrows, wcnt = zip(*[Mx.ref_multiplex(real_in[s * 3:s * 3 + 3], None, 0, P, ta, 4, ca, 170, None, rows.shape[1])
                        for s in range(2)])
    assert_same(rows, np.stack(wrows), nout, np.array(wcnt, np.int32))
    # two plans on two streams at once give what each gives alone
    alone_a, alone_b = multiplex(gpu, pa, x1), multiplex(gpu, pb, xb)
    db = torch.from_numpy(xb).cuda()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    both_a = M.multiplex(pa, d1, stream=sa, iq=True)
    both_b = M.multiplex(pb, db, stream=sb, iq=True)
    sa.synchronize()
    sb.synchronize()
    assert both_b["rows"].shape == (1, default_stride(Mq.COMPLEX, 60, 40, 401), 2)
    assert_same(both_a["rows"].cpu().numpy(), alone_a[0], both_a["nsamples"].cpu().numpy(), alone_a[1])
    assert_same(both_b["rows"].cpu().numpy(), alone_b[0], both_b["nsamples"].cpu().numpy(), alone_b[1])
    want_b, wn_b = expect(xb, Mq.COMPLEX, P, tb, 40, cb, 170, None, None, None, alone_b[0].shape[1])
    assert_same(alone_b[0], want_b, alone_b[1], wn_b)
    pa.close()
    pb.close()


# ---------------------------------------------------------------------------
# end to end: three FM channels made at 48 kHz go onto one capture and come off it on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cnr_db", [None, 14.0], ids=["clean", "cnr14"])
def test_three_fm_channels_through_one_capture_on_the_device(gpu, cnr_db):
    """synthesize_batch at 48 kHz -> one fm_modulate call for the three rows (centre 0, amplitude 0.3) ->
    multiplex(iq=True) onto -30, +3 and +41 kHz of a 192 kHz complex capture -> impair over the row as reals ->
    channelize(iq=True) -> fm_demod -> demod_batch.  The transmitted audio goes to the host, the restatements
    make every stage there (fm_ref.c, mux_ref_iq, impair_ref.c, channel_ref_iq, fm_ref.c) and the oracle decodes
    the three audio rows to exactly their 16 bytes BEFORE anything of the device's is looked at.  Then the
    device's I/Q rows, capture, noisy capture, channel rows, audio rows and lengths equal the host's bit for
    bit, its frames, bytes and episodes the oracle's, and its bytes the messages."""
    M, torch, ctx = gpu
    words = Iq.fm_messages()
    tx_cfg, ocfg = M.rx_config("1200", sample_rate=Mq.FS_IN), O.oracle_config("1200")
    lead = torch.from_numpy(np.array(Mq.TX_LEAD, np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, tx_cfg, torch.from_numpy(words).cuda(), amplitude=1.0, leading_silence=lead)
    n = clean.shape[1]
    assert n % 4 == 0 and n <= 10000
    sigma = Iq.fm_sigma(M, cnr_db)

    host = Mq.fm_host_chain(M, clean.cpu().numpy(), lens.cpu().numpy().astype(np.uint32), sigma)
    nout = host["nout"]
    for k in range(3):                                          # the precondition: the oracle has every message whole
        assert O.oracle_rx_stream(ocfg, host["audio"][k, :nout])["bytes"] == words[k].tobytes(), k

    iq = M.fm_modulate(ctx, clean, nsamples=lens, deviation=M.fm_step(Iq.DEVIATION_HZ, Mq.FS_IN), centre=0.0,
                       amplitude=Iq.CARRIER)
    mplan = M.MuxPlan(ctx, host["taps"], Mq.L_FM, Iq.CENTRES, 0, Iq.P_FM, complex_output=True)
    cap = M.multiplex(mplan, iq, nsamples=lens, iq=True)
    stride = cap["rows"].shape[1]
    noisy = M.impair(ctx, cap["rows"].view(1, 2 * stride), seed=Iq.SEED, sigma=sigma).view(1, stride, 2)
    cplan = M.ChannelPlan(ctx, host["rx_taps"], Iq.D_FM, Iq.CENTRES, 0, Iq.P_FM, complex_input=True)
    ch = M.channelize(cplan, noisy, nsamples=cap["nsamples"], iq=True)
    audio = M.fm_demod(ctx, ch["rows"], nsamples=ch["nsamples"], gain=M.fm_gain(Iq.FS / Iq.D_FM, Iq.DEVIATION_HZ))
    out = M.demod_batch(ctx, M.rx_config("1200"), audio, nsamples=ch["nsamples"], want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    mplan.close()
    cplan.close()
    assert Mq.same_bits(iq.cpu().numpy(), host["iq"])
    assert_same(cap["rows"].cpu().numpy()[0], host["capture"], cap["nsamples"].cpu().numpy(),
                np.array([host["count"]], np.int32))
    assert Mq.same_bits(noisy.cpu().numpy()[0], host["noisy"])
    got_n = ch["nsamples"].cpu().numpy()
    assert np.array_equal(got_n, np.full(3, nout, np.int32))
    assert Mq.same_bits(ch["rows"].cpu().numpy(), host["ch"])
    assert Mq.same_bits(audio.cpu().numpy(), host["audio"])
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, host["audio"], got_n.astype(np.uint32), res, threads=3)
    assert bad == []
    for k in range(3):
        assert res["bytes"][k, :int(res["nbytes"][k])].tobytes() == words[k].tobytes(), k
