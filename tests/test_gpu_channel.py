"""mifsk_channelize_batch (include/mifsk.h, minimodem_amd/csrc/mifsk_channel.hip) against the host
restatement tools/channel_ref.c: every output of every case bit for bit on the float patterns, no
tolerance (a NaN equals a NaN).  Rows are at most 40 000 elements, batches at most 9 rows (but for one of 65 537 rows of 16); both
output arrays are made with guard cells around them, which every call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import _channel as Ch
import _oracle as O
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
ROW_GUARD, NOUT_GUARD = F32(7.25), -77
EINVAL = -22


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def vec_of(kind):
    return 16 // ((2 if kind & Ch.S16 else 4) * (2 if kind & Ch.COMPLEX else 1))


def random_rows(rng, kind, nrows, n):
    shape = (nrows, n, 2) if kind & Ch.COMPLEX else (nrows, n)
    if kind & Ch.S16:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    return rng.standard_normal(shape).astype(F32)


def make_plan(gpu, kind, P, taps, D, centres, r):
    M, _torch, ctx = gpu
    return M.ChannelPlan(ctx, taps, D, centres, r, P, complex_input=bool(kind & Ch.COMPLEX), s16=bool(kind & Ch.S16))


def channelize(gpu, plan, x, lens=None, nout_cap=None, out_stride=None, stream=None):
    """One call with guard cells around both outputs -> (rows [nstreams * K, out_stride], nout) as numpy."""
    M, torch, _ctx = gpu
    d = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ns, width = d.shape[0], d.shape[1]
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    if out_stride is None:
        full = M.carrier_windows(width, plan.ntaps, plan.decim) if nout_cap is None else nout_cap
        out_stride = max(4, (full + 3) // 4 * 4)
    nrows = ns * plan.nchannels
    fr = torch.full((nrows * out_stride + 2 * GUARD,), float(ROW_GUARD), dtype=torch.float32, device=d.device)
    fn = torch.full((nrows + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device=d.device)
    out = {"rows": fr[GUARD:GUARD + nrows * out_stride].view(nrows, out_stride), "nsamples": fn[GUARD:GUARD + nrows]}
    res = M.channelize(plan, d, nsamples=dl, nout_cap=nout_cap, stream=stream, out=out)
    torch.cuda.synchronize()
    assert res is out
    fr, fn = fr.cpu().numpy(), fn.cpu().numpy()
    for guard in (fr[:GUARD], fr[-GUARD:]):
        assert np.all(guard == ROW_GUARD), "the guard cells around the rows were written"
    for guard in (fn[:GUARD], fn[-GUARD:]):
        assert np.all(guard == NOUT_GUARD), "the guard cells around the counts were written"
    return fr[GUARD:-GUARD].reshape(nrows, out_stride), fn[GUARD:-GUARD]


def expect(x, kind, P, taps, D, centres, r, lens, nout_cap, out_stride):
    """what the call must leave: the restatement's outputs, cut at nout_cap, zeros behind"""
    K = len(centres)
    rows = np.zeros((x.shape[0] * K, out_stride), F32)
    nout = np.zeros(x.shape[0] * K, np.int32)
    for s in range(x.shape[0]):
        ref = Ch.ref_channelize(x[s], kind, P, taps, D, centres, r, n=None if lens is None else lens[s])
        cnt = min(ref.shape[1], out_stride if nout_cap is None else nout_cap)
        rows[s * K:(s + 1) * K, :cnt] = ref[:, :cnt]
        nout[s * K:(s + 1) * K] = cnt
    return rows, nout


def check(gpu, x, kind, P, taps, D, centres, r, lens=None, nout_cap=None, out_stride=None, plan=None):
    own = plan is None
    plan = plan or make_plan(gpu, kind, P, taps, D, centres, r)
    rows, nout = channelize(gpu, plan, x, lens, nout_cap, out_stride)
    if own:
        plan.close()
    want_rows, want_nout = expect(np.asarray(x), kind, P, taps, D, centres, r, lens, nout_cap, rows.shape[1])
    assert np.array_equal(nout, want_nout), (nout, want_nout)
    if not Ch.same_f32(rows, want_rows):
        bad = np.argwhere((rows.view(np.uint32) != want_rows.view(np.uint32)) & ~(np.isnan(rows) & np.isnan(want_rows)))
        raise AssertionError("%d outputs differ, first (row, m) = %s: %r != %r" % (
            len(bad), bad[0], rows[tuple(bad[0])], want_rows[tuple(bad[0])]))
    return rows, nout


# ---------------------------------------------------------------------------
# kinds and sizes
# ---------------------------------------------------------------------------
# outputs per full row: more than two of the kernel's chunks (2048 / 1024 / 64 / 32 outputs by K)
M_TARGET = {1: 4500, 2: 2300, 3: 2300, 63: 150, 64: 150, 65: 80, 130: 80}


def size_cases():
    """_channel.size_cases() (whose coverage tests/test_channel_args.py asserts) as pytest parameters"""
    return [pytest.param(*c, id="%s-T%d-D%d-K%d-P%d" % c) for c in Ch.size_cases()]


def centres_of(rng, K, P):
    fixed = [0, -1, P // 2, -(P - 1), 1, -(P // 2)]
    more = rng.integers(-(P - 1), P, max(0, K - len(fixed)))
    return np.array((fixed + [int(v) for v in more])[:K], np.int32)


@pytest.mark.parametrize("name,T,D,K,P", size_cases())
def test_kinds_and_sizes(gpu, name, T, D, K, P):
    M = gpu[0]
    kind = Ch.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + D)
    vec = vec_of(kind)
    n = min(40000, T + (M_TARGET[K] - 1) * D + 3)
    n = (n + vec - 1) // vec * vec
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
    centres = centres_of(rng, K, P)
    x = random_rows(rng, kind, 2, n)
    lens = [n, n - (n // 3)]
    for r in (0, int(centres[-1])):             # r = 0 and r = q (of the last channel)
        check(gpu, x, kind, P, taps, D, centres, r, lens=lens)


# ---------------------------------------------------------------------------
# ragged batches, capacity, alignment, special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Ch.KINDS))
def test_ragged_batches_and_capacity(gpu, name):
    M = gpu[0]
    kind = Ch.KINDS[name]
    rng = np.random.default_rng(7)
    T, D, P = 65, 4, 4800
    vec = vec_of(kind)
    n = 2400 // vec * vec
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0)
    centres = np.array([117, -60, 2400], np.int32)
    lens = [0, T - 1, T, T + D - 1, T + D, n]
    x = random_rows(rng, kind, len(lens), n)
    full = (n - T) // D + 1
    plan = make_plan(gpu, kind, P, taps, D, centres, 117)
    for nout_cap, out_stride in ((None, None), (full - 37, (full + 3) // 4 * 4), (1, 8), (full + 9, full + 9 + 11 & ~3),
                                 (0, 4)):
        rows, nout = check(gpu, x, kind, P, taps, D, centres, 117, lens=lens, nout_cap=nout_cap,
                           out_stride=out_stride, plan=plan)
        cap = rows.shape[1] if nout_cap is None else nout_cap
        want = [min(cap, c) for c in (0, 0, 1, 1, 2, full)]
        assert list(nout.reshape(len(lens), 3)[:, 0]) == want
        for i, c in enumerate(nout):
            assert not np.any(rows[i, c:].view(np.uint32)), "the tail of row %d is not +0.0f" % i
    # lengths beyond the stride are clamped to it
    check(gpu, x, kind, P, taps, D, centres, 117, lens=[n + 1000] * len(lens), plan=plan)
    plan.close()


@pytest.mark.parametrize("name", list(Ch.KINDS))
def test_rows_at_every_alignment_the_stride_rule_allows(gpu, name):
    M, torch, _ctx = gpu
    kind = Ch.KINDS[name]
    rng = np.random.default_rng(5)
    vec = vec_of(kind)
    T, D, P = 63, 3, 4799
    taps = M.channel_taps(T, 500.0, 48000.0, 1.0)
    centres = np.array([5, -700], np.int32)
    n, stride = 37 * vec - 1, 37 * vec                        # 37 vectors: the rows walk through every alignment
    pool = torch.from_numpy(random_rows(rng, kind, 1, 8 * vec + 3 * stride)[0]).cuda()
    plan = make_plan(gpu, kind, P, taps, D, centres, 5)
    for j in range(8):                                        # the base at each 16-byte step of a 128-byte line
        x = pool[j * vec:j * vec + 3 * stride].view((3, stride) + tuple(pool.shape[1:]))[:, :n]
        assert x.data_ptr() % 16 == 0 and x.data_ptr() % 128 == (pool.data_ptr() + 16 * j) % 128
        rows, _nout = channelize(gpu, plan, x)
        want, _ = expect(x.cpu().numpy(), kind, P, taps, D, centres, 5, None, None, rows.shape[1])
        assert Ch.same_f32(rows, want), j
    plan.close()


@pytest.mark.parametrize("cx", [False, True])
def test_special_values(gpu, cx):
    M = gpu[0]
    kind = Ch.COMPLEX if cx else 0
    rng = np.random.default_rng(9)
    T, D, P, n = 64, 7, 65536, 4000
    taps = M.channel_taps(T, 3000.0, 48000.0, 2.0)
    centres = np.array([0, 1000, -20000, P // 2], np.int32)
    x = random_rows(rng, kind, 5, n)
    flat = x.reshape(5, -1)
    flat[0, 300:1500] = 0.0                                   # windows of zeros
    flat[0, 2000:2600] = -0.0
    flat[1, :] = (rng.integers(1, 1 << 22, flat.shape[1]).astype(np.uint32)).view(F32)     # subnormals
    flat[1, ::2] *= -1.0
    flat[2, :] *= F32(1e30)
    flat[3, 1111], flat[3, 2999] = np.inf, -np.inf
    flat[4, 2222] = np.nan
    rows, _nout = check(gpu, x, kind, P, taps, D, centres, 1000)
    assert np.isnan(rows[16:20]).any() and not np.isnan(rows[16:20]).all()     # the NaN stays inside its windows
    assert (np.isinf(rows[12:16]) | np.isnan(rows[12:16])).any() and np.isfinite(rows[12:16]).any()
    assert not np.any(rows[0:4, 50:95].view(np.uint32) & 0x7FFFFFFF)           # zeros in, zeros out


def test_pcm16_rows_give_what_ingest_and_the_float_call_give(gpu):
    M, torch, ctx = gpu
    rng = np.random.default_rng(16)
    T, D, P, n = 65, 4, 4800, 3200
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0)
    centres = np.array([117, -60, 2400], np.int32)
    pcm = random_rows(rng, Ch.S16, 3, n)
    pcm[0, :8] = [-32768, 32767, 0, -1, 1, 12345, -12345, 256]
    lens = [n, n - 801, 1000]
    got, nout = check(gpu, pcm, Ch.S16, P, taps, D, centres, 117, lens=lens)
    f = M.ingest_s16(ctx, torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), pcm.astype(F32) / F32(32768.0))
    via, nvia = check(gpu, f.cpu().numpy(), 0, P, taps, D, centres, 117, lens=lens)
    assert Ch.same_f32(got, via) and np.array_equal(nout, nvia)
    # complex PCM16 against the converted complex float row
    iq = random_rows(rng, Ch.COMPLEX | Ch.S16, 2, n)
    got, nout = check(gpu, iq, Ch.COMPLEX | Ch.S16, P, taps, D, centres, 117)
    via, nvia = check(gpu, iq.astype(F32) / F32(32768.0), Ch.COMPLEX, P, taps, D, centres, 117)
    assert Ch.same_f32(got, via) and np.array_equal(nout, nvia)


def test_complex64_tensors_and_one_row(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(64)
    T, D, P, n = 63, 4, 4800, 2000
    taps = M.channel_taps(T, 400.0, 48000.0, 1.0)
    centres = np.array([-300, 30], np.int32)
    x = random_rows(rng, Ch.COMPLEX, 2, n)
    plan = make_plan(gpu, Ch.COMPLEX, P, taps, D, centres, 17)
    a = M.channelize(plan, torch.from_numpy(x).cuda())
    b = M.channelize(plan, torch.view_as_complex(torch.from_numpy(x).cuda()))
    one = M.channelize(plan, torch.from_numpy(x[1]).cuda())
    torch.cuda.synchronize()
    assert a["rows"].dtype == torch.float32 and a["nsamples"].dtype == torch.int32
    assert a["rows"].shape == (4, (((n - T) // D + 1) + 3) // 4 * 4)
    want, wn = expect(x, Ch.COMPLEX, P, taps, D, centres, 17, None, None, a["rows"].shape[1])
    assert Ch.same_f32(a["rows"].cpu().numpy(), want) and Ch.same_f32(b["rows"].cpu().numpy(), want)
    assert np.array_equal(a["nsamples"].cpu().numpy(), wn) and np.array_equal(b["nsamples"].cpu().numpy(), wn)
    assert Ch.same_f32(one["rows"].cpu().numpy(), want[2:])
    plan.close()


# ---------------------------------------------------------------------------
# reuse, plans, streams
# ---------------------------------------------------------------------------
def test_reuse_of_a_plan_and_of_its_outputs_and_two_plans_at_once(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(21)
    P, n = 4800, 3000
    ta, tb = M.channel_taps(65, 400.0, 48000.0, 2.0), M.channel_taps(385, 300.0, 48000.0, 2.0)
    ca, cb = np.array([117, 237, 57], np.int32), centres_of(rng, 65, P)
    x1, x2 = random_rows(rng, 0, 3, n), random_rows(rng, 0, 3, n)
    pa = make_plan(gpu, 0, P, ta, 4, ca, 117)
    alone1 = channelize(gpu, pa, x1)
    pb = make_plan(gpu, 0, P, tb, 7, cb, 0)                    # two plans alive at once
    both_b = channelize(gpu, pb, x1)
    both_a2 = channelize(gpu, pa, x2)                          # a second call on the same plan, other rows
    both_a1 = channelize(gpu, pa, x1)
    pa.close()
    alone_b = channelize(gpu, pb, x1)
    pb.close()
    assert Ch.same_f32(alone1[0], both_a1[0]) and Ch.same_f32(both_b[0], alone_b[0])
    for got, x, taps, D, c, r in ((alone1, x1, ta, 4, ca, 117), (both_a2, x2, ta, 4, ca, 117), (both_b, x1, tb, 7, cb, 0)):
        want, wn = expect(x, 0, P, taps, D, c, r, None, None, got[0].shape[1])
        assert Ch.same_f32(got[0], want) and np.array_equal(got[1], wn)
    # out= reuse, on a stream of its own: the same as fresh calls, shorter rows leave no old outputs behind
    pa = make_plan(gpu, 0, P, ta, 4, ca, 117)
    side = torch.cuda.Stream()
    d1, d2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    short = torch.from_numpy(np.array([n, 1500, 70], np.int32)).cuda()
    torch.cuda.synchronize()
    out = M.channelize(pa, d1, stream=side)
    side.synchronize()
    first = out["rows"].cpu().numpy().copy()
    again = M.channelize(pa, d2, nsamples=short, stream=side, out=out)
    side.synchronize()
    assert again is out and Ch.same_f32(first, alone1[0])
    want, wn = expect(x2, 0, P, ta, 4, ca, 117, [n, 1500, 70], None, first.shape[1])
    assert Ch.same_f32(out["rows"].cpu().numpy(), want) and np.array_equal(out["nsamples"].cpu().numpy(), wn)
    pa.close()


@pytest.mark.parametrize("name", list(Ch.KINDS))
def test_what_channelize_refuses_of_the_io(gpu, name):
    """with a plan of each kind: every refusal comes back before a launch (the pointers are numbers)"""
    M, _torch, _ctx = gpu
    lib = _lib.load()
    kind = Ch.KINDS[name]
    vec = vec_of(kind)
    plan = make_plan(gpu, kind, 4800, M.channel_taps(65, 400.0, 48000.0, 2.0), 4, [117, -60], 117)
    base = 1 << 20

    def rc(**kw):
        io = _lib.ChannelIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = base, 4000, None, 4000, 2
        io.d_rows, io.out_stride, io.nout_cap, io.d_nout = base + (1 << 24), 4000, 4000, base + (1 << 26)
        for k, v in kw.items():
            setattr(io, k, v)
        return lib.mifsk_channelize_batch(plan.handle, C.byref(io), None)

    assert lib.mifsk_channelize_batch(plan.handle, None, None) == EINVAL
    for field in ("d_samples", "d_rows", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (2, 4, 8):
        assert rc(d_samples=base + off) == EINVAL, off
    for stride in range(4000 + 1, 4000 + vec):                  # not a whole number of 16-byte vectors
        assert rc(stream_stride=stride) == EINVAL, stride
    assert rc(d_rows=base + (1 << 24) + 4) == EINVAL
    for out_stride in (0, 3998, 4001, 4002):
        assert rc(out_stride=out_stride, nout_cap=0) == EINVAL, out_stride
    assert rc(nout_cap=4001) == EINVAL and rc(nout_cap=0xFFFFFFFF) == EINVAL
    assert rc(nstreams=(1 << 30) + 1) == EINVAL                 # nstreams * nchannels
    assert rc(stream_stride=4001, d_rows=None) == EINVAL
    plan.close()


# ---------------------------------------------------------------------------
# end to end: channelize -> demod_batch on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("make", [Ch.three_bell103, Ch.three_bell202_iq])
def test_every_signal_of_a_recording_decodes_on_the_device(gpu, make):
    M, torch, ctx = gpu
    c = make()
    assert c["x"].shape[0] <= 40000
    plan = make_plan(gpu, c["kind"], c["P"], c["taps"], c["D"], c["centres"], c["r"])
    ch = M.channelize(plan, torch.from_numpy(c["x"]).cuda())
    cfg, ocfg = M.rx_config(c["mode"]), O.oracle_config(c["mode"])
    out = M.demod_batch(ctx, cfg, ch["rows"], nsamples=ch["nsamples"], want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    plan.close()
    rows, lens = ch["rows"].cpu().numpy(), ch["nsamples"].cpu().numpy()
    want, wn = expect(c["x"][None], c["kind"], c["P"], c["taps"], c["D"], c["centres"], c["r"], None, None, rows.shape[1])
    assert Ch.same_f32(rows, want) and np.array_equal(lens, wn)
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, rows, lens, res, threads=3)
    assert bad == []                                           # frames, bytes and episodes of the device-made rows
    for k, payload in enumerate(c["payloads"]):
        decoded = res["bytes"][k, :int(res["nbytes"][k])].tobytes()
        assert Ch.payload_condition(decoded, payload), (k, decoded, payload)


# ---------------------------------------------------------------------------
# more rows than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_a_batch_of_more_rows_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    nrows, n, cut = 65537, 16, 40000
    x = rng.standard_normal((nrows, n)).astype(F32)
    P, taps, D, centres, r = 7, np.array([0.75, -0.5], F32), 1, np.array([3], np.int32), 1
    plan = make_plan(gpu, 0, P, taps, D, centres, r)
    d = torch.from_numpy(x).cuda()
    whole = M.channelize(plan, d)
    parts = [M.channelize(plan, d[:cut]), M.channelize(plan, d[cut:])]
    torch.cuda.synchronize()
    plan.close()
    rows, nout = whole["rows"].cpu().numpy(), whole["nsamples"].cpu().numpy()
    assert rows.shape == (nrows, 16) and np.all(nout == n - 1)
    assert Ch.same_f32(rows, np.concatenate([p["rows"].cpu().numpy() for p in parts]))
    assert np.array_equal(nout, np.concatenate([p["nsamples"].cpu().numpy() for p in parts]))
    for s in (0, 65534, 65535, 65536):
        want = Ch.ref_channelize(x[s], 0, P, taps, D, centres, r)
        assert want.shape == (1, n - 1) and Ch.same_f32(rows[s, :n - 1], want[0]) and rows[s, n - 1] == 0, s
