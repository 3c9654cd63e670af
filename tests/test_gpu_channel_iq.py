"""mifsk_channelize_iq_batch (include/mifsk/channel_iq.h, minimodem_amd/csrc/mifsk_channel.hip) against the
host restatement channel_ref_iq (tools/channel_ref.c): the whole output of every case -- I, Q and the zero
tails -- bit for bit on the float patterns, no tolerance (a NaN equals a NaN).  Rows are at most 40 000
elements, batches at most 6 rows (but for one of 65 537 rows of 16); both output arrays are made with guard
cells around them, which every call must leave alone."""
import ctypes as C

import numpy as np
import pytest

import _channel_iq as Iq
import _oracle as O
from _abi import EINVAL, ladder
from minimodem_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
ROW_GUARD, NOUT_GUARD = F32(7.25), -77


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def vec_of(kind):
    return 16 // ((2 if kind & Iq.S16 else 4) * (2 if kind & Iq.COMPLEX else 1))


def even(n):
    return (int(n) + 1) // 2 * 2


def make_plan(gpu, kind, P, taps, D, centres, r):
    M, _torch, ctx = gpu
    return M.ChannelPlan(ctx, taps, D, centres, r, P, complex_input=bool(kind & Iq.COMPLEX), s16=bool(kind & Iq.S16))


def guarded(torch, nrows, out_stride, device):
    """both outputs with guard cells around them -> (the rows' buffer, the counts' buffer, out=)"""
    fr = torch.full((nrows * out_stride * 2 + 2 * GUARD,), float(ROW_GUARD), dtype=torch.float32, device=device)
    fn = torch.full((nrows + 2 * GUARD,), NOUT_GUARD, dtype=torch.int32, device=device)
    out = {"rows": fr[GUARD:GUARD + nrows * out_stride * 2].view(nrows, out_stride, 2), "nsamples": fn[GUARD:GUARD + nrows]}
    return fr, fn, out


def channelize_iq(gpu, plan, x, lens=None, nout_cap=None, out_stride=None, stream=None):
    """One call with guard cells around both outputs -> (rows [nstreams * K, out_stride, 2], nout) as numpy."""
    M, torch, _ctx = gpu
    d = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ns, width = d.shape[0], d.shape[1]
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    if out_stride is None:
        full = M.carrier_windows(width, plan.ntaps, plan.decim) if nout_cap is None else nout_cap
        out_stride = max(2, even(full))
    nrows = ns * plan.nchannels
    fr, fn, out = guarded(torch, nrows, out_stride, d.device)
    res = M.channelize(plan, d, nsamples=dl, nout_cap=nout_cap, stream=stream, out=out, iq=True)
    torch.cuda.synchronize()
    assert res is out
    fr, fn = fr.cpu().numpy(), fn.cpu().numpy()
    for guard in (fr[:GUARD], fr[-GUARD:]):
        assert np.all(guard == ROW_GUARD), "the guard cells around the rows were written"
    for guard in (fn[:GUARD], fn[-GUARD:]):
        assert np.all(guard == NOUT_GUARD), "the guard cells around the counts were written"
    return fr[GUARD:-GUARD].reshape(nrows, out_stride, 2), fn[GUARD:-GUARD]


def expect(x, kind, P, taps, D, centres, r, lens, nout_cap, out_stride):
    """what the call must leave: the restatement's outputs, cut at nout_cap, (+0.0f, +0.0f) behind"""
    K = len(centres)
    rows = np.zeros((x.shape[0] * K, out_stride, 2), F32)
    nout = np.zeros(x.shape[0] * K, np.int32)
    for s in range(x.shape[0]):
        ref = Iq.ref_channelize_iq(x[s], kind, P, taps, D, centres, r, n=None if lens is None else lens[s])
        cnt = min(ref.shape[1], out_stride if nout_cap is None else nout_cap)
        rows[s * K:(s + 1) * K, :cnt] = ref[:, :cnt]
        nout[s * K:(s + 1) * K] = cnt
    return rows, nout


def assert_same(rows, want):
    if not Iq.same_f32(rows, want):
        bad = np.argwhere((rows.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(rows) & np.isnan(want)))
        raise AssertionError("%d values differ, first (row, m, I/Q) = %s: %r != %r" % (
            len(bad), bad[0], rows[tuple(bad[0])], want[tuple(bad[0])]))


def check(gpu, x, kind, P, taps, D, centres, r, lens=None, nout_cap=None, out_stride=None, plan=None):
    own = plan is None
    plan = plan or make_plan(gpu, kind, P, taps, D, centres, r)
    rows, nout = channelize_iq(gpu, plan, x, lens, nout_cap, out_stride)
    if own:
        plan.close()
    want_rows, want_nout = expect(np.asarray(x), kind, P, taps, D, centres, r, lens, nout_cap, rows.shape[1])
    assert np.array_equal(nout, want_nout), (nout, want_nout)
    assert_same(rows, want_rows)
    return rows, nout


# ---------------------------------------------------------------------------
# 1: kinds and sizes
# ---------------------------------------------------------------------------
# outputs per full row: more than two of the kernel's chunks (2048 / 1024 / 64 / 32 outputs by K)
M_TARGET = {1: 4500, 2: 2300, 3: 2300, 63: 150, 64: 150, 65: 80, 130: 80}


def size_cases():
    return [pytest.param(*c, id="%s-T%d-D%d-K%d-P%d" % c) for c in Iq.size_cases()]


def sized_case(M, name, T, D, K, P):
    """the inputs of one case of Iq.size_cases(): two rows of n elements -> (kind, taps, centres, x, lens)"""
    kind = Iq.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + D)
    vec = vec_of(kind)
    n = min(40000, T + (M_TARGET[K] - 1) * D + 3)
    n = (n + vec - 1) // vec * vec
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
    return kind, taps, Iq.centres_of(rng, K, P), Iq.random_rows(rng, kind, 2, n), [n, n - (n // 3)]


@pytest.mark.parametrize("name,T,D,K,P", size_cases())
def test_kinds_and_sizes(gpu, name, T, D, K, P):
    kind, taps, centres, x, lens = sized_case(gpu[0], name, T, D, K, P)
    assert x.shape[1] <= 40000
    for r in (0, int(centres[-1])):             # r = 0 and r = q (of the last channel)
        check(gpu, x, kind, P, taps, D, centres, r, lens=lens)


# ---------------------------------------------------------------------------
# 2: ragged rows and capacity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Iq.KINDS))
def test_ragged_rows_and_capacity(gpu, name):
    M = gpu[0]
    kind = Iq.KINDS[name]
    rng = np.random.default_rng(7)
    T, D, P = 65, 4, 4800
    vec = vec_of(kind)
    n = 2400 // vec * vec
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0)
    centres = np.array([117, -60, 2400], np.int32)
    lens = [0, T - 1, T, T + D - 1, T + D, n]
    x = Iq.random_rows(rng, kind, len(lens), n)
    full = (n - T) // D + 1
    plan = make_plan(gpu, kind, P, taps, D, centres, 117)
    for nout_cap, out_stride in ((None, None), (full - 37, even(full)), (1, 2), (0, 2), (full + 9, even(full + 9) + 2)):
        rows, nout = check(gpu, x, kind, P, taps, D, centres, 117, lens=lens, nout_cap=nout_cap,
                           out_stride=out_stride, plan=plan)
        assert rows.shape[1] == (even(full) if out_stride is None else out_stride)
        cap = rows.shape[1] if nout_cap is None else nout_cap
        want = [min(cap, c) for c in (0, 0, 1, 1, 2, full)]
        assert list(nout.reshape(len(lens), 3)[:, 0]) == want
        for i, c in enumerate(nout):
            assert not np.any(rows[i, c:].view(np.uint32)), "the tail of row %d is not (+0.0f, +0.0f)" % i
    # lengths beyond the stride are clamped to it
    check(gpu, x, kind, P, taps, D, centres, 117, lens=[n + 1000] * len(lens), plan=plan)
    plan.close()


# ---------------------------------------------------------------------------
# 3: the I plane is the real entry's output
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real-f32", "complex-s16"])
def test_the_i_plane_equals_the_real_entry(gpu, name):
    """one plan, one input, both entries: rows_iq[..., 0] == rows_real bit for bit (the K = 3 case of test 1)"""
    M, torch, _ctx = gpu
    case = [c for c in Iq.size_cases() if c[0] == name and c[3] == 3][0]
    kind, taps, centres, x, lens = sized_case(M, *case)
    _name, _T, D, _K, P = case
    plan = make_plan(gpu, kind, P, taps, D, centres, int(centres[-1]))
    d = torch.from_numpy(x).cuda()
    dl = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    real = M.channelize(plan, d, nsamples=dl)
    stride = real["rows"].shape[1]
    iq, nout = channelize_iq(gpu, plan, d, lens=lens, out_stride=stride)
    plan.close()
    real_rows = real["rows"].cpu().numpy()
    assert real_rows.shape == (6, stride) and iq.shape == (6, stride, 2)
    assert np.array_equal(nout, real["nsamples"].cpu().numpy()) and nout.min() > 1000
    assert_same(np.ascontiguousarray(iq[..., 0]), real_rows)
    assert np.any(iq[..., 1])


# ---------------------------------------------------------------------------
# 4: special values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [False, True])
def test_special_values(gpu, cx):
    M = gpu[0]
    kind = Iq.COMPLEX if cx else 0
    rng = np.random.default_rng(9)
    T, D, P, n = 64, 7, 65536, 4000
    taps = M.channel_taps(T, 3000.0, 48000.0, 2.0)
    centres = np.array([0, 1000, -20000, P // 2], np.int32)
    x = Iq.random_rows(rng, kind, 5, n)
    flat = x.reshape(5, -1)
    flat[0, 300:1500] = 0.0                                   # windows of zeros
    flat[0, 2000:2600] = -0.0
    flat[1, :] = (rng.integers(1, 1 << 22, flat.shape[1]).astype(np.uint32)).view(F32)     # subnormals
    flat[1, ::2] *= -1.0
    flat[2, :] *= F32(1e30)
    flat[3, 1111], flat[3, 2999] = np.inf, -np.inf
    flat[4, 2222] = np.nan
    rows, _nout = check(gpu, x, kind, P, taps, D, centres, 1000)
    for plane in (0, 1):
        p = rows[..., plane]
        assert np.isnan(p[16:20]).any() and not np.isnan(p[16:20]).all()       # the NaN stays inside its windows
        assert (np.isinf(p[12:16]) | np.isnan(p[12:16])).any() and np.isfinite(p[12:16]).any()
        assert not np.any(p[0:4, 50:95].view(np.uint32) & 0x7FFFFFFF)         # zeros in, zeros out


# ---------------------------------------------------------------------------
# 5: refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Iq.KINDS))
def test_what_the_entry_refuses_of_the_io(gpu, name):
    """with a plan of each kind and real arrays: every refusal comes back in the header's order, and after each
    one both outputs and their guard cells hold what they held"""
    M, torch, _ctx = gpu
    lib = _lib.load()
    kind = Iq.KINDS[name]
    vec = vec_of(kind)
    plan = make_plan(gpu, kind, 4800, M.channel_taps(65, 400.0, 48000.0, 2.0), 4, [117, -60], 117)
    n, out_stride = 50 * vec, 64
    d = torch.from_numpy(Iq.random_rows(np.random.default_rng(3), kind, 2, n)).cuda()
    fr, fn, out = guarded(torch, 4, out_stride, d.device)
    before = (fr.cpu().numpy().copy(), fn.cpu().numpy().copy())
    samples, rows, nout = d.data_ptr(), out["rows"].data_ptr(), out["nsamples"].data_ptr()
    assert samples % 16 == 0 and rows % 16 == 0

    def rc(ctx=plan.handle, **kw):
        io = _lib.ChannelIO()
        io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
        io.d_rows, io.out_stride, io.nout_cap, io.d_nout = rows, out_stride, out_stride, nout
        for k, v in kw.items():
            setattr(io, k, v)
        got = lib.mifsk_channelize_iq_batch(ctx, C.byref(io), None)
        torch.cuda.synchronize()
        assert np.array_equal(fr.cpu().numpy(), before[0]) and np.array_equal(fn.cpu().numpy(), before[1]), kw
        return got

    assert lib.mifsk_channelize_iq_batch(plan.handle, None, None) == EINVAL
    for field in ("d_samples", "d_rows", "d_nout"):
        assert rc(**{field: None}) == EINVAL, field
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-1) == EINVAL
    for off in (2, 4, 8):
        assert rc(d_samples=samples + off) == EINVAL, off
    for stride in range(n + 1, n + vec):                        # not a whole number of 16-byte vectors
        assert rc(stream_stride=stride) == EINVAL, stride
    for off in (4, 8, 12):                                      # 8: a whole element, not 16 bytes
        assert rc(d_rows=rows + off) == EINVAL, off
    for stride in (0, 1, 63, 65, 1 << 31, (1 << 31) + 2, 1 << 32, 1 << 40):   # none, odd, above 2^31 - 2
        assert rc(out_stride=stride, nout_cap=0) == EINVAL, stride
    assert rc(out_stride=(1 << 31) - 1, nout_cap=0) == EINVAL
    assert rc(nout_cap=out_stride + 1) == EINVAL and rc(nout_cap=0xFFFFFFFF) == EINVAL
    assert rc(nstreams=(1 << 30) + 1) == EINVAL                 # nstreams * nchannels
    ladder(rc, dict(nstreams=(1 << 30) + 1),
           [dict(d_nout=None), dict(nstreams=0), dict(d_samples=samples + 8), dict(stream_stride=n + vec - 1),
            dict(d_rows=rows + 8), dict(out_stride=0, nout_cap=0), dict(out_stride=63, nout_cap=0),
            dict(out_stride=1 << 31, nout_cap=0), dict(nout_cap=out_stride + 1)])
    # what passes the checks runs: the same io, nothing replaced
    io = _lib.ChannelIO()
    io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = samples, n, None, n, 2
    io.d_rows, io.out_stride, io.nout_cap, io.d_nout = rows, out_stride, out_stride, nout
    assert lib.mifsk_channelize_iq_batch(plan.handle, C.byref(io), None) == 0
    torch.cuda.synchronize()
    plan.close()
    cnt = (n - 65) // 4 + 1 if n >= 65 else 0
    assert np.all(out["nsamples"].cpu().numpy() == min(cnt, out_stride))
    got = fr.cpu().numpy()
    assert np.all(got[:GUARD] == ROW_GUARD) and np.all(got[-GUARD:] == ROW_GUARD)


# ---------------------------------------------------------------------------
# 6: more rows than one launch takes (65 535, the grid's y limit): the row-block loop
# ---------------------------------------------------------------------------
def test_a_batch_of_more_rows_than_one_launch_takes(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(65537)
    nrows, n, cut = 65537, 16, 40000
    x = rng.standard_normal((nrows, n)).astype(F32)
    P, taps, D, centres, r = 7, np.array([0.75, -0.5], F32), 1, np.array([3], np.int32), 1
    plan = make_plan(gpu, 0, P, taps, D, centres, r)
    d = torch.from_numpy(x).cuda()
    whole = M.channelize(plan, d, iq=True)
    parts = [M.channelize(plan, d[:cut], iq=True), M.channelize(plan, d[cut:], iq=True)]
    torch.cuda.synchronize()
    plan.close()
    rows, nout = whole["rows"].cpu().numpy(), whole["nsamples"].cpu().numpy()
    assert rows.shape == (nrows, 16, 2) and np.all(nout == n - 1)
    assert Iq.same_f32(rows, np.concatenate([p["rows"].cpu().numpy() for p in parts]))
    assert np.array_equal(nout, np.concatenate([p["nsamples"].cpu().numpy() for p in parts]))
    for s in (0, 65534, 65535, 65536):
        want = Iq.ref_channelize_iq(x[s], 0, P, taps, D, centres, r)
        assert want.shape == (1, n - 1, 2) and Iq.same_f32(rows[s, :n - 1], want[0]), s
        assert not np.any(rows[s, n - 1].view(np.uint32)), s


# ---------------------------------------------------------------------------
# 7: the Python surface
# ---------------------------------------------------------------------------
def test_the_python_surface(gpu):
    M, torch, _ctx = gpu
    rng = np.random.default_rng(64)
    T, D, P, n = 63, 4, 4800, 2002
    full = (n - T) // D + 1
    assert full % 2 == 1                                        # the default stride rounds up to even
    ta, ca = M.channel_taps(T, 400.0, 48000.0, 1.0), np.array([-300, 30], np.int32)
    x = Iq.random_rows(rng, Iq.COMPLEX, 2, n)
    pa = make_plan(gpu, Iq.COMPLEX, P, ta, D, ca, 0)
    a = M.channelize(pa, torch.from_numpy(x).cuda(), iq=True)
    b = M.channelize(pa, torch.view_as_complex(torch.from_numpy(x).cuda()), iq=True)
    one = M.channelize(pa, torch.from_numpy(x[1]).cuda(), iq=True)
    capped = M.channelize(pa, torch.from_numpy(x).cuda(), nout_cap=1, iq=True)
    torch.cuda.synchronize()
    assert a["rows"].dtype == torch.float32 and a["nsamples"].dtype == torch.int32
    assert a["rows"].shape == (4, full + 1, 2) and a["nsamples"].shape == (4,) and a["rows"].is_contiguous()
    assert capped["rows"].shape == (4, 2, 2) and np.all(capped["nsamples"].cpu().numpy() == 1)
    want, wn = expect(x, Iq.COMPLEX, P, ta, D, ca, 0, None, None, full + 1)
    assert_same(a["rows"].cpu().numpy(), want)
    assert_same(b["rows"].cpu().numpy(), want)
    assert_same(one["rows"].cpu().numpy(), want[2:])
    assert np.array_equal(a["nsamples"].cpu().numpy(), wn) and np.array_equal(b["nsamples"].cpu().numpy(), wn)
    # the default path is the real entry's, as before
    real = M.channelize(pa, torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert real["rows"].shape == (4, (full + 3) // 4 * 4)
    assert_same(real["rows"].cpu().numpy()[:, :full], np.ascontiguousarray(want[:, :full, 0]))
    # out= of the stated shape is honoured, and only that shape
    x2 = Iq.random_rows(rng, Iq.COMPLEX, 2, n)
    short = [n, 700]
    again = M.channelize(pa, torch.from_numpy(x2).cuda(), nsamples=torch.from_numpy(np.array(short, np.int32)).cuda(),
                         out=a, iq=True)
    torch.cuda.synchronize()
    assert again is a
    want2, wn2 = expect(x2, Iq.COMPLEX, P, ta, D, ca, 0, short, None, full + 1)
    assert_same(a["rows"].cpu().numpy(), want2)
    assert np.array_equal(a["nsamples"].cpu().numpy(), wn2)
    with pytest.raises(AssertionError):
        M.channelize(pa, torch.from_numpy(x).cuda(), out=real, iq=True)         # real rows are not I/Q rows
    with pytest.raises(AssertionError):
        M.channelize(pa, torch.from_numpy(x).cuda(), out=a)                     # ... nor the other way round
    # two plans on two streams at once give what each gives alone
    tb, cb = M.channel_taps(385, 300.0, 48000.0, 2.0), Iq.centres_of(rng, 65, P)
    y = Iq.random_rows(rng, 0, 3, 3000)
    pb = make_plan(gpu, 0, P, tb, 7, cb, 5)
    alone_a, alone_b = channelize_iq(gpu, pa, x), channelize_iq(gpu, pb, y)
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    both_a = M.channelize(pa, dx, stream=sa, iq=True)
    both_b = M.channelize(pb, dy, stream=sb, iq=True)
    sa.synchronize()
    sb.synchronize()
    assert_same(both_a["rows"].cpu().numpy(), alone_a[0])
    assert_same(both_b["rows"].cpu().numpy(), alone_b[0])
    assert np.array_equal(both_a["nsamples"].cpu().numpy(), alone_a[1])
    assert np.array_equal(both_b["nsamples"].cpu().numpy(), alone_b[1])
    want_b, wn_b = expect(y, 0, P, tb, 7, cb, 5, None, None, alone_b[0].shape[1])
    assert_same(alone_b[0], want_b)
    assert np.array_equal(alone_b[1], wn_b)
    pa.close()
    pb.close()


# ---------------------------------------------------------------------------
# end to end: three FM channels of one capture decode on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cnr_db", [None, 14.0], ids=["clean", "cnr14"])
def test_three_fm_channels_of_one_capture_decode_on_the_device(gpu, cnr_db):
    """Three Bell-202 messages, each FM-modulated at its own centre of a 192 kHz complex capture (fm_modulate's
    `centre`), summed in float32 and impaired: channelize(iq=True) with out_centre 0 -> fm_demod -> demod_batch.
    The transmitted audio goes to the host, the restatements make every stage there (fm_ref.c, float32 sum,
    impair_ref.c, channel_ref_iq, fm_ref.c) and the oracle decodes the three audio rows to exactly their 16 bytes
    BEFORE anything of the device's is looked at.  Then the device's capture, I/Q rows, audio rows and lengths
    equal the host's bit for bit, its frames, bytes and episodes the oracle's, and its bytes the messages."""
    M, torch, ctx = gpu
    words = Iq.fm_messages()
    tx_cfg, cfg, ocfg = M.rx_config("1200", sample_rate=Iq.FS), M.rx_config("1200"), O.oracle_config("1200")
    lead = torch.from_numpy(np.array(Iq.LEAD, np.int32)).cuda()
    clean, lens = M.synthesize_batch(ctx, tx_cfg, torch.from_numpy(words).cuda(), amplitude=1.0, leading_silence=lead)
    n = clean.shape[1]
    assert n % 4 == 0 and n <= 40000
    sigma = Iq.fm_sigma(M, cnr_db)
    gain = M.fm_gain(Iq.FS / Iq.D_FM, Iq.DEVIATION_HZ)

    host = Iq.fm_host_chain(M, clean.cpu().numpy(), lens.cpu().numpy().astype(np.uint32), sigma)
    nout = host["nout"]
    assert nout == (n - Iq.NTAPS) // Iq.D_FM + 1 and nout % 4 == 0
    for k in range(3):                                          # the precondition: the oracle has every message whole
        assert O.oracle_rx_stream(ocfg, host["audio"][k, :nout])["bytes"] == words[k].tobytes(), k

    dev = M.fm_step(Iq.DEVIATION_HZ, Iq.FS)
    rows = [M.fm_modulate(ctx, clean[k:k + 1], nsamples=lens[k:k + 1], deviation=dev, centre=M.fm_step(off, Iq.FS),
                          amplitude=Iq.CARRIER) for k, off in enumerate(Iq.OFFSETS)]
    capture = (rows[0] + rows[1]) + rows[2]                     # float32, in channel order
    noisy = M.impair(ctx, capture.view(1, 2 * n), seed=Iq.SEED, sigma=sigma).view(1, n, 2)
    plan = M.ChannelPlan(ctx, host["taps"], Iq.D_FM, Iq.CENTRES, 0, Iq.P_FM, complex_input=True)
    ch = M.channelize(plan, noisy, iq=True)
    audio = M.fm_demod(ctx, ch["rows"], nsamples=ch["nsamples"], gain=gain)
    out = M.demod_batch(ctx, cfg, audio, nsamples=ch["nsamples"], want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    plan.close()
    assert Iq.same_f32(capture.cpu().numpy()[0], host["capture"])
    assert Iq.same_f32(noisy.cpu().numpy()[0], host["noisy"])
    got_iq, got_n = ch["rows"].cpu().numpy(), ch["nsamples"].cpu().numpy()
    assert got_iq.shape == (3, nout, 2) and np.array_equal(got_n, np.full(3, nout, np.int32))
    assert_same(got_iq, host["iq"])
    got_audio = audio.cpu().numpy()
    assert got_audio.shape == host["audio"].shape and Iq.same_f32(got_audio, host["audio"])
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, host["audio"], got_n.astype(np.uint32), res, threads=3)
    assert bad == []
    for k in range(3):
        assert res["bytes"][k, :int(res["nbytes"][k])].tobytes() == words[k].tobytes(), k
