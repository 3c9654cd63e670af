"""Every wrapper that takes a batch of rows, on torch's current stream and on a side stream: the outputs
are equal bit for bit.  The outputs of a launch on a side stream are allocated (and filled) on that
stream and marked as used on the current one, so that dropping them at once and allocating again on
the current stream cannot hand their memory out under the kernel -- ingest_s16 and synthesize_batch
included, which once allocated on the current stream and did not mark theirs.

Shapes: 3 rows of lengths 0, 5 and the width, the width the smallest whole number of 16-byte vectors
that holds one frame, window or tap set of the entry."""
import numpy as np
import pytest

import minimodem_amd as M

LENS = (0, 5)          # ... and the width


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU: the batch entries have no CPU fallback")
    return torch, M.Context(0)


@pytest.fixture(scope="module")
def cfg():
    return M.rx_config("4800")          # 10 samples per bit: a frame and its leader within 256 samples


@pytest.fixture(scope="module")
def signal(gpu, cfg):
    """(one transmitted word per row [3, width], the lengths 0, 5, width, demod_batch's result for them)"""
    torch, ctx = gpu
    words = torch.tensor([[0x55], [0x41], [0x5A]], dtype=torch.uint8, device="cuda")
    x, _n = M.synthesize_batch(ctx, cfg, words)
    assert 64 <= x.shape[1] <= 256 and x.shape[1] % 4 == 0
    lens = lengths(torch, x.shape[1])
    res = M.demod_batch(ctx, cfg, x, nsamples=lens, want=("bytes", "bits", "frames", "episodes"))
    torch.cuda.synchronize()
    assert int(res["nframes"][2]) >= 1
    return x, lens, res


def lengths(torch, width, rows=3):
    return torch.tensor((LENS + (width,) * rows)[:rows], dtype=torch.int32, device="cuda")


def rows_f32(torch, shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)).cuda()


def rows_s16(torch, shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-32768, 32768, shape, dtype=np.int16)).cuda()


def tensors(torch, res):
    """the tensors (or arrays) of a wrapper's result, by name"""
    if isinstance(res, dict):
        return {k: v for k, v in res.items() if torch.is_tensor(v) or isinstance(v, np.ndarray)}
    return dict(enumerate(res if isinstance(res, (tuple, list)) else (res,)))


def raw(t):
    return (t if isinstance(t, np.ndarray) else t.cpu().numpy()).tobytes()


def on_both_streams(torch, call):
    """call(stream) makes its inputs on the current stream and returns the wrapper's result for `stream`"""
    want = {k: raw(t) for k, t in tensors(torch, call(None)).items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = tensors(torch, call(side))
    shapes = {k: (tuple(t.shape), t.dtype) for k, t in res.items() if torch.is_tensor(t)}
    with torch.cuda.stream(side):
        kept = {k: t.clone() if torch.is_tensor(t) else t for k, t in res.items()}      # behind the kernel
    del res
    # the outputs are dropped while the side stream may still run: memory of the same size, asked for
    # on the current stream and filled there, must not be theirs
    again = [torch.full(shape, 85, dtype=dtype, device="cuda") for shape, dtype in shapes.values()]
    side.synchronize()
    torch.cuda.synchronize()
    del again
    assert sorted(kept) == sorted(want)
    for k, t in kept.items():
        assert raw(t) == want[k], "%s differs between the current stream and a side stream" % k


def ready(torch, stream):
    """the inputs were made on the current stream: a side stream starts behind it"""
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())


@pytest.mark.gpu
def test_synthesize_batch(gpu, cfg):
    torch, ctx = gpu

    def call(stream):
        words = torch.from_numpy(np.arange(24, dtype=np.uint8).reshape(3, 8) + 0x40).cuda()
        nwords = lengths(torch, 8)
        ready(torch, stream)
        return M.synthesize_batch(ctx, cfg, words, nwords=nwords, stride=1024, stream=stream)
    on_both_streams(torch, call)


@pytest.mark.gpu
def test_demod_batch(gpu, cfg, signal):
    torch, ctx = gpu
    x, lens, _res = signal
    on_both_streams(torch, lambda stream: M.demod_batch(ctx, cfg, x, nsamples=lens, stream=stream,
                                                        want=("bytes", "bits", "frames", "episodes")))


@pytest.mark.gpu
def test_frame_softbits(gpu, cfg, signal):
    torch, ctx = gpu
    x, lens, res = signal
    on_both_streams(torch, lambda stream: M.frame_softbits(ctx, cfg, x, res, nsamples=lens, stream=stream))


@pytest.mark.gpu
def test_carrier_survey(gpu, cfg, signal):
    torch, ctx = gpu
    x, lens, _res = signal
    on_both_streams(torch, lambda stream: M.carrier_survey(ctx, cfg, x, nsamples=lens, spectrum=True, stream=stream))


@pytest.mark.gpu
def test_slab_session_feed(gpu, cfg, signal):
    torch, ctx = gpu
    x = signal[0].cpu().numpy()
    new = [x[0, :0], x[1, :5], x[2]]
    on_both_streams(torch, lambda stream: M.SlabSession(ctx, cfg, 3).feed(new, final=True, stream=stream))


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True])
def test_channelize_complex_rows(gpu, s16):
    torch, ctx = gpu
    plan = M.ChannelPlan(ctx, M.channel_taps(64, 1200.0, 48000.0), 4, [-3, 5], 1, 64, complex_input=True, s16=s16)
    iq = (rows_s16 if s16 else rows_f32)(torch, (3, 64, 2), 11)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.channelize(plan, iq, nsamples=lens, stream=stream))


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True])
def test_multiplex_to_complex_rows(gpu, s16):
    torch, ctx = gpu
    plan = M.MuxPlan(ctx, M.channel_taps(64, 1200.0, 48000.0, 8.0), 4, [5], 1, 64, complex_output=True, s16=s16)
    x = rows_f32(torch, (3, 64), 12)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.multiplex(plan, x, nsamples=lens, stream=stream))


@pytest.mark.gpu
def test_impair(gpu):
    torch, ctx = gpu
    x = rows_f32(torch, (3, 64), 13)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.impair(ctx, x, nsamples=lens, seed=3, sigma=0.1, gain=0.5, dc=0.01,
                                                   stream=stream))


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True])
def test_fm_demod(gpu, s16):
    torch, ctx = gpu
    iq = (rows_s16 if s16 else rows_f32)(torch, (3, 64, 2), 14)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.fm_demod(ctx, iq, nsamples=lens, gain=2.0, stream=stream))


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [False, True])
def test_fm_modulate(gpu, s16):
    torch, ctx = gpu
    x = rows_f32(torch, (3, 64), 15)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.fm_modulate(ctx, x, nsamples=lens, deviation=0.01, centre=0.002, s16=s16,
                                                        stream=stream))


@pytest.mark.gpu
def test_ingest_s16(gpu):
    torch, ctx = gpu
    pcm = rows_s16(torch, (3, 64), 16)
    lens = lengths(torch, 64)
    on_both_streams(torch, lambda stream: M.ingest_s16(ctx, pcm, nsamples=lens, rxnoise=0.25, stream=stream))


@pytest.mark.gpu
def test_ingest_rxnoise(gpu):
    torch, ctx = gpu

    def call(stream):
        x = rows_f32(torch, (3, 64), 17)             # (in place: new rows for every call)
        lens = lengths(torch, 64)
        ready(torch, stream)
        return M.ingest_rxnoise(ctx, x, 0.25, nsamples=lens, stream=stream)
    on_both_streams(torch, call)
