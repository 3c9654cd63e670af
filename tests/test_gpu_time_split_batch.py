"""A small batch of long recordings decoded across the chip by cutting all of them in time with
one plan (mifsk_demod_long_batch; DESIGN.md "cutting a stream in time", "Several recordings").
The yardstick everywhere is ONE demod_batch call over the same batch, compared per stream and bit
for bit: frames (f32 patterns included), bits, bytes, episodes (their float totals included),
counts, status and the --auto-carrier band.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import _golden as G
from test_gpu_time_split import WANT, _bursty, _lattice, _recording

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _upload(torch, streams):
    lens = [len(x) for x in streams]
    host = np.zeros((len(streams), max(4, (max(lens) + 3) & ~3)), np.float32)
    for i, x in enumerate(streams):
        host[i, :len(x)] = x
    return torch.from_numpy(host).cuda(), lens


def _one_call(M, torch, ctx, cfg, d, lens, engine=None):
    dn = torch.tensor(lens, dtype=torch.int32, device="cuda")
    band = ("carrier_band",) if cfg.auto_carrier_threshold > 0 else ()
    out = M.demod_batch(ctx, cfg, d, nsamples=dn, want=WANT + band,
                        episodes_cap=M.max_episodes(cfg, max(lens)), engine=engine)
    torch.cuda.synchronize()
    return M.results_to_host(out)


def _split(M, ctx, cfg, d, lens, **kw):
    out = M.demod_long_batch(ctx, cfg, d, nsamples=lens, want=WANT, **kw)
    stats = out.pop("stats")
    return M.results_to_host(out), stats


def _same(a, i, b, j, cfg, what):
    """stream i of `a` is stream j of `b`, as test_gpu_time_split._same compares"""
    nf = int(a["nframes"][i])
    assert nf == int(b["nframes"][j]), what
    assert a["frames"][i, :nf].tobytes() == b["frames"][j, :nf].tobytes(), what
    assert a["bits"][i, :nf].tobytes() == b["bits"][j, :nf].tobytes(), what
    nb = int(a["nbytes"][i])
    assert nb == int(b["nbytes"][j]) and a["bytes"][i, :nb].tobytes() == b["bytes"][j, :nb].tobytes(), what
    ne = int(a["nepisodes"][i])
    assert ne == int(b["nepisodes"][j]), what
    assert a["episodes"][i, :ne].tobytes() == b["episodes"][j, :ne].tobytes(), what
    assert int(a["status"][i]) == int(b["status"][j]), what
    if cfg.auto_carrier_threshold > 0:
        assert int(a["carrier_band"][i]) == int(b["carrier_band"][j]), what
    return nf


UNEQUAL = ["t01_1200", "t03_rtty", "t40_rxnoise_0p05_rxone", "t50_auto_300", "t70_callerid_mdmf",
           "t80_same", "t81_tdd"]

_cases = {}


def _unequal(M, torch, ctx, name, engine):
    """Five unequal streams of one golden (1, 2, 3 and 5 copies, and one shorter than W, which
    stays whole beside the cut ones), the forced small chunk, and the one call over them --
    made once per (golden, engine) and left unchanged."""
    key = (name, engine)
    if key not in _cases:
        g = G.load(name)
        cfg = M.rx_config(**g["cfg_kwargs"])
        W = 2 * cfg.samplebuf_size
        seed = zlib.crc32(name.encode())
        streams = [_recording(g["samples"], np.random.default_rng(seed + c), copies=c, sample_rate=cfg.sample_rate)
                   for c in (1, 2, 3, 5)]
        streams.insert(2, streams[0][:W - 7].copy())
        lat = _lattice(cfg)
        L = lat * max(1, (max(len(x) for x in streams) // 12) // lat)
        d, lens = _upload(torch, streams)
        _cases[key] = (cfg, d, lens, L, W, _one_call(M, torch, ctx, cfg, d, lens, engine=engine))
    return _cases[key]


@pytest.mark.parametrize("name", UNEQUAL)
@pytest.mark.parametrize("engine", [None, "wave", "workgroup"])
def test_unequal_streams_cut_small_equal_one_call(gpu, name, engine):
    M, torch, ctx = gpu
    if engine == "workgroup" and G.load(name)["cfg_kwargs"].get("auto_carrier_threshold", 0) > 0:
        pytest.skip("the workgroup engine has no in-loop --auto-carrier")
    cfg, d, lens, L, W, want = _unequal(M, torch, ctx, name, engine)
    got, st = _split(M, ctx, cfg, d, lens, chunk=L, warmup=W, engine=engine)
    assert [s["nsamples"] for s in st] == lens
    assert all(s["chunk"] == L and s["warmup"] == W for s in st)
    assert [s["nchunks"] for s in st] == [(n - W) // L + 1 if n > W else 1 for n in lens]
    assert sum(s["nchunks"] >= 2 for s in st) >= 3 and st[2]["nchunks"] == 1, st
    for i in range(len(lens)):
        _same(got, i, want, i, cfg, (name, engine, i, st[i]))
        assert st[i]["accepted"] <= st[i]["nchunks"] - 1 and st[i]["rounds"] <= max(0, st[i]["nchunks"] - 1)


@pytest.mark.parametrize("name", UNEQUAL)
def test_reversed_order_of_streams_gives_reversed_outputs(gpu, name):
    M, torch, ctx = gpu
    cfg, d, lens, L, W, want = _unequal(M, torch, ctx, name, None)
    got, st = _split(M, ctx, cfg, d.flip(0).contiguous(), lens[::-1], chunk=L, warmup=W)
    n = len(lens)
    assert [s["nsamples"] for s in st] == lens[::-1]
    for i in range(n):
        _same(got, i, want, n - 1 - i, cfg, (name, i, st[i]))


@pytest.mark.parametrize("name", ["t01_1200", "t03_rtty", "t40_rxnoise_0p05_rxone", "t80_same"])
def test_reject_all_reruns_every_chunk_of_every_stream_in_parallel(gpu, name):
    M, torch, ctx = gpu
    g = G.load(name)
    cfg = M.rx_config(**g["cfg_kwargs"])
    streams = [_recording(g["samples"], np.random.default_rng(7 + c), copies=c, sample_rate=cfg.sample_rate)
               for c in (1, 2, 3, 5)]
    lat = _lattice(cfg)
    L = lat * max(1, (max(len(x) for x in streams) // 10) // lat)
    d, lens = _upload(torch, streams)
    got, st = _split(M, ctx, cfg, d, lens, chunk=L, warmup=2 * cfg.samplebuf_size, reject_all=True)
    want = _one_call(M, torch, ctx, cfg, d, lens)
    for i in range(len(lens)):
        _same(got, i, want, i, cfg, (name, i, st[i]))
        assert st[i]["accepted"] == 0, st[i]
        if cfg.rx_one == 0:
            # every chunk went through the re-run path at least once
            assert st[i]["rerun"] >= st[i]["nchunks"] - 1, st[i]
    assert sum(s["nchunks"] >= 2 for s in st) >= 3, st
    # Verification is per stream: what a stream's guesses met with does not depend on its
    # neighbours, so its accepted / re-run / rounds figures are those of the stream decoded alone
    # with the same cut.
    for i, n in enumerate(lens):
        alone = M.demod_long(ctx, cfg, d[i, :n], want=("bytes",), chunk=L, warmup=2 * cfg.samplebuf_size,
                             reject_all=True)["stats"]
        if st[i]["nchunks"] >= 2:
            assert st[i] == alone, (name, i, st[i], alone)
        else:
            assert alone["nchunks"] == 1 and st[i]["rerun"] == st[i]["rounds"] == 0, (name, i, st[i], alone)
    # The stats carry no round count of the call.  A stream has a row re-run in every round until
    # it is settled, so the call's rounds are the largest per-stream figure, and the bound below
    # is structural only: it holds by the definition of the per-stream count.
    rounds = max(s["rounds"] for s in st)
    assert rounds <= max(s["nchunks"] - 1 for s in st), st
    if cfg.rx_one == 0:
        assert rounds >= 1
        assert all(1 <= s["rounds"] <= s["nchunks"] - 1 for s in st if s["nchunks"] >= 2), st


@pytest.mark.parametrize("engine", [None, "wave", "workgroup"])
def test_empty_and_tiny_streams_beside_cut_ones(gpu, engine):
    """A stream of no samples and one of three samples are rows of the flat batch like any other:
    a row of length 0, and a final slab of 0 samples for the tail."""
    M, torch, ctx = gpu
    g = G.load("t01_1200")
    cfg = M.rx_config(**g["cfg_kwargs"])
    rec = [_recording(g["samples"], np.random.default_rng(31 + c), copies=c, sample_rate=cfg.sample_rate)
           for c in (2, 3)]
    streams = [np.zeros(0, np.float32), rec[0], rec[1][:3].copy(), rec[1], np.zeros(0, np.float32)]
    lat = _lattice(cfg)
    W = 2 * cfg.samplebuf_size
    L = lat * max(1, (len(rec[1]) // 12) // lat)
    d, lens = _upload(torch, streams)
    got, st = _split(M, ctx, cfg, d, lens, chunk=L, warmup=W, engine=engine)
    want = _one_call(M, torch, ctx, cfg, d, lens, engine=engine)
    assert [s["nchunks"] >= 2 for s in st] == [False, True, False, True, False], st
    for i in range(len(lens)):
        _same(got, i, want, i, cfg, (engine, i, st[i]))
    assert int(got["nframes"][0]) == 0 and int(got["nframes"][4]) == 0 and int(got["nframes"][3]) > 0


def test_error_codes_of_the_call(gpu):
    """What the planner cannot refuse: the row layout, and the workgroup engine with --auto-carrier."""
    import ctypes as C
    from minimodem_amd import _lib
    M, torch, ctx = gpu
    lib = _lib.load()
    cfg = M.rx_config("1200")
    d = torch.zeros((2, 96000), dtype=torch.float32, device="cuda")
    nf = torch.zeros(2, dtype=torch.int32, device="cuda")
    io = _lib.DemodIO()
    io.nstreams = 2
    io.d_nframes = nf.data_ptr()

    def rc(cfg, stride, lens, nstreams=2, engine=None, ptr=None):
        arr = (C.c_uint64 * len(lens))(*lens) if lens is not None else None
        p = M._time_split_params(None, None, None, engine, False)
        return lib.mifsk_demod_long_batch(ctx.handle, C.byref(cfg), C.c_void_p(d.data_ptr() if ptr is None else ptr),
                                          stride, arr, nstreams, C.byref(p), C.byref(io), None, None)

    assert rc(cfg, 95998, [5000, 5000]) == -22                  # stream_stride % 4
    assert rc(cfg, 96000, [96001, 5000]) == -22                 # a stream longer than its row
    assert rc(cfg, 96000, [5000, 5000], nstreams=0) == -22
    assert rc(cfg, 96000, None) == -22                          # no lengths
    assert rc(cfg, 96000, [5000, 5000], ptr=d.data_ptr() + 4) == -22    # not 16-byte aligned
    auto = M.rx_config(**G.load("t50_auto_300")["cfg_kwargs"])
    assert auto.auto_carrier_threshold > 0
    assert rc(auto, 96000, [96000, 5000], engine="workgroup") == -22
    with pytest.raises(RuntimeError):
        M.demod_long_batch(ctx, auto, d, engine="workgroup")
    # the same calls, well formed, are accepted
    for c, engine in ((cfg, "workgroup"), (auto, "wave")):
        out = M.demod_long_batch(ctx, c, d, nsamples=[96000, 5000], engine=engine)
        assert [s["nchunks"] for s in out["stats"]] == [1, 1] and int(out["nframes"].sum()) == 0
    torch.cuda.synchronize()


def test_one_stream_is_demod_long(gpu):
    M, torch, ctx = gpu
    g = G.load("t01_1200")
    cfg = M.rx_config(**g["cfg_kwargs"])
    x = _recording(g["samples"], np.random.default_rng(21), copies=3, sample_rate=cfg.sample_rate)
    x = x[:len(x) - (len(x) % 4) - 1]                  # not a multiple of 4: the padded-copy path too
    d, lens = _upload(torch, [x])
    lat = _lattice(cfg)
    for kw in ({"chunk": lat * max(1, (len(x) // 9) // lat), "warmup": 2 * cfg.samplebuf_size},
               {"chunk": lat * max(1, (len(x) // 9) // lat), "warmup": 2 * cfg.samplebuf_size, "reject_all": True},
               {"chunks": 7, "warmup": 2 * cfg.samplebuf_size + lat, "engine": "wave"},
               {}):
        got, st = _split(M, ctx, cfg, d, lens, **kw)
        out = M.demod_long(ctx, cfg, d[0, :len(x)], want=WANT, **kw)
        st1 = out.pop("stats")
        _same(got, 0, M.results_to_host(out), 0, cfg, kw)
        assert st == [st1], kw
        assert (st1["nchunks"] >= 2) == bool(kw), (kw, st1)      # (the library's choice: the single call)


@pytest.fixture(scope="module")
def bursts_1200(gpu):
    """two 5-minute Bell-202 recordings of bursts at 20 dB; the streams below are rolled and
    truncated copies of them, which keeps host generation to a few seconds"""
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    return cfg, [_bursty(M, cfg, 300, np.random.default_rng(100 + i), snr_db=20) for i in range(2)]


def _rolled(recs, count, seconds, sample_rate, rng):
    streams = []
    for i in range(count):
        n = int(rng.uniform(seconds[0], seconds[1]) * sample_rate)
        streams.append(np.roll(recs[i % 2], int(rng.integers(0, len(recs[i % 2]))))[:n])
    return streams


def test_library_choice_cuts_eight_streams_of_minutes(gpu, bursts_1200):
    M, torch, ctx = gpu
    cfg, recs = bursts_1200
    streams = _rolled(recs, 8, (150, 200), cfg.sample_rate, np.random.default_rng(5))
    d, lens = _upload(torch, streams)
    got, st = _split(M, ctx, cfg, d, lens)
    want = _one_call(M, torch, ctx, cfg, d, lens)
    assert all(s["nchunks"] >= 2 for s in st), st
    assert len({s["chunk"] for s in st}) == 1
    for i in range(8):
        _same(got, i, want, i, cfg, (i, st[i]))
    print("rows", sum(s["nchunks"] for s in st), "L", st[0]["chunk"], "W", st[0]["warmup"],
          [(s["nchunks"], s["accepted"], s["rerun"], s["rounds"]) for s in st])


def test_library_choice_leaves_eight_short_streams_to_one_call(gpu, bursts_1200):
    M, torch, ctx = gpu
    cfg, recs = bursts_1200
    streams = _rolled(recs, 8, (8, 8), cfg.sample_rate, np.random.default_rng(6))
    streams[3] = streams[3][:-5]
    d, lens = _upload(torch, streams)
    got, st = _split(M, ctx, cfg, d, lens)
    want = _one_call(M, torch, ctx, cfg, d, lens)
    assert [s["nchunks"] for s in st] == [1] * 8 and [s["chunk"] for s in st] == lens
    assert all(s["accepted"] == s["rerun"] == s["rounds"] == 0 for s in st)
    for i in range(8):
        assert _same(got, i, want, i, cfg, i) > 0


def test_speed_sixteen_streams_of_five_minutes(gpu, bursts_1200):
    """16 x 5 minutes of bursty Bell-202 at 20 dB: the split with the library's choices against
    the demod_batch call it replaces, in the same process, device events after a preheat.  No
    margin beyond 1.0: a split slower than the call it replaces is a failed feature."""
    M, torch, ctx = gpu
    cfg, recs = bursts_1200
    streams = _rolled(recs, 16, (300, 300), cfg.sample_rate, np.random.default_rng(8))
    d, lens = _upload(torch, streams)
    dn = torch.tensor(lens, dtype=torch.int32, device="cuda")
    # preheat both paths (tables, allocator)
    M.demod_batch(ctx, cfg, d[:, :48000 * 8].contiguous(), want=("bytes",))
    M.demod_long_batch(ctx, cfg, d[:, :48000 * 120].contiguous(), want=("bytes",))
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    single = M.demod_batch(ctx, cfg, d, nsamples=dn, want=("bytes",))
    e1.record()
    torch.cuda.synchronize()
    t_batch = e0.elapsed_time(e1)
    e1.record()
    out = M.demod_long_batch(ctx, cfg, d, nsamples=lens, want=("bytes",))
    e2.record()
    torch.cuda.synchronize()
    t_split = e1.elapsed_time(e2)
    st = out["stats"]
    msg = ("one call %.1f ms, time-split %.1f ms, ratio %.2fx, rows %d L=%d W=%d, call's rounds %d, "
           "per stream K/accepted/rerun %s" % (
               t_batch, t_split, t_batch / t_split, sum(s["nchunks"] for s in st), st[0]["chunk"],
               st[0]["warmup"], max(s["rounds"] for s in st),
               " ".join("%d/%d/%d" % (s["nchunks"], s["accepted"], s["rerun"]) for s in st)))
    print(msg)
    for i in range(16):
        nb = int(single["nbytes"][i])
        assert nb > 0 and nb == int(out["nbytes"][i]), (i, msg)
        assert torch.equal(single["bytes"][i, :nb], out["bytes"][i, :nb]), (i, msg)
    assert t_split < t_batch, msg
