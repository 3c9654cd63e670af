"""One long recording decoded across the chip by cutting it in time (mifsk_demod_long; DESIGN.md
"cutting a stream in time").  Whatever the cut -- chunk starts mid-frame, mid-episode or in
silence, guesses accepted or all re-run -- the outputs must be those of ONE demod_batch call over
the whole recording, bit for bit: frames (f32 patterns included), bits, bytes, episodes (their
float totals included), status and the --auto-carrier band."""
import math
import time
import zlib

import numpy as np
import pytest

import _golden as G
import _oracle as O
from _timesplit import _lattice  # noqa: F401  (the other time-split modules take it from here)

pytestmark = pytest.mark.gpu

WANT = ("bytes", "bits", "frames", "episodes")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _single(M, torch, ctx, cfg, x, engine=None):
    n = len(x)
    host = np.zeros(((n + 3) & ~3), np.float32)
    host[:n] = x
    d = torch.from_numpy(host[None, :]).cuda()
    dn = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = M.demod_batch(ctx, cfg, d, nsamples=dn, want=WANT + (("carrier_band",) if cfg.auto_carrier_threshold > 0 else ()),
                        episodes_cap=M.max_episodes(cfg, n), engine=engine)
    torch.cuda.synchronize()
    return M.results_to_host(out)


def _long(M, torch, ctx, cfg, x, **kw):
    d = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = M.demod_long(ctx, cfg, d, want=WANT, **kw)
    stats = out.pop("stats")
    return M.results_to_host(out), stats


def _same(a, b, cfg, what):
    nf = int(a["nframes"][0])
    assert nf == int(b["nframes"][0]), what
    assert a["frames"][0, :nf].tobytes() == b["frames"][0, :nf].tobytes(), what
    assert a["bits"][0, :nf].tobytes() == b["bits"][0, :nf].tobytes(), what
    nb = int(a["nbytes"][0])
    assert nb == int(b["nbytes"][0]) and a["bytes"][0, :nb].tobytes() == b["bytes"][0, :nb].tobytes(), what
    ne = int(a["nepisodes"][0])
    assert ne == int(b["nepisodes"][0]), what
    assert a["episodes"][0, :ne].tobytes() == b["episodes"][0, :ne].tobytes(), what
    assert int(a["status"][0]) == int(b["status"][0]), what
    if cfg.auto_carrier_threshold > 0:
        assert int(a["carrier_band"][0]) == int(b["carrier_band"][0]), what
    return nf


def _recording(x, rng, copies=3, sample_rate=48000):
    parts = []
    for _ in range(copies):
        parts.append(np.zeros(int(rng.integers(0, sample_rate // 3)), np.float32))
        parts.append(x)
    parts.append(np.zeros(int(rng.integers(0, sample_rate // 5)), np.float32))
    return np.concatenate(parts).astype(np.float32)


GOLDENS = [n for n in G.names() if n != "t04_0p5"]     # (0.5 baud: 6 M samples, one frame per 2 s)


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("engine", [None, "wave", "workgroup"])
def test_golden_recordings_joined_and_cut_small_equal_one_call(gpu, name, engine):
    M, torch, ctx = gpu
    g = G.load(name)
    cfg = M.rx_config(**g["cfg_kwargs"])
    if engine == "workgroup" and cfg.auto_carrier_threshold > 0:
        pytest.skip("the workgroup engine has no in-loop --auto-carrier")
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = _recording(g["samples"], rng, sample_rate=cfg.sample_rate)
    lat = _lattice(cfg)
    W = 2 * cfg.samplebuf_size
    want = _single(M, torch, ctx, cfg, x, engine=engine)
    for mult in (1, 3):
        L = lat * max(1, (len(x) // 12) // lat // mult)
        got, st = _long(M, torch, ctx, cfg, x, chunk=L, warmup=W + lat * (mult - 1), engine=engine)
        assert st["nchunks"] >= 2 or len(x) < 2 * L + W, st
        _same(got, want, cfg, (name, engine, st))


@pytest.mark.parametrize("name", ["t01_1200", "t03_rtty", "t40_rxnoise_0p05_rxone", "t50_auto_300",
                                  "t80_same", "t70_callerid_mdmf"])
def test_reject_all_reruns_every_chunk_and_still_equals_one_call(gpu, name):
    M, torch, ctx = gpu
    g = G.load(name)
    cfg = M.rx_config(**g["cfg_kwargs"])
    x = _recording(g["samples"], np.random.default_rng(7), sample_rate=cfg.sample_rate)
    lat = _lattice(cfg)
    L = lat * max(1, (len(x) // 10) // lat)
    got, st = _long(M, torch, ctx, cfg, x, chunk=L, warmup=2 * cfg.samplebuf_size, reject_all=True)
    want = _single(M, torch, ctx, cfg, x)
    _same(got, want, cfg, (name, st))
    assert st["nchunks"] >= 2 and st["accepted"] == 0
    if cfg.rx_one == 0:
        # every chunk went through the re-run path at least once
        assert st["rerun"] >= st["nchunks"] - 1 and 1 <= st["rounds"] <= st["nchunks"] - 1, st


def _bursty(M, cfg, seconds, rng, snr_db=None, dc=0.0, continuous=False):
    """Bursts of 20 - 120 random 8N1 bytes (or one continuous carrier) between silences."""
    sr = cfg.sample_rate
    parts, total = [], 0
    while total < seconds * sr:
        if not continuous:
            gap = np.zeros(int(rng.uniform(0.04, 1.25) * sr), np.float32)
            parts.append(gap)
            total += len(gap)
        nbytes = int(rng.integers(20, 121)) if not continuous else int(seconds * cfg.data_rate / 10) + 10
        words = rng.integers(0, 256 if cfg.n_data_bits >= 8 else (1 << cfg.n_data_bits), size=nbytes, dtype=np.uint8)
        b = M.synthesize(cfg, words, leading_silence=0)
        parts.append(b)
        total += len(b)
    x = np.concatenate(parts)[: int(seconds * sr)].astype(np.float32)
    if snr_db is not None:
        p = float(np.mean(x[x != 0] ** 2)) if np.any(x) else 1.0
        x = x + rng.normal(0, math.sqrt(p / 10 ** (snr_db / 10)), x.shape).astype(np.float32)
    return (x + np.float32(dc)).astype(np.float32)


MODES = [("1200", {}), ("300", {}), ("rtty", {}), ("same", {}), ("tdd", {}),
         ("12000", {}), ("1200", {"sample_rate": 24000, "mark_f": 1200.0, "space_f": 2400.0})]


@pytest.mark.parametrize("mode,kw", MODES)
@pytest.mark.parametrize("cond", ["clean", "20dB", "6dB_dc", "continuous_12dB"])
def test_modes_minutes_long_equal_one_call_and_oracle(gpu, mode, kw, cond):
    M, torch, ctx = gpu
    cfg = M.rx_config(mode, **kw)
    rng = np.random.default_rng(11)
    snr = {"clean": None, "20dB": 20, "6dB_dc": 6, "continuous_12dB": 12}[cond]
    x = _bursty(M, cfg, 120, rng, snr_db=snr, dc=0.05 if cond == "6dB_dc" else 0.0,
                continuous=cond.startswith("continuous"))
    lat = _lattice(cfg)
    W = max(2 * cfg.samplebuf_size, (2 * cfg.sample_rate) // lat * lat)
    L = lat * max(1, (len(x) // 32) // lat)
    got, st = _long(M, torch, ctx, cfg, x, chunk=L, warmup=W)
    want = _single(M, torch, ctx, cfg, x)
    nf = _same(got, want, cfg, (mode, cond, st))
    if cond == "clean":
        ref = O.oracle_rx_stream(O.oracle_config(mode, **kw), x)
        assert nf == len(ref["frames"]) and got["frames"][0, :nf].tobytes() == ref["frames"].tobytes()
    print(mode, kw, cond, st)


def test_library_choice_on_a_long_recording(gpu):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    x = _bursty(M, cfg, 300, np.random.default_rng(3), snr_db=20)
    got, st = _long(M, torch, ctx, cfg, x)
    want = _single(M, torch, ctx, cfg, x)
    _same(got, want, cfg, st)
    assert st["nchunks"] >= 2, st


@pytest.mark.parametrize("engine", [None, "wave", "workgroup"])
def test_sync_byte_frames_are_suppressed_as_in_one_call(gpu, engine):
    """--sync-byte: frames equal to the sync byte are kept in the frame list (MIFSK_FRAME_SYNC)
    and left out of the bytes, across the cuts as in the single call."""
    M, torch, ctx = gpu
    g = G.load("t01_1200")
    payload = np.frombuffer(g["payload"], np.uint8)
    sync = int(np.bincount(payload).argmax())
    cfg = M.rx_config("1200", sync_byte=sync)
    x = _recording(g["samples"], np.random.default_rng(9), copies=4, sample_rate=cfg.sample_rate)
    lat = _lattice(cfg)
    got, st = _long(M, torch, ctx, cfg, x, chunk=lat * max(1, (len(x) // 16) // lat),
                    warmup=2 * cfg.samplebuf_size, engine=engine)
    want = _single(M, torch, ctx, cfg, x, engine=engine)
    nf = _same(got, want, cfg, (engine, st))
    suppressed = int(np.count_nonzero(got["frames"][0, :nf]["flags"] & 2))
    assert st["nchunks"] >= 8 and suppressed > 0 and int(got["nbytes"][0]) == nf - suppressed


def test_text_through_stream_text(gpu):
    """baudot, caller-ID and UIC text printed from the stitched bits and episodes."""
    M, torch, ctx = gpu
    for name in ("t03_rtty", "t70_callerid_mdmf", "t81_tdd"):
        g = G.load(name)
        cfg = M.rx_config(**g["cfg_kwargs"])
        x = _recording(g["samples"], np.random.default_rng(5), sample_rate=cfg.sample_rate)
        lat = _lattice(cfg)
        got, st = _long(M, torch, ctx, cfg, x, chunk=lat * max(1, (len(x) // 8) // lat),
                        warmup=2 * cfg.samplebuf_size)
        want = _single(M, torch, ctx, cfg, x)
        t1 = M.stream_text(cfg, got["bits"][0, :int(got["nframes"][0])],
                           got["episodes"][0, :int(got["nepisodes"][0])])
        t2 = M.stream_text(cfg, want["bits"][0, :int(want["nframes"][0])],
                           want["episodes"][0, :int(want["nepisodes"][0])])
        assert t1 == t2, name


def test_speed_one_hour_bursty_1200_at_20dB(gpu):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    x = _bursty(M, cfg, 3600, np.random.default_rng(2024), snr_db=20)
    d = torch.from_numpy(x).cuda()
    dn = torch.tensor([len(x)], dtype=torch.int32, device="cuda")
    host = torch.zeros((1, (len(x) + 3) & ~3), dtype=torch.float32, device="cuda")
    host[0, :len(x)] = d
    # preheat both paths (tables, allocator)
    M.demod_batch(ctx, cfg, host[:, :48000 * 8].contiguous(), want=("bytes",))
    M.demod_long(ctx, cfg, d[:48000 * 120].contiguous(), want=("bytes",))
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    single = M.demod_batch(ctx, cfg, host, nsamples=dn, want=("bytes",))
    e1.record()
    torch.cuda.synchronize()
    t_single = e0.elapsed_time(e1)
    t0 = time.perf_counter()
    e1.record()
    out = M.demod_long(ctx, cfg, d, want=("bytes",))
    e2.record()
    torch.cuda.synchronize()
    t_long = e1.elapsed_time(e2)
    wall = (time.perf_counter() - t0) * 1e3
    st = out["stats"]
    nb = int(single["nbytes"][0])
    assert nb == int(out["nbytes"][0])
    assert torch.equal(single["bytes"][0, :nb], out["bytes"][0, :nb])
    speedup = t_single / t_long
    msg = ("single %.1f ms, time-split %.1f ms (wall %.1f), speedup %.2fx, K=%d L=%d W=%d accepted %d/%d, "
           "rerun %d, rounds %d" % (t_single, t_long, wall, speedup, st["nchunks"], st["chunk"], st["warmup"],
                                   st["accepted"], st["nchunks"] - 1, st["rerun"], st["rounds"]))
    print(msg)
    assert speedup >= 5.0, msg
