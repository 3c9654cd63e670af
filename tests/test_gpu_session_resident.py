"""The resident session (MIFSK_SESSION_RESIDENT, csrc/mifsk_session.cpp and session_append_kernel in
csrc/mifsk_ingest.hip): the unconsumed tails stay in device memory, a feed uploads only its new
samples -- float32 or PCM16 -- or takes them from a device tensor.  Whatever the cuts and the
source, the concatenated frames, bytes and episodes are the oracle's, bit for bit, and `pending`
and `consumed` are the host-tail session's."""
import ctypes as C
import time

import numpy as np
import pytest

import _golden as G
import _oracle as O

pytestmark = pytest.mark.gpu

SOURCES = ["host_f32", "host_s16", "dev_f32", "dev_s16", "dev_s16_slice"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _pieces(streams, cuts, k):
    new = []
    for i, x in enumerate(streams):
        e = [0] + list(cuts[i]) + [len(x)]
        new.append(x[e[k]:e[k + 1]])
    return new


def _feed_one(torch, sess, new, final, source="host_f32", rxnoise=0.0):
    """one feed of the pieces `new` (numpy arrays of the source's element type) from `source`"""
    if source.startswith("host"):
        return sess.feed(new, final=final, rxnoise=rxnoise)
    n, kmax = len(new), max(len(p) for p in new)
    dtype = new[0].dtype
    lead = 1 if source.endswith("slice") else 0
    # (what lies behind a row's samples is not the stream's: make it loud)
    slab = np.full((n, lead + kmax), 12345, dtype)
    for i, p in enumerate(new):
        slab[i, lead:lead + len(p)] = p
    t = torch.from_numpy(slab).cuda()[:, lead:]
    assert t.data_ptr() % 4 == 2 * lead or kmax == 0
    return sess.feed(t, final=final, rxnoise=rxnoise, nsamples=[len(p) for p in new])


def _feed(M, torch, ctx, cfg, streams, cuts, source="host_f32", rxnoise=0.0, shadow=False, each=None, **kw):
    """cuts[i]: sorted cut positions of stream i (the same number for every stream).  shadow: a
    host-tail session is fed the same pieces, and pending / consumed must agree on every feed
    that is not the final one (pending: of the streams the loop has not finished -- of those
    the resident session holds nothing).  each(k, new, sess, res): called after every feed."""
    n, ncalls = len(streams), len(cuts[0]) + 1
    sess = M.Session(ctx, cfg, n, resident=True, **kw)
    host = M.Session(ctx, cfg, n, **kw) if shadow else None
    acc = [dict(frames=[], bytes=b"", episodes=[]) for _ in range(n)]
    for k in range(ncalls):
        new = _pieces(streams, cuts, k)
        final = k == ncalls - 1
        res = _feed_one(torch, sess, new, final, source, rxnoise)
        if host is not None:
            ref = host.feed(new, final=final)
            assert [(r["consumed"], r["finished"]) for r in res] == [(r["consumed"], r["finished"]) for r in ref], k
            if not final:
                assert [0 if r["finished"] else r["pending"] for r in ref] == [r["pending"] for r in res], k
        for i, r in enumerate(res):
            assert r["status"] == 0
            acc[i]["frames"].append(r["frames"])
            acc[i]["bytes"] += r["bytes"]
            acc[i]["episodes"].append(r["episodes"])
            assert r["finished"] == (ref[i]["finished"] if host is not None else final)
        if each is not None:
            each(k, new, sess, res)
    assert sess.info()["feeds"] == ncalls and sess.info()["resident"] == 1
    sess.close()
    if host is not None:
        host.close()
    for a in acc:
        a["frames"] = np.concatenate(a["frames"])
        a["episodes"] = np.concatenate(a["episodes"])
    return acc


def _same(got, ref, what):
    assert got["frames"].tobytes() == ref["frames"].tobytes(), what
    assert got["bytes"] == ref["bytes"], what
    assert got["episodes"].tobytes() == ref["episodes"].tobytes(), what


# ---- 1. every golden, every variant, fed in pieces --------------------------

@pytest.mark.parametrize("variant", ["library", "wave", "workgroup", "ring"])
@pytest.mark.parametrize("name", G.names())
def test_any_golden_fed_in_pieces_equals_the_oracle(gpu, name, variant):
    M, torch, ctx = gpu
    g = G.load(name)
    cfg = M.rx_config(**g["cfg_kwargs"])
    ocfg = O.oracle_config(**g["cfg_kwargs"])
    x = g["samples"]
    if len(x) > 2000000:
        pytest.skip("0.5 baud: one samplebuf is longer than the recording's pieces")
    if variant == "workgroup" and cfg.auto_carrier_threshold > 0:
        pytest.skip("--auto-carrier runs on the wavefront engine")
    ring = variant == "ring"
    ref = O.oracle_rx_stream(ocfg, x, ring_mode=ring)
    rng = np.random.default_rng(len(x) + 7)
    for trial in range(2):
        cuts = sorted(int(c) for c in rng.integers(0, len(x) + 1, size=3))
        if trial == 1:
            cuts = [1, 2, len(x) // 2, len(x)]                 # tiny pieces, and an empty final one
        got = _feed(M, torch, ctx, cfg, [x], [cuts], shadow=True, ring_exact=ring,
                    engine=None if variant in ("library", "ring") else variant)[0]
        _same(got, ref, (name, cuts))


# ---- 2. sources, 4. only new samples cross the bus ---------------------------

_NWORDS = {"1200": 60, "300": 24, "12000": 200, "same": 40, "rtty": 6}
_SEED = {"1200": 11, "300": 12, "12000": 13, "same": 14, "rtty": 15}
_ragged_cache = {}


def _ragged(M, mode):
    """the ragged noisy batch of tests/test_gpu_session.py (9 streams, five cuts each), once per
    mode: the float streams, the same rounded to PCM16, the cuts"""
    if mode not in _ragged_cache:
        cfg = M.rx_config(mode)
        rng = np.random.default_rng(_SEED[mode])
        nwords = _NWORDS[mode]
        streams = []
        for i in range(9):
            words = rng.integers(0 if mode == "rtty" else 32, 32 if mode == "rtty" else 127, size=nwords + i, dtype=np.uint8)
            x = M.synthesize(cfg, words, amplitude=0.7, leading_silence=int(rng.integers(0, 300)))
            if i % 3 == 1:                                     # a second burst behind a gap
                x = np.concatenate([x, np.zeros(int(rng.integers(100, 3000)), np.float32),
                                    M.synthesize(cfg, words[: nwords // 2], amplitude=0.7)])
            streams.append((x + rng.normal(0, 0.056, x.shape)).astype(np.float32))
        pcm = [np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) for x in streams]
        cuts = [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=5)) for x in streams]
        _ragged_cache[mode] = dict(f32=streams, s16=pcm, cuts=cuts, refs={})
    return _ragged_cache[mode]


def _dc(rxnoise):
    # simpleaudio-sndfile.c:67-69 with rand()/RAND_MAX == 0, in float
    return np.float32(0) if rxnoise == 0.0 else (np.float32(0) - np.float32(0.5)) * (np.float32(rxnoise) * np.float32(2))


def _ragged_refs(M, mode, kind, rxnoise):
    """the oracle over what the device makes of each stream, computed in numpy float32"""
    b = _ragged(M, mode)
    key = (kind, rxnoise)
    if key not in b["refs"]:
        ocfg = O.oracle_config(mode)
        dc = _dc(rxnoise)
        refs = []
        for i in range(9):
            if kind == "s16":
                y = b["s16"][i].astype(np.float32) / np.float32(32768) + dc
            else:
                y = b["f32"][i] + dc if rxnoise != 0.0 else b["f32"][i]
            assert y.dtype == np.float32
            refs.append(O.oracle_rx_stream(ocfg, y))
        b["refs"][key] = refs
    return b["refs"][key]


@pytest.mark.parametrize("rxnoise", [0.0, 0.05])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", ["1200", "300", "12000", "same", "rtty"])
def test_ragged_noisy_batch_from_every_source(gpu, mode, source, rxnoise):
    M, torch, ctx = gpu
    cfg = M.rx_config(mode)
    b = _ragged(M, mode)
    kind = "s16" if "s16" in source else "f32"
    streams, cuts = b[kind], b["cuts"]
    esz = streams[0].dtype.itemsize
    bounds = []

    def each(k, new, sess, res):
        # 4.: a condition on what the feed uploaded -- the new samples, each piece rounded up to
        # 16 bytes, and at most 64 bytes of table per stream
        bounds.append(sum((len(p) * esz + 15) // 16 * 16 for p in new) + 64 * len(new))
        if source.startswith("host"):
            assert sess.info()["h2d_bytes_last"] <= bounds[-1], (k, sess.info())
        else:
            assert sess.info()["h2d_bytes_last"] <= 64 * len(new), (k, sess.info())   # the table alone

    got = _feed(M, torch, ctx, cfg, streams, cuts, source=source, rxnoise=rxnoise, each=each)
    for i, ref in enumerate(_ragged_refs(M, mode, kind, rxnoise)):
        _same(got[i], ref, (mode, source, rxnoise, i))
    if source == "host_f32" and rxnoise == 0.0:
        # the bound is not vacuous: the host-tail session uploads its tails again
        host = M.Session(ctx, cfg, 9)
        over = 0
        for k in range(6):
            host.feed(_pieces(streams, cuts, k), final=(k == 5))
            over += host.info()["h2d_bytes_last"] > bounds[k]
        assert host.info()["resident"] == 0 and host.info()["row_capacity"] == 0
        host.close()
        assert over >= 1


# ---- 3. growth ---------------------------------------------------------------

def test_rows_grow_with_the_feed(gpu):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    rng = np.random.default_rng(3)
    x = M.synthesize(cfg, rng.integers(32, 127, size=640, dtype=np.uint8), leading_silence=100)
    assert len(x) > 30 * 64 + 200000 + 1000
    cuts = [64 * (j + 1) for j in range(30)] + [30 * 64 + 200000]
    caps = []
    got = _feed(M, torch, ctx, cfg, [x], [cuts], each=lambda k, new, sess, res: caps.append(sess.info()["row_capacity"]))[0]
    assert all(c % 4 == 0 for c in caps) and all(b >= a for a, b in zip(caps, caps[1:]))
    # 30 x 64 samples are less than a samplebuf: nothing is passed yet, the row holds them all
    assert caps[0] >= 64 and caps[29] >= 30 * 64 > caps[0]
    assert caps[30] >= 200000 > caps[29]
    assert caps[31] == caps[30]
    _same(got, O.oracle_rx_stream(O.oracle_config("1200"), x), "growth")


# ---- 5. finished streams hold nothing ----------------------------------------

def test_finished_streams_hold_nothing(gpu):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200", rx_one=1)
    ocfg = O.oracle_config("1200", rx_one=1)
    rng = np.random.default_rng(5)
    w = rng.integers(32, 127, size=200, dtype=np.uint8)
    x0 = np.concatenate([M.synthesize(cfg, w[:40], leading_silence=200), np.zeros(24000, np.float32),
                         M.synthesize(cfg, w[40:140])])
    x1 = M.synthesize(cfg, w, leading_silence=50)              # one burst, up to the stream's end
    streams = [x0, x1]
    nfeeds = (max(len(x0), len(x1)) + 4799) // 4800
    sess = M.Session(ctx, cfg, 2, resident=True)
    acc = [dict(frames=[], bytes=b"", episodes=[]) for _ in range(2)]
    done_at, caps = None, []
    for k in range(nfeeds):
        new = [x[k * 4800:(k + 1) * 4800] for x in streams]
        res = sess.feed(new, final=(k == nfeeds - 1))
        caps.append(sess.info()["row_capacity"])
        for i, r in enumerate(res):
            acc[i]["frames"].append(r["frames"])
            acc[i]["bytes"] += r["bytes"]
            acc[i]["episodes"].append(r["episodes"])
        if done_at is not None:
            r = res[0]
            assert r["pending"] == 0 and r["finished"]
            assert len(r["frames"]) == 0 and r["bytes"] == b"" and len(r["episodes"]) == 0
        elif res[0]["finished"]:
            done_at = k
            assert res[0]["pending"] == 0
    sess.close()
    assert done_at is not None and nfeeds - 1 - done_at >= 10, (done_at, nfeeds)
    assert len(set(caps[done_at:])) == 1                       # no growth once only stream 1 is live
    assert caps[-1] < 2 * cfg.samplebuf_size + 4800 + (2 * cfg.samplebuf_size + 4800) // 4 + 8
    for i, x in enumerate(streams):
        ref = O.oracle_rx_stream(ocfg, x)
        got = dict(frames=np.concatenate(acc[i]["frames"]), bytes=acc[i]["bytes"],
                   episodes=np.concatenate(acc[i]["episodes"]))
        _same(got, ref, ("rx_one", i))
    # --rx-one: the first burst and nothing of the second
    assert acc[0]["bytes"].startswith(bytes(w[:40])) and bytes(w[40:60]) not in acc[0]["bytes"]


# ---- 6. argument errors ------------------------------------------------------

def test_argument_errors(gpu):
    M, torch, ctx = gpu
    from minimodem_amd import _lib
    lib = _lib.load()
    cfg = M.rx_config("1200")
    x = M.synthesize(cfg, np.arange(40, 80, dtype=np.uint8))
    cnt = (C.c_uint32 * 2)(5, 0)
    ptrs = (C.c_void_p * 2)(x.ctypes.data, None)
    zero = C.c_float(0.0)
    h = C.c_void_p()
    assert lib.mifsk_session_create(C.byref(h), ctx.handle, C.byref(cfg), 1, _lib.SESSION_RESIDENT | 0x40) == -22
    assert lib.mifsk_session_create(C.byref(h), ctx.handle, C.byref(cfg), 1, _lib.SESSION_RESIDENT | 0x4000) == -22
    assert lib.mifsk_session_create(C.byref(h), ctx.handle, C.byref(cfg), 1,
                                    _lib.SESSION_RESIDENT | _lib.IO_RING_EXACT | _lib.IO_ENGINE_WORKGROUP) == -22
    plain = M.Session(ctx, cfg, 2)
    assert lib.mifsk_session_feed_ex(plain.handle, ptrs, cnt, _lib.FEED_F32, zero, 0) == -22
    d = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.mifsk_session_feed_device(plain.handle, C.c_void_p(d.data_ptr()), 8, cnt, _lib.FEED_F32, zero, 0,
                                         _lib.PIPELINE_NO_PRODUCER) == -22
    assert plain.info()["feeds"] == 0
    plain.close()
    s = M.Session(ctx, cfg, 2, resident=True)
    assert lib.mifsk_session_feed_ex(s.handle, ptrs, cnt, 2, zero, 0) == -22                   # an unknown kind
    assert lib.mifsk_session_feed_ex(s.handle, None, cnt, _lib.FEED_F32, zero, 0) == -22        # a count without its samples
    assert lib.mifsk_session_feed_ex(s.handle, (C.c_void_p * 2)(None, None), cnt, _lib.FEED_S16, zero, 0) == -22
    assert lib.mifsk_session_feed(s.handle, None, cnt, 0) == -22
    assert lib.mifsk_session_feed_device(s.handle, None, 8, cnt, _lib.FEED_F32, zero, 0, _lib.PIPELINE_NO_PRODUCER) == -22
    assert lib.mifsk_session_feed_device(s.handle, C.c_void_p(d.data_ptr()), 4, cnt, _lib.FEED_F32, zero, 0,
                                         _lib.PIPELINE_NO_PRODUCER) == -22                     # stride < a count
    assert lib.mifsk_session_feed_device(s.handle, C.c_void_p(d.data_ptr()), 8, cnt, 7, zero, 0,
                                         _lib.PIPELINE_NO_PRODUCER) == -22
    with pytest.raises(ValueError):
        s.feed([x, x.astype(np.int16)])                                                       # two kinds in one feed
    with pytest.raises(ValueError):
        s.feed([x.astype(np.float64), None])
    assert s.info()["feeds"] == 0 and s.info()["h2d_bytes_total"] == 0
    # the rejected feeds left nothing behind: the session decodes as a new one does
    r = s.feed([x[:7001], None])
    r2 = s.feed([x[7001:], None], final=True)
    assert r[0]["bytes"] + r2[0]["bytes"] == bytes(range(40, 80)) and r2[1]["bytes"] == b"" and r2[1]["finished"]
    assert lib.mifsk_session_feed_ex(s.handle, ptrs, cnt, _lib.FEED_F32, zero, 1) == -22        # after the final feed
    with pytest.raises(RuntimeError):
        s.feed([None, None], final=True)
    assert s.info()["feeds"] == 2
    assert not lib.mifsk_session_get(s.handle, 2) and lib.mifsk_session_pending(s.handle, -1) == 0
    s.close()


# ---- 7. speed ----------------------------------------------------------------

def test_speed_resident_against_host_tail_1024_streams():
    """1024 Bell-202 streams of 2 s at 20 dB in 20 feeds of 4800 samples: the resident session
    from host float32 and from host PCM16 may take at most 1.15 x the host-tail session's wall
    time (smallest of three, one untimed run of each path first), and all three decode alike."""
    import torch  # noqa: F401  (the device must be there)
    import minimodem_amd as M
    ctx = M.Context()
    cfg = M.rx_config("1200")
    n, nfeeds, piece = 1024, 20, 4800
    rng = np.random.default_rng(2024)
    total = nfeeds * piece
    base = []
    for j in range(8):                                         # eight payloads, 128 noisy copies of each
        y = M.synthesize(cfg, rng.integers(32, 127, size=230, dtype=np.uint8), amplitude=0.5,
                         leading_silence=int(rng.integers(0, 2000)))
        base.append(np.concatenate([y, np.zeros(total, np.float32)])[:total])
    sigma = np.float32(0.5 / np.sqrt(2.0) / 10.0)              # 20 dB below the tone's power
    pcm = np.empty((n, total), np.int16)
    for i in range(n):
        noise = rng.standard_normal(total, dtype=np.float32) * sigma
        pcm[i] = np.rint((base[i % 8] + noise) * 32768.0).astype(np.int16)
    f32 = pcm.astype(np.float32) / np.float32(32768)           # the same floats as the device makes of PCM16

    def run(resident, data):
        sess = M.Session(ctx, cfg, n, want_frames=False, resident=resident)
        out = [b""] * n
        dt = 0.0
        for k in range(nfeeds):
            new = [data[i, k * piece:(k + 1) * piece] for i in range(n)]
            t0 = time.perf_counter()
            res = sess.feed(new, final=(k == nfeeds - 1))
            dt += time.perf_counter() - t0
            for i, r in enumerate(res):
                out[i] += r["bytes"]
        h2d = sess.info()["h2d_bytes_total"]
        sess.close()
        return dt, out, h2d

    paths = [("host-tail", False, f32), ("resident f32", True, f32), ("resident s16", True, pcm)]
    outs, h2d = {}, {}
    for name, resident, data in paths:                         # untimed: code objects, pinned buffers
        _, outs[name], h2d[name] = run(resident, data)
    best = {name: min(run(resident, data)[0] for _ in range(3)) for name, resident, data in paths}
    ctx.close()
    assert outs["resident f32"] == outs["host-tail"] and outs["resident s16"] == outs["host-tail"]
    assert sum(len(o) for o in outs["host-tail"]) > n * 200   # the streams decode
    assert h2d["resident s16"] < h2d["resident f32"] < h2d["host-tail"]
    r32, r16 = best["resident f32"] / best["host-tail"], best["resident s16"] / best["host-tail"]
    msg = "20 feeds: host-tail %.1f ms, resident f32 %.1f ms (x %.3f), resident s16 %.1f ms (x %.3f); h2d %r" % (
        best["host-tail"] * 1e3, best["resident f32"] * 1e3, r32, best["resident s16"] * 1e3, r16, h2d)
    print(msg)
    assert r32 <= 1.15 and r16 <= 1.15, msg
