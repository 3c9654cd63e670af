"""--confidence (-c) and --limit (-l) through the product, against the oracle, bit for bit.

The receive loop reads the two values in several separate places on the device -- the wavefront
engine's winner selection (two ballots while the best confidence is below the limit, a serial loop
otherwise), its lattice replay predicate, the workgroup engine's bulk replay, its shortcut that
forwards a scored first try, its general path, and the early exit of a search across chunks of
candidates -- and every other sweep runs at the defaults, 1.5 / 2.3.  Here nine (threshold, limit)
pairs per rate, placed at quartiles of the oracle's own confidences (_thresholds.py), at the six
rates of _shapes.RATES with 8-N-1 frames, over six streams (clean, sigma 0.1 / 0.25 / 0.4, cut short,
noise only): one launch, in slabs on the resumable instantiations, chained, and under --auto-carrier,
where the band is dropped after 21 searches without confidence and detected again."""
import numpy as np
import pytest

import _oracle as O
import _shapes as S
import _thresholds as T
from test_gpu_chain import _chained
from test_gpu_frameshapes import _host_lib
from test_gpu_parity import VARIANTS, VARIANT_IDS, assert_stream_equal, gpu, run_gpu_streams  # noqa: F401
from test_gpu_slabs import _feed_in_slabs

CNT_BULK_FRAMES = 3                     # MIFSK_CNT_BULK_FRAMES (include/mifsk.h)
AUTO = (("auto_carrier_threshold", 0.001),)
AUTO_RATES = ["1200", "240"]
AUTO_PAIRS = ["c-q50-l-q75", "c1e9"]
SLAB_PAIRS = ["c0-l0", "c-q50-l-q75", "l-inf"]


def product_config(rate, pid, extra=()):
    return _host_lib().rx_config(T.rate_mode(rate), **dict(T.SHAPE, **dict(T.pair(rate, pid), **dict(extra))))


@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_the_threshold_sweep_is_worth_running(rate):
    """What keeps the sweep honest, on the CPU, at every rate: the product's and the oracle's
    configurations agree on both values for all nine pairs (the limit is lifted to the threshold,
    inf stays inf); at least 6 of the 9 oracle outcomes -- the frames and episodes of all six
    streams -- are pairwise distinct; every pair with another threshold than the default's differs
    from the default outcome; no stream yields more frames than mifsk_max_frames or more episodes
    than mifsk_max_episodes (nor than the 16 episode records run_gpu_streams asks for); the
    default run finds at least 30 frames in each keyed stream up to sigma = 0.25; and with the limit
    at q50 the oracle accepts a frame whose confidence equals the limit."""
    M = _host_lib()
    streams = T.streams_of(rate)
    outcomes = {}
    for pid, kw in T.pairs(rate):
        cfg = product_config(rate, pid)
        ocfg = O.oracle_config(T.rate_mode(rate), **dict(T.SHAPE, **kw))
        for field in ("confidence_threshold", "search_limit"):
            assert getattr(cfg, field) == getattr(ocfg, field), (rate, pid, field)
        assert cfg.confidence_threshold == np.float32(kw.get("confidence_threshold", 1.5)), (rate, pid)
        assert cfg.search_limit == max(np.float32(kw.get("search_limit", 2.3)), np.float32(cfg.confidence_threshold)), (rate, pid)
        refs = T.oracle_results(rate, pid)
        for s, ref in zip(streams, refs):
            assert len(ref["frames"]) <= M.max_frames(cfg, len(s)), (rate, pid)
            assert len(ref["episodes"]) <= min(16, M.max_episodes(cfg, len(s))), (rate, pid)
        outcomes[pid] = T.outcome(refs)
    assert len(set(outcomes.values())) >= 6, rate
    for pid, kw in T.pairs(rate):
        if "confidence_threshold" in kw:
            assert outcomes[pid] != outcomes["default"], (rate, pid)
    for i in (0, 1, 2, 4):
        assert len(T.oracle_results(rate, "default")[i]["frames"]) >= 30, (rate, T.STREAM_IDS[i])
    # the quartiles are observed confidences: with the limit at q50 some frame is accepted AT the limit
    q50 = np.float32(T.quartiles(rate)[1])
    for ring in (False, True):
        assert any(np.any(r["frames"]["confidence"] == q50) for r in T.oracle_results(rate, "l-q50", ring)), (rate, ring)


@pytest.mark.parametrize("rate", AUTO_RATES)
def test_the_band_is_detected_again_and_again_when_nothing_decodes(rate):
    """--auto-carrier under -c 1e9: every 21 searches without confidence drop the band (minimodem.c:1297)
    and the scan for it starts over -- the oracle scans at least three times as many windows of the
    clean stream as at the default options.  What test_auto_carrier_under_thresholds runs, on the CPU."""
    scans = [T.oracle_results(rate, pid, extra=AUTO)[0]["n_scan_windows"] for pid in ("default", "c1e9")]
    assert scans[0] >= 1 and scans[1] >= 3 * scans[0], scans
    for pid in AUTO_PAIRS:
        ocfg = O.oracle_config(T.rate_mode(rate), **dict(T.SHAPE, **dict(T.pair(rate, pid), **dict(AUTO))))
        cfg = product_config(rate, pid, AUTO)
        assert (cfg.confidence_threshold, cfg.search_limit) == (ocfg.confidence_threshold, ocfg.search_limit)
        assert all(len(r["episodes"]) <= 16 for r in T.oracle_results(rate, pid, extra=AUTO))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_confidence_options_match_oracle(gpu, rate, variant):  # noqa: F811
    """The nine pairs of a rate in one launch each: every stream's frames (confidence and amplitude
    as bit patterns), bytes and episodes are the oracle's in the matching addressing mode."""
    M, torch, ctx = gpu
    engine, ring = variant
    streams = T.streams_of(rate)
    total = 0
    for pid, _kw in T.pairs(rate):
        res = run_gpu_streams(M, torch, ctx, product_config(rate, pid), streams, engine=engine, ring=ring)
        for i, ref in enumerate(T.oracle_results(rate, pid, ring)):
            assert_stream_equal(res, i, ref, "%s/%s/%s" % (rate, pid, T.STREAM_IDS[i]))
            total += len(ref["frames"])
    assert total >= 9 * 30


def _cuts(rate, streams):
    rng = np.random.default_rng([T.SEED, S.RATE_IDS.index(rate), 4242])
    return [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=2)) for x in streams]


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["wave", "workgroup", "alternate"])
@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_confidence_options_in_three_slabs_match_oracle(gpu, rate, engine):  # noqa: F811
    """The resumable instantiations have a replay branch of their own (and the buffer arithmetic of a
    saved state): the same streams in three slabs cut at seeded positions, on both engines and on
    the two taking turns."""
    M, torch, ctx = gpu
    streams = T.streams_of(rate)
    cuts = _cuts(rate, streams)
    for pid in SLAB_PAIRS:
        got = _feed_in_slabs(M, ctx, product_config(rate, pid), streams, cuts, engine=engine)
        for i, ref in enumerate(T.oracle_results(rate, pid)):
            label = (rate, pid, T.STREAM_IDS[i], cuts[i])
            assert got[i]["frames"].tobytes() == ref["frames"].tobytes(), label
            assert got[i]["bytes"] == ref["bytes"], label
            assert got[i]["episodes"].tobytes() == ref["episodes"].tobytes(), label


@pytest.mark.gpu
@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_confidence_options_chained_match_oracle(gpu, monkeypatch, rate):  # noqa: F811
    """... and cut into 2 groups of streams x 4 time chunks, every one a launch of the wavefront
    engine's resumable kernel (where the rate's instantiation has a resumable twin)."""
    M, torch, ctx = gpu
    streams = T.streams_of(rate)
    stride = (max(len(s) for s in streams) + 3) & ~3
    monkeypatch.setenv("MIFSK_EXPERIMENT", "1")
    monkeypatch.setenv("MIFSK_CHAIN", "2,4")
    if not _chained(M, ctx, product_config(rate, "default"), len(streams), stride, "wave")[0]:
        pytest.skip("no resumable twin for this rate's instantiation")
    for pid in SLAB_PAIRS:
        cfg = product_config(rate, pid)
        assert _chained(M, ctx, cfg, len(streams), stride, "wave") == (2, 4)
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine="wave")
        for i, ref in enumerate(T.oracle_results(rate, pid)):
            assert_stream_equal(res, i, ref, "%s/%s/%s chained" % (rate, pid, T.STREAM_IDS[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("ring", [False, True], ids=["flat", "ring"])
@pytest.mark.parametrize("rate", AUTO_RATES)
def test_auto_carrier_under_thresholds(gpu, rate, ring):  # noqa: F811
    """--auto-carrier with a threshold in the middle of the distribution and with one nothing
    reaches: the band found last and every episode's b_mark are the oracle's."""
    M, torch, ctx = gpu
    streams = T.streams_of(rate)
    for pid in AUTO_PAIRS:
        res = run_gpu_streams(M, torch, ctx, product_config(rate, pid, AUTO), streams, ring=ring)
        for i, ref in enumerate(T.oracle_results(rate, pid, ring, AUTO)):
            label = "%s/%s/%s auto" % (rate, pid, T.STREAM_IDS[i])
            assert int(res["carrier_band"][i]) == ref["carrier_band"], label
            assert_stream_equal(res, i, ref, label)
            ne = int(res["nepisodes"][i])
            assert np.array_equal(res["episodes"][i, :ne]["b_mark"], ref["episodes"]["b_mark"]), label


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["wave", "workgroup"])
def test_no_frame_is_taken_from_the_lattice_under_an_infinite_limit(gpu, engine):  # noqa: F811
    """The option is read where the speculation is decided: with -l inf no finite confidence
    reaches the limit and MIFSK_CNT_BULK_FRAMES stays 0 on the sigma = 0.1 stream at 1200 baud; at
    the default limit the lattice delivers frames."""
    M, torch, ctx = gpu
    x = T.streams_of("1200")[1]
    bulk = {}
    for pid in ("default", "l-inf"):
        res = run_gpu_streams(M, torch, ctx, product_config("1200", pid), [x], engine=engine,
                              want=("bytes", "frames", "episodes", "bits", "counters"))
        ref = T.oracle_results("1200", pid)[1]
        assert_stream_equal(res, 0, ref, "1200/%s" % pid)
        assert np.all(np.isfinite(ref["frames"]["confidence"]))
        bulk[pid] = int(res["counters"][0, CNT_BULK_FRAMES])
    assert bulk["l-inf"] == 0 and bulk["default"] > 0, bulk
