"""The confidence options of tests/test_gpu_thresholds.py: --confidence (-c) and --limit (-l) drive
every decision of the receive loop -- a search stops at the first candidate that reaches the limit,
a speculated frame is accepted without a search when it reaches the limit, a frame counts only
above the threshold -- and the confidence scale depends on the bit length, so the values are placed
at quartiles of the ORACLE's own frame confidences at each rate.  Plain helpers: the streams of a
rate, its nine (threshold, limit) pairs, the oracle's outcome under each."""
import functools

import numpy as np

import _oracle as O
import _shapes as S

SHAPE = dict(n_data_bits=8, nstartbits=1, nstopbits=1.0)
NFRAMES = 40
SIGMAS = (0.0, 0.1, 0.25, 0.4)
# (meets every condition of test_the_threshold_sweep_is_worth_running at all six rates)
SEED = 11
STREAM_IDS = ["clean", "s0.1", "s0.25", "s0.4", "cut", "noise"]
INF = float("inf")


def rate_mode(rate):
    return S.RATES[S.RATE_IDS.index(rate)][1]


def make_streams(cfg, seed):
    """clean, sigma 0.1 / 0.25 / 0.4, clean and cut B // 3 samples short, noise only (sigma 0.3 over
    30 frames' worth): 40 frames of random words behind 12 idle bits from _shapes.py's keyer."""
    rng = np.random.default_rng(seed)
    segs = S.frame_segments(cfg, S.random_words(rng, cfg, NFRAMES))
    streams = []
    for sigma in SIGMAS + (0.0,):
        x = S.key_fsk(cfg, segs, leading_silence=int(rng.integers(0, 201)))
        if sigma:
            x = (x + rng.normal(0, sigma, x.shape)).astype(np.float32)
        streams.append(x)
    streams[4] = streams[4][: len(streams[4]) - int(cfg.bit_nsamples) // 3]
    streams.append(rng.normal(0, 0.3, 30 * int(cfg.expect_nsamples)).astype(np.float32))
    return streams


@functools.lru_cache(maxsize=None)
def streams_of(rate):
    cfg = O.oracle_config(rate_mode(rate), **SHAPE)
    return make_streams(cfg, [SEED, S.RATE_IDS.index(rate)])


@functools.lru_cache(maxsize=None)
def quartiles(rate):
    """q25, q50, q75 (as float32 values) of the finite frame confidences the oracle finds in the
    sigma = 0.25 and sigma = 0.4 streams at the default options.  Observed values, not interpolated
    ones: a confidence EQUAL to the limit or to the threshold then occurs, which is where `>=`
    (fsk.c:499) and `<=` (minimodem.c:1292) differ from `>` and `<`."""
    cfg = O.oracle_config(rate_mode(rate), **SHAPE)
    x = streams_of(rate)
    c = np.concatenate([O.oracle_rx_stream(cfg, x[i])["frames"]["confidence"] for i in (2, 3)])
    c = c[np.isfinite(c)]
    return tuple(float(np.float32(q)) for q in np.quantile(c, (0.25, 0.5, 0.75), method="nearest"))


PAIR_IDS = ["default", "c0-l0", "c0.5", "l-q50", "l-inf", "c-q25", "c-q50-l-q75", "c-q50-l-inf", "c1e9"]


def pairs(rate):
    """[(id, option kwargs)]: the nine (threshold, limit) pairs of a rate; an option left out is not given"""
    q25, q50, q75 = quartiles(rate)
    kws = [dict(),
           dict(confidence_threshold=0.0, search_limit=0.0),    # limit == 0: the serial selection loop; carrier on noise
           dict(confidence_threshold=0.5),                      # frames out of noise, many refinements
           dict(search_limit=q50),                              # early exit in the middle of the distribution
           dict(search_limit=INF),                              # no early exit, the lattice accepts nothing finite
           dict(confidence_threshold=q25),                      # the limit lifted to the threshold by the config rule
           dict(confidence_threshold=q50, search_limit=q75),    # carrier dropped and re-acquired in mid stream
           dict(confidence_threshold=q50, search_limit=INF),
           dict(confidence_threshold=1e9)]                      # nothing decodes; noconfidence wraps 21 again and again
    return list(zip(PAIR_IDS, kws))


def pair(rate, pid):
    return dict(pairs(rate))[pid]


_refs = {}


def oracle_results(rate, pid, ring=False, extra=()):
    """the oracle's results over the six streams of a rate under one pair, made once per
    (rate, pair, addressing mode, further options)"""
    key = (rate, pid, bool(ring), tuple(extra))
    if key not in _refs:
        ocfg = O.oracle_config(rate_mode(rate), **dict(SHAPE, **dict(pair(rate, pid), **dict(extra))))
        _refs[key] = [O.oracle_rx_stream(ocfg, s, ring_mode=ring) for s in streams_of(rate)]
    return _refs[key]


def outcome(refs):
    """frames and episodes of all six streams, as one hashable value"""
    return tuple((r["frames"].tobytes(), r["episodes"].tobytes()) for r in refs)
