"""Every bit length from 3 to 320 samples through the product, against the oracle.

The receive kernels choose their code by the bit length B and by how the bit offsets round
(fill_devcfg in csrc/mifsk_plan.cpp: linear / grid lattice, the skew pad word, div_magic, the
tail of the last group of 16, the short last tile step, one shared-segment plan per B >= 256,
the slow path of store4_skewed at B = 3).  The other parity tests run about two dozen bit
lengths; this file runs all of them at 48 kHz, at three rates per length: spb = B exactly (the
multiples of 4 are linear-grid), B - 0.3 and B + 0.4 (nothing is linear).  The batches are tiny
on purpose: the point is the shapes, not the load.

Per configuration five streams seeded by B -- clean, sigma 0.03, sigma 0.2 (refinements and
rescans), one cut B // 3 samples short of its end, one of noise only -- each through the three
variants of test_gpu_parity.py, everything compared with oracle_rx_stream as that file does."""
import functools

import numpy as np
import pytest

import _oracle as O
from test_gpu_parity import VARIANTS, VARIANT_IDS, assert_stream_equal, gpu, run_gpu_streams  # noqa: F401

B_MIN, B_MAX = 3, 320
RATES = [("exact", 0.0), ("minus0.3", -0.3), ("plus0.4", 0.4)]
RATE_IDS = [r[0] for r in RATES]
ACCEPTED = {"exact": 318, "minus0.3": 317, "plus0.4": 318}
RANGES = [(lo, min(lo + 15, B_MAX)) for lo in range(B_MIN, B_MAX + 1, 16)]
RANGE_IDS = ["B%d-%d" % r for r in RANGES]
NSTREAMS = 5
SEED = 29


def bit_lengths(rate, lo=B_MIN, hi=B_MAX):
    """the (B, baudmode string) of every configuration of a rate in [lo, hi]: all of them but
    (3, 2.7), which mifsk_rx_config_init refuses"""
    delta = dict(RATES)[rate]
    return [(B, repr(48000.0 / (B + delta))) for B in range(lo, hi + 1) if not (B == 3 and delta < 0)]


@functools.lru_cache(maxsize=None)
def _host_lib():
    import minimodem_amd as M
    return M


def make_streams(cfg, ocfg, B, rate):
    """-> (payload, the five streams of one configuration), seeded by B and the rate.
    (SEED: around B = 120 .. 131 the Bell-103 tones are hardly a bin apart and how many frames
    the REFERENCE finds in 16 bytes depends on the bytes -- with about nine seeds in ten some
    configuration's sigma = 0.03 stream has fewer than the three frames the CPU test below asks of
    every configuration.  This one was taken for the oracle's frame counts alone.)"""
    M = _host_lib()
    rng = np.random.default_rng([SEED, RATE_IDS.index(rate), B])
    payload = rng.integers(32, 127, size=16, dtype=np.uint8)
    streams = []
    for sigma in (0.0, 0.03, 0.2, 0.0):
        x = M.synthesize(cfg, payload, leading_silence=int(rng.integers(0, 201)))
        if sigma:
            x = (x + rng.normal(0, sigma, x.shape)).astype(np.float32)
        streams.append(x)
    streams[3] = streams[3][: len(streams[3]) - B // 3]            # ends inside a bit window
    streams.append(rng.normal(0, 0.3, 6 * int(ocfg.expect_nsamples)).astype(np.float32))
    return payload.tobytes(), streams


@functools.lru_cache(maxsize=1)
def _batch(span, rate):
    """[(B, mode, cfg, ocfg, streams, {ring: oracle results})] of one range of bit lengths.  One
    range is kept: the variants of a (range, rate) run one after the other, and the oracle runs
    once per addressing mode for them all."""
    M = _host_lib()
    out = []
    for B, mode in bit_lengths(rate, *span):
        cfg, ocfg = M.rx_config(mode), O.oracle_config(mode)
        out.append((B, mode, cfg, ocfg, make_streams(cfg, ocfg, B, rate)[1], {}))
    return out


def oracle_results(ocfg, streams, refs, ring):
    if ring not in refs:
        refs[ring] = [O.oracle_rx_stream(ocfg, s, ring_mode=ring) for s in streams]
    return refs[ring]


@pytest.mark.parametrize("rate", RATE_IDS)
def test_every_bit_length_is_accepted_and_the_streams_are_worth_decoding(rate):
    """The input side, on the CPU: every B but (3, 2.7) is accepted with bit_nsamples == B by
    the product's and the oracle's configuration alike; and what keeps the sweep honest -- the
    oracle finds at least 3 frames in every configuration's sigma = 0.03 stream, and decodes
    the clean stream's payload exactly in at least 90 % of the configurations (the Bell-103
    tones sit too close to the baud rate around B = 120 .. 131, and the shortest bits lose
    frames to the search's start-up)."""
    M = _host_lib()
    assert len(bit_lengths(rate)) == ACCEPTED[rate]
    if rate == "minus0.3":
        with pytest.raises(ValueError):
            M.rx_config(repr(48000.0 / 2.7))
        with pytest.raises(ValueError):
            O.oracle_config(repr(48000.0 / 2.7))
    decoded = 0
    for B, mode in bit_lengths(rate):
        cfg, ocfg = M.rx_config(mode), O.oracle_config(mode)
        assert cfg.bit_nsamples == B == ocfg.bit_nsamples, (B, mode)
        payload, streams = make_streams(cfg, ocfg, B, rate)
        assert len(O.oracle_rx_stream(ocfg, streams[1])["frames"]) >= 3, (B, mode)
        decoded += payload in O.oracle_rx_stream(ocfg, streams[0])["bytes"]
    assert decoded >= 0.9 * ACCEPTED[rate], (decoded, ACCEPTED[rate])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("rate", RATE_IDS)
@pytest.mark.parametrize("span", RANGES, ids=RANGE_IDS)
def test_bit_lengths_match_oracle(gpu, span, rate, variant):  # noqa: F811
    M, torch, ctx = gpu
    engine, ring = variant
    total = 0
    for B, mode, cfg, ocfg, streams, refs in _batch(span, rate):
        assert cfg.bit_nsamples == B
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine=engine, ring=ring)
        for i, ref in enumerate(oracle_results(ocfg, streams, refs, ring)):
            assert_stream_equal(res, i, ref, "B=%d %s" % (B, mode))
            total += len(ref["frames"])
    assert total >= 3 * 3 * (span[1] - span[0])


def lattice_kind(kernel):
    """the second template argument of a wavefront-engine kernel name: 'tiled' (-1), 'direct'
    (-2) or 'linear' (0, or the NQ of a resident instantiation)"""
    args = kernel[kernel.index("<") + 1: kernel.rindex(">")].split(",")
    nq = int(args[1])
    return {-1: "tiled", -2: "direct"}.get(nq, "linear")


def sweep_coverage(M, ctx):
    """{variant id: {(kernel, lattice_mode): [bit lengths, all three rates]}}"""
    cover = {}
    for (engine, ring), vid in zip(VARIANTS, VARIANT_IDS):
        seen = cover.setdefault(vid, {})
        for rate in RATE_IDS:
            for B, mode in bit_lengths(rate):
                p = M.demod_plan(ctx, M.rx_config(mode), NSTREAMS, engine=engine, ring_exact=ring)
                assert p["engine"] == engine
                seen.setdefault((p["kernel"], p["lattice_mode"]), []).append(B)
    return cover


@pytest.mark.gpu
def test_the_sweep_reaches_every_lattice_kind(gpu):  # noqa: F811
    """What the sweep's launches are (mifsk_demod_plan at the sweep's batch size): on the
    wavefront engine with flat addressing the tiled, the linear and the direct instantiations
    all occur -- tiled exactly from the tile threshold of 256 samples per bit on, linear only at
    exact multiples of 4 samples per bit.  tests/README.md records the whole table."""
    M, torch, ctx = gpu
    cover = sweep_coverage(M, ctx)
    flat = cover["wave-flat"]
    kinds = {}
    for (kernel, _mode), bs in flat.items():
        assert "demod_wave_kernel<" in kernel
        kinds.setdefault(lattice_kind(kernel), []).extend(bs)
    assert set(kinds) == {"tiled", "linear", "direct"}, sorted(flat)
    assert min(kinds["tiled"]) == 256 and set(kinds["tiled"]) == set(range(256, B_MAX + 1))
    assert all(B % 4 == 0 for B in kinds["linear"])
    for vid in VARIANT_IDS:
        assert sum(len(bs) for bs in cover[vid].values()) == sum(ACCEPTED.values())
