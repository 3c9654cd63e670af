"""Every frame shape, 1 to 64 bit windows a frame, through the product, against the oracle.

The receive kernels choose their code by the bit length and by the number of bit windows of a
frame (expect_n_bits; n_bits on the device): frames per lane pass and per LATTICE block, the size
of the magnitude buffer, nbits_magic behind udiv_magic, the grid lattice (lock_advance ==
(n_bits - 1) * B depends on the stop bits), which shared-segment plans of a long-window scan are
valid (J * n_bits <= SEGW_MAX; two lanes a window up to 32 windows), the generic confidence pass,
the extraction of up to 64 data bits.  test_gpu_bitlengths.py runs every bit length with 10
windows a frame; this file runs 187 shapes -- --binary-raw 1 .. 64, and 5 / 7 / 8 data bits x 0 ..
20 start bits x 0 .. 3 stop bits -- at the six rates of _shapes.RATES, each the smallest that
reaches a kernel family.  Five streams per configuration from the numpy keyer of _shapes.py
(clean, sigma 0.03, sigma 0.2, cut B // 3 short, noise only) through the three variants of
test_gpu_parity.py, everything compared with oracle_rx_stream as that file does.

(_shapes.SEED: with about three seeds in four some configuration with 3 or 0.5 stop bits has a
sigma = 0.03 stream in which the ORACLE locks on fewer than the three frames the CPU test below
asks of every configuration.  This one was taken for the oracle's frame counts alone.)"""
import functools

import numpy as np
import pytest

import _oracle as O
import _shapes as S
from test_gpu_parity import VARIANTS, VARIANT_IDS, _bits_equal_f32, assert_stream_equal, gpu, run_gpu_streams  # noqa: F401

FRAME_SYNC, FRAME_REFINED = 2, 4


@functools.lru_cache(maxsize=None)
def _host_lib():
    import minimodem_amd as M
    return M


def both_configs(mode, kw, opts=None):
    M = _host_lib()
    allkw = dict(kw, **(opts or {}))
    return M.rx_config(mode, **allkw), O.oracle_config(mode, **allkw)


@functools.lru_cache(maxsize=1)
def _batch(rate, gid):
    """[(label, cfg, ocfg, streams, {ring: oracle results})] of one group of shapes.  One group is
    kept: its variants run one after the other, and the oracle runs once per addressing mode."""
    out = []
    for label, mode, kw, seed in S.configs(rate, dict(S.GROUPS)[gid]):
        cfg, ocfg = both_configs(mode, kw)
        out.append((label, cfg, ocfg, S.make_streams(cfg, seed)[1], {}))
    return out


def oracle_results(ocfg, streams, refs, ring):
    if ring not in refs:
        refs[ring] = [O.oracle_rx_stream(ocfg, s, ring_mode=ring) for s in streams]
    return refs[ring]


@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_every_shape_is_accepted_and_the_streams_are_worth_decoding(rate):
    """The input side, on the CPU: all 187 shapes are accepted by the product's and the oracle's
    configuration alike, with the same expect_n_bits (every value from 1 to 64 occurs),
    bit_nsamples, frame_nsamples and expect string; and what keeps the sweep honest -- the oracle
    finds at least 3 frames in every configuration's sigma = 0.03 stream, and at least one REFINED
    frame in every group of shapes among the sigma = 0.2 streams."""
    B = dict((r, b) for r, _m, b in S.RATES)[rate]
    seen = set()
    for gid, shapes in S.GROUPS:
        refined = 0
        for label, mode, kw, seed in S.configs(rate, shapes):
            cfg, ocfg = both_configs(mode, kw)
            for field in ("expect_n_bits", "bit_nsamples", "frame_nsamples", "expect_nsamples", "expect_data", "n_data_bits"):
                assert getattr(cfg, field) == getattr(ocfg, field), (label, field)
            assert cfg.expect_n_bits == S.shape_n_bits(kw) and cfg.bit_nsamples == B, label
            seen.add(int(cfg.expect_n_bits))
            streams = S.make_streams(cfg, seed)[1]
            assert len(O.oracle_rx_stream(ocfg, streams[1])["frames"]) >= 3, label
            refined += int(np.count_nonzero(O.oracle_rx_stream(ocfg, streams[2])["frames"]["flags"] & FRAME_REFINED))
        assert refined >= 1, (rate, gid)
    assert seen == set(range(1, 65))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("gid", S.GROUP_IDS)
@pytest.mark.parametrize("rate", S.RATE_IDS)
def test_frame_shapes_match_oracle(gpu, rate, gid, variant):  # noqa: F811
    M, torch, ctx = gpu
    engine, ring = variant
    total = 0
    batch = _batch(rate, gid)
    for label, cfg, ocfg, streams, refs in batch:
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine=engine, ring=ring)
        for i, ref in enumerate(oracle_results(ocfg, streams, refs, ring)):
            assert_stream_equal(res, i, ref, label)
            total += len(ref["frames"])
    # (the oracle's counts on the CPU: at least 16 frames a configuration in every group at every
    # rate; four keyed streams of at least three frames each is what is asked here)
    assert total >= 4 * 3 * len(batch)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_raw_frames_of_43_to_64_bits_at_240_baud_through_the_tile(gpu, variant):  # noqa: F811
    """The combination the planner tool's old invariant excluded and no test had launched: at
    200 samples per bit the SCAN slab of a frame of 43 and more windows no longer fits a wave's
    share of LDS and the flat wavefront plan is the tiled instantiation below kTileMinBit (with a
    direct lattice, and no shared segments: those are planned from 256 samples on); RING
    addressing runs demod_wave_kernel<4, -2> there.  Named here besides the sweep: the first,
    the last and the 47-bit frame of that range."""
    M, torch, ctx = gpu
    engine, ring = variant
    for n in (43, 47, 64):
        (label, mode, kw, seed), = S.configs("240", [dict(binary_raw_nbits=n)])
        cfg, ocfg = both_configs(mode, kw)
        p = M.demod_plan(ctx, cfg, S.NSTREAMS, engine=engine, ring_exact=ring)
        if engine == "wave":
            assert ("demod_wave_kernel<4, -2>" if ring else "demod_wave_kernel<10, -1>") in p["kernel"], p
        streams = S.make_streams(cfg, seed)[1]
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine=engine, ring=ring)
        total = 0
        for i, s in enumerate(streams):
            ref = O.oracle_rx_stream(ocfg, s, ring_mode=ring)
            assert_stream_equal(res, i, ref, label)
            total += len(ref["frames"])
        assert total >= 12


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("rate", ["240", "b300.4"])
def test_three_stop_bits_end_the_loop_where_the_reference_does(gpu, rate, variant):  # noqa: F811
    """The reference sizes its buffer without the stop bits (minimodem.c:1056-1060): with 3 of them
    a frame is as long as half of it, the advance behind a frame found late in its search is
    longer than what is valid, and `if (advance > samples_nvalid) break` (minimodem.c:1150-1152)
    ends the loop in mid stream -- the cut stream of 240/5-3-3 stops after 8 of its 16 frames.  The
    workgroup engine's plain instantiations took `advance <= N - base` for that test and decoded
    on (16 frames against the oracle's 8; 240 and 159.8 baud, 5-3-3 and 7-1-3: what the sweep
    found); such configurations now run its resumable instantiation, which carries the file
    position.  The failing configurations by name, besides their place in the sweep."""
    M, torch, ctx = gpu
    engine, ring = variant
    stopped = 0
    for shape in (dict(n_data_bits=5, nstartbits=3, nstopbits=3.0), dict(n_data_bits=7, nstartbits=1, nstopbits=3.0)):
        (label, mode, kw, seed), = S.configs(rate, [shape])
        cfg, ocfg = both_configs(mode, kw)
        assert cfg.try_max[1] + cfg.frame_nsamples - cfg.nsamples_overscan > cfg.samplebuf_size // 2
        if engine == "workgroup":
            p = M.demod_plan(ctx, cfg, S.NSTREAMS, engine=engine)
            assert p["engine"] == "workgroup" and p["kernel"].endswith(", true>"), p
        words, streams = S.make_streams(cfg, seed)
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine=engine, ring=ring)
        for i, s in enumerate(streams):
            ref = O.oracle_rx_stream(ocfg, s, ring_mode=ring)
            assert_stream_equal(res, i, ref, label)
            # (a keyed stream the loop left early: fewer than half of its frames, none in its second half)
            stopped += i < 4 and len(ref["frames"]) <= len(words) // 2 and \
                all(int(f["start"]) < len(s) // 2 for f in ref["frames"])
    assert stopped >= 1


@functools.lru_cache(maxsize=1)
def _option_batch(rate):
    """[(label, cfg, ocfg, words, sync frames, [clean, sigma 0.2], {ring: oracle results})]"""
    ri = S.RATE_IDS.index(rate)
    out = []
    for k, (kw, opts, nsync) in enumerate(S.OPTIONS):
        cfg, ocfg = both_configs(S.RATES[ri][1], kw, opts)
        words, streams = S.make_streams(cfg, [S.SEED, ri, S.OPTION_SEED + k], sync_frames=nsync)
        out.append(("%s/%s" % (rate, S.OPTION_IDS[k]), cfg, ocfg, words, nsync, [streams[0], streams[2]], {}))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("rate", S.OPTION_RATES)
def test_frame_options_match_oracle(gpu, rate, variant):  # noqa: F811
    """What is done with a frame's bits once it is found, at shapes the named modes do not have:
    --msb-first on 1 .. 64 data bits (the reversal accumulates in 32 bits above 32, as the
    reference's does), --invert-start-stop, --inverted-freqs, and a sync byte -- SAME's 0xAB on
    raw 8, 0x16 on 8-N-1, one above 2^32 on raw 40 -- behind 16 frames of which the keyer sends
    it: frames equal to it carry MIFSK_FRAME_SYNC and are absent from the bytes."""
    M, torch, ctx = gpu
    engine, ring = variant
    nsynced = 0
    for label, cfg, ocfg, words, nsync, streams, refs in _option_batch(rate):
        res = run_gpu_streams(M, torch, ctx, cfg, streams, engine=engine, ring=ring)
        for i, ref in enumerate(oracle_results(ocfg, streams, refs, ring)):
            assert_stream_equal(res, i, ref, label)
            nf = int(res["nframes"][i])
            fr = res["frames"][i, :nf]
            synced = (fr["flags"] & FRAME_SYNC) != 0
            if nsync:
                assert np.array_equal(synced, fr["bits"] == np.uint64(cfg.sync_byte)), label
                assert int(res["nbytes"][i]) == nf - int(synced.sum()), label
                got = bytes(int(b) & 0xFF for b in fr["bits"][~synced])
                assert res["bytes"][i, :int(res["nbytes"][i])].tobytes() == got, label
                nsynced += int(synced.sum()) if i == 0 else 0
            else:
                assert not synced.any(), label
        # the clean stream of a shape with start bits carries what was sent.  (Not asked of the
        # raw shapes: nothing marks where their frames begin, the search after a lock may settle
        # a bit off -- the oracle does the same; nor with --msb-first: the keyer sends bit 0 first.)
        if cfg.nstartbits and not cfg.msb_first:
            got = set(int(b) for b in res["bits"][0, :int(res["nframes"][0])])
            assert sum(1 for w in words[nsync:] if w in got) >= len(words[nsync:]) - 2, label
    # the 16 sync frames of 8-N-1 are found where they are; those of the raw shapes mostly are
    assert nsynced >= 16, nsynced


RAW_FIND = [1, 2, 7, 9, 11, 33, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("n", RAW_FIND, ids=["raw%d" % n for n in RAW_FIND])
def test_find_frame_batch_with_raw_expect_strings(gpu, n):  # noqa: F811
    """mifsk_find_frame_batch with expect strings of 1 .. 64 data bits at 40 samples per bit: 7
    to 448 candidates of a chunk at the workgroup engine's W_CAP, the geometries of
    test_find_frame_batch_with_47_bit_expect_string (the last: 67 candidates, more than a chunk)."""
    M, torch, ctx = gpu
    (label, mode, kw, seed), = S.configs("1200", [dict(binary_raw_nbits=n)])
    cfg, ocfg = both_configs(mode, kw)
    assert cfg.expect_n_bits == n and cfg.bit_nsamples == 40
    rng = np.random.default_rng(seed + [7513])
    x = S.key_fsk(cfg, S.frame_segments(cfg, S.random_words(rng, cfg, max(8, 480 // n)), lead_bits=24, tail_bits=16),
                  leading_silence=int(rng.integers(0, 300)))
    x = (x + rng.normal(0, 0.05, x.shape)).astype(np.float32)
    offs = rng.integers(0, len(x) - int(cfg.expect_nsamples) - 200, size=48)
    geos = [(0, 120, 40, 2.3), (40, 100, 33, 2.3), (40, 100, 12, float("inf")), (0, 120, 15, float("inf")),
            (0, 200, 3, float("inf"))]
    prob = np.zeros(len(offs) * len(geos), M.SEARCH_DTYPE)
    k = 0
    for off in offs:
        for first, tmax, step, limit in geos:
            prob[k] = (int(off), len(x) - int(off), first, tmax, step, limit, 0)
            k += 1
    r = M.find_frame_batch(ctx, cfg, torch.from_numpy(x).cuda(), prob)
    lib = O.oracle_lib()
    plan = lib.ofsk_plan_new(float(ocfg.sample_rate), ocfg.mark_f, ocfg.space_f, ocfg.band_width)
    xp = np.concatenate([x, np.zeros(int(ocfg.expect_nsamples) + 400, np.float32)])
    hits = 0
    for row, got in zip(prob, r):
        conf, bits, ampl, start = O.oracle_find_frame(
            plan, xp[int(row["sample_offset"]):], int(ocfg.expect_nsamples), int(row["try_first"]),
            int(row["try_max"]), int(row["try_step"]), float(row["search_limit"]), ocfg.expect_data)
        assert (bits, start) == (int(got["bits"]), int(got["frame_start"]))
        assert _bits_equal_f32([conf, ampl], [got["confidence"], got["amplitude"]])
        assert int(got["n_positions"]) == lib.ofsk_last_n_positions()
        hits += conf > 0
    lib.ofsk_plan_destroy(plan)
    assert hits >= 5


def sweep_coverage(M, ctx):
    """{variant id: {(rate, kernel, lattice_mode): [(expect_n_bits, frames_per_block)]}}"""
    cover = {}
    for (engine, ring), vid in zip(VARIANTS, VARIANT_IDS):
        seen = cover.setdefault(vid, {})
        for rate in S.RATE_IDS:
            for _label, mode, kw, _seed in S.configs(rate):
                p = M.demod_plan(ctx, M.rx_config(mode, **kw), S.NSTREAMS, engine=engine, ring_exact=ring)
                assert p["engine"] == engine
                kernel = p["kernel"][p["kernel"].index("demod"):]
                seen.setdefault((rate, kernel, p["lattice_mode"]), []).append((S.shape_n_bits(kw), p["frames_per_block"]))
    return cover


@pytest.mark.gpu
def test_the_shape_sweep_reaches_every_instantiation(gpu):  # noqa: F811
    """What the sweep's launches are (mifsk_demod_plan at the sweep's batch size; nothing is
    launched here): the plans that only frame shapes other than 8-N-1's reach.  tests/README.md
    records the whole table."""
    M, torch, ctx = gpu
    cover = sweep_coverage(M, ctx)
    every = set(range(1, 65))
    nbits = lambda vid, key: set(n for n, _f in cover[vid].get(key, []))            # noqa: E731
    flat, ringv, wg = cover["wave-flat"], cover["wave-ring"], cover["workgroup-flat"]
    # the tiled kernel with a direct lattice, and below the bit length from which the planner prefers it
    tiled_direct = [k for k in flat if "demod_wave_kernel<10, -1>" in k[1] and k[2] == 2]
    assert set(k[0] for k in tiled_direct) == {"240", "b300.4", "45.45"}
    assert nbits("wave-flat", ("240", "demod_wave_kernel<10, -1>", 2)) == set(range(43, 65))
    assert not any("demod_wave_kernel<10, -1>" in k[1] for k in flat if k[0] in ("1200", "b40.4", "12000"))
    # the narrow direct instantiation under RING, long frames
    assert nbits("wave-ring", ("45.45", "demod_wave_kernel<4, -2>", 0)) == set(range(8, 65))
    assert nbits("wave-ring", ("240", "demod_wave_kernel<4, -2>", 0)) == set(range(43, 65))
    assert min(nbits("wave-ring", ("b300.4", "demod_wave_kernel<4, -2>", 0))) == 30
    # the workgroup engine without a slab
    assert nbits("workgroup-flat", ("45.45", "demod_kernel<false, 0, 3>", 0)) == set(range(35, 65))
    # the linear instantiations of both engines at every number of windows
    assert nbits("wave-flat", ("1200", "demod_wave_kernel<10, 10>", 1)) == every
    assert nbits("wave-flat", ("12000", "demod_wave_kernel<10, 0>", 1)) == every
    assert nbits("workgroup-flat", ("1200", "demod_kernel<true, 10, 2>", 1)) == every
    assert nbits("workgroup-flat", ("12000", "demod_kernel<true, 0, 3>", 1)) == every
    fpb = set(f for v in wg.values() for _n, f in v)
    assert min(f for f in fpb if f) <= 8 and 64 in fpb and len(fpb) >= 20, sorted(fpb)
    assert set(f for v in flat.values() for _n, f in v) >= {16, 32, 64}
    for vid in VARIANT_IDS:
        assert sum(len(v) for v in cover[vid].values()) == len(S.RATES) * len(S.SHAPES)
    assert all(k[2] == 0 for k in ringv)
