"""mifsk_find_frame_batch over its whole parameter space, against the oracle's fsk_find_frame.

The receive loop hands the search a handful of (try_first, try_max, try_step, limit) tuples; the
entry point takes any.  find_frame_kernel walks the zig-zag in chunks of W_CAP / n_bits candidates
(at most P_CAP), leaves it early -- across chunks -- at the first best that reaches the problem's
own limit, reads zeros beyond `navail`, and must end the scan where the reference does: `t >=
try_max` ends the whole zig-zag while lower candidates remain (fsk.c:477-484).  About 60 problems a
configuration in one call: try_first in {0, 1, mid, try_max - 1} x try_max giving 1, 2, one chunk,
one chunk + 1 and three chunks of candidates, with seeded offsets, steps in {1, 3, larger than
try_max}, limits in {0, the oracle's median confidence over the unlimited searches (an observed
value: some scan ends on a candidate equal to its limit), inf} and navail ending inside the first, a
middle and the last bit window of the first candidate, and beyond the reach.  bits, frame_start and
n_positions are compared as integers, confidence and amplitude as float32 bit patterns."""
import functools

import numpy as np
import pytest

import _oracle as O
import _shapes as S
from test_gpu_frameshapes import _host_lib
from test_gpu_parity import _bits_equal_f32, _uic_stream, gpu  # noqa: F401

W_CAP, P_CAP = 448, 64                  # mifsk_device.h: bit windows / candidates of one chunk
INF = float("inf")
SIGMA = 0.2

# (id, baudmode, options, use_sync_string values, candidates a chunk)
CONFIGS = [
    ("1200", "1200", {}, (0,), 40),                             # 11 windows a frame
    ("12000", "12000", {}, (0,), 40),                           # 4 samples a bit
    ("rtty", "rtty", {}, (0,), 56),
    ("uic-ground", "uic-ground", {}, (0, 1), 9),                # 47 windows
    ("raw64", "1200", dict(binary_raw_nbits=64), (0,), 7),
]
CONFIG_IDS = [c[0] for c in CONFIGS]


def _stream(M, cid, cfg, rng):
    if cid == "uic-ground":
        return _uic_stream(M, cfg, rng, 8, sigma=SIGMA)[0]
    nframes = max(12, 1000 // int(cfg.expect_n_bits))
    x = S.key_fsk(cfg, S.frame_segments(cfg, S.random_words(rng, cfg, nframes), lead_bits=24, tail_bits=16),
                  leading_silence=int(rng.integers(0, 300)))
    return (x + rng.normal(0, SIGMA, x.shape)).astype(np.float32)


def _oracle(plan, ocfg, x, row, limit=None):
    """ofsk_find_frame over the problem's readable samples, zeros behind them -> (conf, bits, ampl, start, n_positions)"""
    lib = O.oracle_lib()
    off, navail = int(row["sample_offset"]), int(row["navail"])
    reach = int(row["try_max"]) + int(ocfg.expect_nsamples) + int(ocfg.bit_nsamples) + 8
    xs = np.concatenate([x[off: off + navail], np.zeros(reach, np.float32)])
    expect = ocfg.expect_sync if row["use_sync_string"] else ocfg.expect_data
    r = O.oracle_find_frame(plan, xs, int(ocfg.expect_nsamples), int(row["try_first"]), int(row["try_max"]),
                            int(row["try_step"]), float(row["search_limit"]) if limit is None else limit, expect)
    return r + (int(lib.ofsk_last_n_positions()), xs)


def grid_candidates(row):
    """positions first + k * step, k of either sign, inside [0, try_max): what a scan that did not
    end at its upward break would visit"""
    first, tmax, step = int(row["try_first"]), int(row["try_max"]), int(row["try_step"])
    return first // step + (tmax - first - 1) // step + 1


@functools.lru_cache(maxsize=None)
def case(cid):
    """-> (cfg, ocfg, samples, problems, [oracle result of each], the median limit)"""
    M = _host_lib()
    _cid, mode, kw, syncs, per_chunk = CONFIGS[CONFIG_IDS.index(cid)]
    cfg, ocfg = M.rx_config(mode, **kw), O.oracle_config(mode, **kw)
    nb, B = int(cfg.expect_n_bits), int(cfg.bit_nsamples)
    assert per_chunk == min(W_CAP // nb, P_CAP)
    rng = np.random.default_rng([133, CONFIG_IDS.index(cid)])
    x = _stream(M, cid, cfg, rng)
    starts = O.oracle_rx_stream(ocfg, x)["frames"]["start"]
    assert len(starts) >= 4
    counts = [1, 2, per_chunk, per_chunk + 1, 3 * per_chunk]
    rows = []
    k = 0
    for use_sync in syncs:
        for rep in range(3):            # (try_first x try_max x try_step in full: 60 problems)
            for ci, count in enumerate(counts):
                for fclass in range(4):
                    sclass = (rep + ci + fclass) % 3
                    step = (1, 3, count + 7)[sclass]
                    tmax = count if sclass == 2 else (count - 1) * step + 1
                    first = min((0, 1, tmax // 2, tmax - 1)[fclass], tmax - 1)
                    last = int(cfg.bit_offset[nb - 1])
                    reach = tmax - 1 + last + B
                    navail = (first + B // 2, first + int(cfg.bit_offset[nb // 2]) + B // 2, first + last + B // 2,
                              reach + 100)[int(rng.integers(0, 4))]
                    # two offsets in three put a frame the oracle's receive loop finds inside the scan's range
                    off = int(rng.integers(0, len(x) - reach - 100))
                    if k % 3:
                        near = int(starts[int(rng.integers(0, len(starts)))]) - int(rng.integers(0, tmax))
                        off = min(max(near, 0), len(x) - reach - 101)
                    rows.append((off, navail, first, tmax, step, (0.0, -1.0, INF)[(rep + fclass + 2 * ci) % 3], use_sync))
                    k += 1
        # eight more, aimed: three chunks upwards from 0 at the median limit, a frame the receive loop finds
        # somewhere in the second or third chunk -- the early exit behind the first chunk
        for j in range(8):
            step = (1, 3)[j & 1]
            tmax = (3 * per_chunk - 1) * step + 1
            reach = tmax - 1 + int(cfg.bit_offset[nb - 1]) + B
            t = step * (per_chunk + 1 + (j * (2 * per_chunk - 3)) // 8)
            off = min(max(int(starts[int(rng.integers(0, len(starts)))]) - t, 0), len(x) - reach - 101)
            rows.append((off, reach + 100, 0, tmax, step, -1.0, use_sync))
    prob = np.array(rows, dtype=M.SEARCH_DTYPE)
    assert np.all(prob["sample_offset"] + prob["navail"] <= len(x))         # nothing is read outside the buffer
    lib = O.oracle_lib()
    plan = lib.ofsk_plan_new(float(ocfg.sample_rate), ocfg.mark_f, ocfg.space_f, ocfg.band_width)
    unlimited = np.array([_oracle(plan, ocfg, x, row, limit=INF)[0] for row in prob], np.float32)
    good = unlimited[np.isfinite(unlimited) & (unlimited > 0)]
    # (an observed value: the problems whose unlimited search ends on it get it for their limit, so that
    # a best candidate EQUAL to the limit ends a scan, fsk.c:499's >=)
    median = np.float32(np.quantile(good, 0.5, method="nearest"))
    prob["search_limit"][(prob["search_limit"] < 0) | (unlimited == median)] = median
    refs = [_oracle(plan, ocfg, x, row) for row in prob]
    lib.ofsk_plan_destroy(plan)
    return cfg, ocfg, x, prob, refs, float(median)


@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_the_problems_reach_every_branch_of_a_search(cid):
    """On the CPU: every level of every factor occurs, try_first x try_max x try_step in full;
    in at least one problem the oracle's scan ends at its upward break with lower candidates left
    (ofsk_last_n_positions below the number of grid positions); a search leaves a later chunk than
    the first early, another runs through all three chunks; and zeros beyond navail matter -- some
    problem's window ends inside the first bit."""
    cfg, ocfg, x, prob, refs, median = case(cid)
    per_chunk = min(W_CAP // int(cfg.expect_n_bits), P_CAP)
    assert len(prob) in (68, 136) and np.isfinite(median) and median > 0
    assert set(prob["try_step"][prob["try_step"] < prob["try_max"]]) >= {1, 3} and np.any(prob["try_step"] > prob["try_max"])
    lims = prob["search_limit"]
    cand = np.array([grid_candidates(row) for row in prob])
    assert np.any(lims == 0) and np.any(np.isinf(lims)) and np.any(lims == np.float32(median))
    for step in (prob["try_step"] == 1, prob["try_step"] == 3, prob["try_step"] > prob["try_max"]):
        assert len(set(prob["try_max"][step])) == 5
        for first in (prob["try_first"] == 0, prob["try_first"] == 1, prob["try_first"] == prob["try_max"] // 2,
                      prob["try_first"] == prob["try_max"] - 1):
            assert len(set(prob["try_max"][step & first])) >= 4             # (try_max == 2: mid == 1 == try_max - 1)
    npos = np.array([r[4] for r in refs])
    unl = np.isinf(lims)
    assert np.any(unl & (npos < cand)), "no scan ended at its upward break"
    assert np.all(npos <= cand) and np.all(npos >= 1)
    assert np.any(unl & (npos == 3 * per_chunk))                        # all three chunks
    # an early exit behind the first chunk (upwards from 0 nothing but the limit ends a scan early)
    assert np.any(~unl & (prob["try_first"] == 0) & (npos > per_chunk) & (npos < cand))
    assert any(r[0] == np.float32(median) == row["search_limit"] for r, row in zip(refs, prob))   # >= at equality
    B = int(cfg.bit_nsamples)
    assert np.any(prob["navail"] < prob["try_first"] + B)
    # (two offsets in three are aimed at a frame: a quarter of the searches at least find one)
    assert sum(r[0] > 0 for r in refs) >= len(prob) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_find_frame_batch_matches_oracle_over_its_parameter_space(gpu, cid):  # noqa: F811
    M, torch, ctx = gpu
    cfg, ocfg, x, prob, refs, _median = case(cid)
    r = M.find_frame_batch(ctx, cfg, torch.from_numpy(x).cuda(), prob)
    for k, (row, got, (conf, bits, ampl, start, npos, _xs)) in enumerate(zip(prob, r, refs)):
        label = (cid, k, row.tolist())
        assert (bits, start) == (int(got["bits"]), int(got["frame_start"])), label
        assert int(got["n_positions"]) == npos, label
        assert _bits_equal_f32([conf, ampl], [got["confidence"], got["amplitude"]]), label


@pytest.mark.gpu
def test_legacy_find_frame_over_the_same_tuples(gpu):  # noqa: F811
    """fsk_find_frame of include/fsk.h with host buffers, a dozen of the 1200-baud tuples (every
    fifth: each class of try_max, of step and of limit is among them)"""
    M, torch, ctx = gpu
    cfg, ocfg, x, prob, refs, _median = case("1200")
    plan = M.LegacyPlan(float(ocfg.sample_rate), ocfg.mark_f, ocfg.space_f, ocfg.band_width)
    picked = list(range(0, 60, 5))
    assert len(set(int(prob[k]["try_max"]) for k in picked)) >= 5 and len(set(float(prob[k]["search_limit"]) for k in picked)) == 3
    for k in picked:
        row, (conf, bits, ampl, start, _npos, xs) = prob[k], refs[k]
        got = plan.find_frame(xs, int(ocfg.expect_nsamples), int(row["try_first"]), int(row["try_max"]),
                              int(row["try_step"]), float(row["search_limit"]), ocfg.expect_data)
        assert (got[1], got[3]) == (bits, start), (k, row.tolist())
        assert _bits_equal_f32([got[0], got[2]], [conf, ampl]), (k, row.tolist())
    plan.close()
