"""The planner of mifsk_demod_long_batch (a small batch of long recordings cut in time by one chunk
and one warmup; DESIGN.md "cutting a stream in time", "Several recordings"): host only, no GPU."""
import ctypes as C
import time

import pytest

import minimodem_amd as M
from minimodem_amd import _lib
from _timesplit import _default_warmup, _lattice

GIB4 = 4 << 30


def _raw(cfg, lens, chunk=None, warmup=None, chunks=None, engine=None, flags=0):
    """(rc, list of dicts) of mifsk_time_split_plan_batch_get"""
    lib = _lib.load()
    n = len(lens)
    arr = (C.c_uint64 * max(1, n))(*lens)
    st = (_lib.TimeSplitStats * max(1, n))()
    p = M._time_split_params(chunk, warmup, chunks, engine, False)
    p.flags |= flags
    rc = lib.mifsk_time_split_plan_batch_get(C.byref(cfg), arr, n, C.byref(p), st)
    return rc, [{k: int(getattr(st[m], k)) for k, _ in st[m]._fields_} for m in range(n)]


def _raw_single(cfg, n, chunk=None, warmup=None, chunks=None):
    st = _lib.TimeSplitStats()
    p = M._time_split_params(chunk, warmup, chunks, None, False)
    rc = _lib.load().mifsk_time_split_plan_get(C.byref(cfg), n, C.byref(p), C.byref(st))
    return rc, {k: int(getattr(st, k)) for k, _ in st._fields_}


@pytest.mark.parametrize("mode", ["1200", "rtty", "same", "12000"])
def test_one_stream_is_the_single_planner_field_for_field(mode):
    cfg = M.rx_config(mode)
    W = _default_warmup(cfg)
    lat = _lattice(cfg)
    wmin = 2 * cfg.samplebuf_size
    hour = 3600 * cfg.sample_rate
    lengths = [0, 1, 3, wmin, W // 2, W - 1, W, W + 1, 4 * W - 1, 4 * W, 4 * W + 1, hour, 24 * 30 * hour,
               1 << 40, 1 << 62]
    params = [{}, {"chunks": 64}, {"chunks": 5000}, {"warmup": wmin}, {"warmup": wmin + lat, "chunks": 100},
              {"chunk": 3 * lat}, {"chunk": 1000 * lat, "warmup": wmin}, {"chunk": 50 * lat, "warmup": W}]
    seen_split = seen_error = 0
    for n in lengths:
        for kw in params:
            rc1, one = _raw_single(cfg, n, **kw)
            rcb, many = _raw(cfg, [n], **kw)
            assert rcb == rc1, (mode, n, kw)
            seen_error += rc1 != 0
            if rc1 == 0:
                assert many == [one], (mode, n, kw)
                seen_split += one["nchunks"] > 1
    assert seen_split >= 10 and seen_error >= 1     # (2^62 samples: -EINVAL from both)
    assert M.time_split_plan_batch(cfg, [hour]) == [M.time_split_plan(cfg, hour)]


@pytest.mark.parametrize("mode", ["1200", "rtty", "same"])
@pytest.mark.parametrize("kw", [{}, {"chunks": 300}, {"chunks": 100000}])
def test_mixed_lengths_share_one_chunk_and_one_warmup(mode, kw):
    cfg = M.rx_config(mode)
    W = _default_warmup(cfg)
    hour = 60 * cfg.sample_rate * 60
    lens = [0, W // 2, W + 1, 5 * W, hour, 3 * hour]
    plan = M.time_split_plan_batch(cfg, lens, **kw)
    assert [p["nsamples"] for p in plan] == lens
    assert len({p["chunk"] for p in plan}) == 1 and len({p["warmup"] for p in plan}) == 1
    L = plan[0]["chunk"]
    assert plan[0]["warmup"] == W and L > 0 and L % _lattice(cfg) == 0 and L % 4 == 0
    for n, p in zip(lens, plan):
        assert p["lattice"] == _lattice(cfg)
        assert p["nchunks"] == ((n - W) // L + 1 if n > W else 1), (n, p)
        assert p["samples_speculative"] == 2 * (p["nchunks"] - 1) * W
        assert p["accepted"] == p["rerun"] == p["rounds"] == p["samples_rerun"] == 0
        assert L + W < 2 ** 31
    total = sum(p["nchunks"] for p in plan)
    target = kw.get("chunks", 1024)
    assert total <= target + len(lens)
    assert (total - len(lens)) * W * 4 <= GIB4
    if target <= GIB4 // (W * 4):
        # nothing capped the target: the chip is filled to within the rounding of L to the lattice
        assert total >= min(target, sum(max(0, n - W) for n in lens) // _lattice(cfg)) // 2


def test_the_overlap_budget_caps_the_chunk_count():
    cfg = M.rx_config("1200")
    W = _default_warmup(cfg)
    month = 30 * 24 * 3600 * cfg.sample_rate
    plan = M.time_split_plan_batch(cfg, [month // 8] * 8, chunks=1 << 20)
    total = sum(p["nchunks"] for p in plan)
    assert (total - 8) * W * 4 <= GIB4 and total >= GIB4 // (W * 4) // 2


def test_librarys_choice_leaves_short_streams_whole():
    cfg = M.rx_config("1200")
    W = _default_warmup(cfg)
    lens = [0, 5, W, W + 1, 2 * W, 4 * W - 1]
    plan = M.time_split_plan_batch(cfg, lens)
    assert [p["nchunks"] for p in plan] == [1] * len(lens)
    assert [p["chunk"] for p in plan] == lens                  # the single call: no cut
    assert all(p["samples_speculative"] == 0 for p in plan)
    # one stream as long as 4 W and the batch is cut, the short ones beside it by the same L
    plan = M.time_split_plan_batch(cfg, lens + [4 * W])
    assert plan[-1]["nchunks"] >= 2 and len({p["chunk"] for p in plan}) == 1
    # forced parameters that leave no second chunk anywhere: one chunk each as well
    lat = _lattice(cfg)
    plan = M.time_split_plan_batch(cfg, [2 * lat, 3 * lat], chunk=4 * lat, warmup=2 * cfg.samplebuf_size)
    assert [p["nchunks"] for p in plan] == [1, 1]


def test_error_codes():
    cfg = M.rx_config("1200")
    lat = _lattice(cfg)
    lens = [10 ** 7, 3 * 10 ** 7]
    assert _raw(cfg, lens)[0] == 0
    assert _raw(cfg, lens, chunk=lat + 4)[0] == -22                       # off the lattice
    assert _raw(cfg, lens, warmup=2 * cfg.samplebuf_size - 1)[0] == -22   # the pause could fall outside
    assert _raw(cfg, lens, flags=0x80000)[0] == -22                       # unknown flag
    assert _raw(cfg, lens, flags=_lib.IO_ENGINE_WAVE | _lib.IO_ENGINE_WORKGROUP)[0] == -22
    assert _raw(cfg, lens, flags=_lib.IO_RING_EXACT)[0] == -95            # -ENOTSUP
    assert _raw(cfg, [])[0] == -22                                        # nstreams <= 0
    assert _raw(cfg, [1 << 62])[0] == -22
    # rows of 2^31 samples or more
    assert _raw(cfg, [1 << 45, 10 ** 7], chunks=16)[0] == -22
    lib = _lib.load()
    st = (_lib.TimeSplitStats * 2)()
    arr = (C.c_uint64 * 2)(*lens)
    p = M._time_split_params(None, None, None, None, False)
    assert lib.mifsk_time_split_plan_batch_get(C.byref(cfg), None, 2, C.byref(p), st) == -22
    assert lib.mifsk_time_split_plan_batch_get(C.byref(cfg), arr, 2, C.byref(p), None) == -22
    assert lib.mifsk_time_split_plan_batch_get(C.byref(cfg), arr, -1, C.byref(p), st) == -22
    assert lib.mifsk_time_split_plan_batch_get(C.byref(cfg), arr, 2, None, st) == 0     # the library's choices
    with pytest.raises(ValueError):
        M.time_split_plan_batch(cfg, lens, chunk=lat + 4)
    assert lib.mifsk_abi_version() == 8


def test_256_streams_of_a_month_each_are_planned_at_once():
    """The planner is closed-form.  The host-only planner's 1024 chunks would be rows of 3 * 10^10
    samples for 256 months of audio, and with the default 10 s warm-up the 4 GiB overlap budget
    allows no more than 2236 chunks: rows of 2^31 samples or more are -EINVAL, at once.  With the
    shortest warm-up and 2^16 chunks the batch is planned, at once as well."""
    cfg = M.rx_config("1200")
    month = 30 * 24 * 3600 * cfg.sample_rate
    lens = [month - 1000 * m for m in range(256)]
    t0 = time.perf_counter()
    rc, _ = _raw(cfg, lens)
    W = 2 * cfg.samplebuf_size
    plan = M.time_split_plan_batch(cfg, lens, warmup=W, chunks=1 << 16)
    dt = time.perf_counter() - t0
    assert rc == -22
    assert dt < 0.5, dt
    L = plan[0]["chunk"]
    total = sum(p["nchunks"] for p in plan)
    assert L % _lattice(cfg) == 0 and L + W < 2 ** 31
    assert all(p["nchunks"] == (n - W) // L + 1 for n, p in zip(lens, plan))
    assert (1 << 15) <= total <= (1 << 16) + 256
    assert (total - 256) * W * 4 <= GIB4
