"""The planner of mifsk_demod_long (one long recording cut in time; DESIGN.md "cutting a stream
in time"): host only, no GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import minimodem_amd as M
from minimodem_amd import _lib
from _timesplit import _lattice

MODES = ["1200", "300", "rtty", "tdd", "same", "12000", "uic-train", "callerid"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seconds", [30, 600, 3600])
def test_library_choice_is_on_the_lattice_and_covers_the_recording(mode, seconds):
    cfg = M.rx_config(mode)
    n = seconds * cfg.sample_rate + 12345
    p = M.time_split_plan(cfg, n)
    assert p["nsamples"] == n
    assert p["lattice"] == _lattice(cfg)
    if mode == "rtty":
        # an odd half buffer (9513): the lattice is four of them, so rows stay 16-byte aligned
        assert (cfg.samplebuf_size // 2) % 2 == 1 and p["lattice"] == 4 * (cfg.samplebuf_size // 2)
    assert p["warmup"] >= 2 * cfg.samplebuf_size
    if p["nchunks"] == 1:
        assert n < 4 * p["warmup"], p
        return
    L, W, K = p["chunk"], p["warmup"], p["nchunks"]
    assert L % p["lattice"] == 0 and L % 4 == 0          # rows start 16-byte aligned
    assert (K - 1) * L + W <= n < K * L + W                # the last chunk runs to the end
    assert K <= 1024 + 1
    assert p["samples_speculative"] == 2 * (K - 1) * W


def test_forced_chunk_and_warmup_are_kept():
    cfg = M.rx_config("1200")
    lat = _lattice(cfg)
    W = 2 * cfg.samplebuf_size
    p = M.time_split_plan(cfg, 100 * lat + 7, chunk=3 * lat, warmup=W)
    assert p["chunk"] == 3 * lat and p["warmup"] == W
    assert p["nchunks"] == (100 * lat + 7 - W) // (3 * lat) + 1


def test_short_recording_is_one_chunk():
    cfg = M.rx_config("1200")
    p = M.time_split_plan(cfg, 5 * cfg.sample_rate)
    assert p["nchunks"] == 1 and p["chunk"] == 5 * cfg.sample_rate
    # forced parameters that leave no second chunk: the single call as well
    lat = _lattice(cfg)
    p = M.time_split_plan(cfg, 2 * lat, chunk=4 * lat, warmup=2 * cfg.samplebuf_size)
    assert p["nchunks"] == 1


def _rc(cfg, n, **kw):
    lib = _lib.load()
    st = _lib.TimeSplitStats()
    p = M._time_split_params(kw.get("chunk"), kw.get("warmup"), None, kw.get("engine"), False)
    p.flags |= kw.get("flags", 0)
    return lib.mifsk_time_split_plan_get(C.byref(cfg), n, C.byref(p), C.byref(st))


def test_invalid_parameters():
    cfg = M.rx_config("1200")
    lat = _lattice(cfg)
    n = 10 ** 7
    assert _rc(cfg, n) == 0
    assert _rc(cfg, n, chunk=lat + 4) == -22                      # off the lattice
    assert _rc(cfg, n, warmup=2 * cfg.samplebuf_size - 1) == -22  # the pause could fall outside
    assert _rc(cfg, n, flags=0x80000) == -22                      # unknown flag
    assert _rc(cfg, n, flags=_lib.IO_ENGINE_WAVE | _lib.IO_ENGINE_WORKGROUP) == -22
    assert _rc(cfg, n, flags=_lib.IO_RING_EXACT) == -95           # -ENOTSUP
    with pytest.raises(ValueError):
        M.time_split_plan(cfg, n, chunk=lat + 4)


_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LONG_PLANS = r"""
import sys
sys.path.insert(0, %r)
import minimodem_amd as M
for mode in ("1200", "same", "rtty"):
    cfg = M.rx_config(mode)
    for hours in (3, 6, 8, 24, 24 * 30):
        n = int(hours * 3600 * cfg.sample_rate)
        p = M.time_split_plan(cfg, n)
        print(mode, n, p["nchunks"], p["chunk"], p["warmup"])
    for n in (1 << 40, (1 << 62) - 1):
        try:
            p = M.time_split_plan(cfg, n)
            print(mode, n, p["nchunks"], p["chunk"], p["warmup"])
        except ValueError as e:
            print(mode, n, "error", str(e).split(": ")[-1])
"""


def test_library_choice_for_recordings_of_hours_to_months_returns_promptly():
    """The planner's choice is closed-form: a day (and a month) at 48 kHz is planned at once, keeps
    the chip full and the warm-up overlap of the row copy within 4 GiB; lengths whose rows would
    pass 2^31 samples are -EINVAL.  (Run in a child process: a planner that loops must fail the
    test, not hang it.)"""
    r = subprocess.run([sys.executable, "-c", _LONG_PLANS % _ROOT], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert len(lines) == 21
    for mode, n, *rest in lines:
        cfg = M.rx_config(mode)
        n = int(n)
        if rest[0] == "error":
            assert rest[1] == "-22" and n >= 1 << 40, (mode, n, rest)
            continue
        K, L, W = (int(v) for v in rest)
        assert K >= 512, (mode, n, K)                       # still the chip's worth of chunks
        assert (K - 1) * L + W <= n < K * L + W
        assert L % _lattice(cfg) == 0 and L + W < 2 ** 31
        assert (K - 1) * W * 4 <= 4 << 30                   # the overlap of the row copy
    # a day and a month are planned, not refused
    assert all(rest[0] != "error" for mode, n, *rest in lines if int(n) <= 30 * 24 * 3600 * 48000)
