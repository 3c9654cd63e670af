#!/usr/bin/env python3
"""Time of the carrier survey (mifsk_detect_carrier_batch) on five workloads, against
the measured FP64 vector FMA rate of the same device and the 8 TB/s read roofline.

    1200          1024 rows x 480 000 samples, float32, window = hop = 40, bands and magnitudes only
    1200-spectrum the same with every band's magnitude written
    1200-pcm16    the same from PCM16 rows
    rtty          64 rows x 60 s (2 880 000 samples), window = hop = 1056
    1200-hop8     the first workload with hop 8 (five-fold overlap)
    legacy        LegacyPlan.detect_carrier (the drop-in fsk_detect_carrier: one window per call, host
                  memory) in a host loop over 256 of the first workload's windows, wall time
    fma64         tools/ubench/fma64_rate.hip: v_fma_f64 with nothing in the way

Every step is a process of its own under its own time limit; the first one that fails, is killed by a
signal or runs out of time ends the run.  A workload step: rows made on the device (a tone per row
plus noise), 0.3 s of untimed launches, then `rounds` windows of K launches on one stream between two
device events, K sized so that a window lasts `window_ms`; the figure is the median of the rounds.
FMAs are counted as windows x bands x samples x 2 (re and im), bytes as the rows read once plus the
outputs written once.

    python tools/bench_carrier.py [--out profiles/carrier_survey.json]

Needs the GPU: there is no other path.
"""
import json
import statistics
import sys
import time

import _benchsteps as B

sys.path.insert(0, B.ROOT)

HBM_PEAK = 8.0e12
WORKLOADS = {
    # name: (mode, rows, samples, hop (0: window), pcm16, spectrum)
    "1200": ("1200", 1024, 480000, 0, False, False),
    "1200-spectrum": ("1200", 1024, 480000, 0, False, True),
    "1200-pcm16": ("1200", 1024, 480000, 0, True, False),
    "rtty": ("rtty", 64, 2880000, 0, False, False),
    "1200-hop8": ("1200", 1024, 480000, 8, False, False),
}
LIMITS = {"workload": 240, "legacy": 120}       # seconds


def make_rows(torch, cfg, rows, n, pcm16):
    """a tone in a band of its own per row, on for the second half of the row, plus noise"""
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    t = torch.arange(n, device="cuda", dtype=torch.float32)
    band = torch.randint(2, int(cfg.nbands) - 2, (rows, 1), generator=g, device="cuda").to(torch.float32)
    w = 2.0 * 3.141592653589793 * band * float(cfg.band_width) / float(cfg.sample_rate)
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 27) // n)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        x[r0:r1] = 0.5 * torch.sin(w[r0:r1] * t[None, :]) * (t[None, :] >= n // 2) \
            + 0.02 * torch.randn((r1 - r0, n), generator=g, device="cuda")
    if pcm16:
        x = (x * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    return x


def step_workload(name, rounds, window_ms, preheat_ms):
    import torch
    import minimodem_amd as M
    mode, rows, n, hop, pcm16, spectrum = WORKLOADS[name]
    ctx = M.Context()
    cfg = M.rx_config(mode)
    window = M.carrier_window_default(cfg)
    hop = hop or window
    d = make_rows(torch, cfg, rows, n, pcm16)
    nwin = M.carrier_windows(n, window, hop)
    out = M.carrier_survey(ctx, cfg, d, window=window, hop=hop, spectrum=spectrum)
    torch.cuda.synchronize()

    def call():
        M.carrier_survey(ctx, cfg, d, window=window, hop=hop, spectrum=spectrum, out=out)

    k, ms = B.timed_windows(call, rounds, window_ms, preheat_ms)
    band = out["band"]
    found = int((band >= 0).sum())
    assert int((band == -2).sum()) == 0 and found > rows * nwin // 4, (found, rows * nwin)
    med = ms["median"]
    windows = rows * nwin
    fma = windows * int(cfg.nbands) * window * 2
    read = rows * n * (2 if pcm16 else 4)
    written = windows * 8 + (windows * int(cfg.nbands) * 4 if spectrum else 0)
    res = {"workload": {"mode": mode, "rows": rows, "samples_per_row": n, "window": window, "hop": hop,
                        "pcm16": pcm16, "spectrum": spectrum, "nbands": int(cfg.nbands), "fftsize": int(cfg.fftsize),
                        "windows": windows, "windows_with_a_band": found},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds,
           "ms": ms,
           "windows_per_s": windows / med * 1e3, "fma_per_s": fma / med * 1e3,
           "bytes_read": read, "bytes_written": written,
           "read_bytes_per_s": read / med * 1e3, "written_bytes_per_s": written / med * 1e3,
           "share_of_8TBps_read": read / med * 1e3 / HBM_PEAK}
    ctx.close()
    print(json.dumps(res))


def step_legacy():
    import numpy as np
    import torch
    import minimodem_amd as M
    cfg = M.rx_config("1200")
    x = make_rows(torch, cfg, 1, 480000, False)[0].cpu().numpy()
    wins = [np.ascontiguousarray(x[240000 + 40 * i:240040 + 40 * i]) for i in range(256)]
    plan = M.LegacyPlan(float(cfg.sample_rate), cfg.mark_f, cfg.space_f, cfg.band_width)
    for w in wins[:16]:
        plan.detect_carrier(w, 0.001)
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        bands = [plan.detect_carrier(w, 0.001) for w in wins]
        secs.append(time.perf_counter() - t0)
    plan.close()
    med = statistics.median(secs)
    print(json.dumps({"windows": 256, "seconds": {"median": med, "min": min(secs), "max": max(secs)},
                      "windows_per_s": 256 / med, "windows_with_a_band": sum(b >= 0 for b in bands)}))


def show(name, r, peak):
    print("%-14s %8.3f ms  %.3e windows/s  %.2f TFMA/s (%.0f %% of %.2f)  read %.2f TB/s" % (
        name, r["ms"]["median"], r["windows_per_s"], r["fma_per_s"] * 1e-12,
        100 * r["share_of_measured_fma64"], peak * 1e-12, r["read_bytes_per_s"] * 1e-12), flush=True)


def finish(result, step):
    legacy = step("legacy", LIMITS["legacy"])
    result["legacy_host_loop"] = legacy
    if "1200" in result["workloads"]:
        result["batched_over_legacy_windows_per_s"] = result["workloads"]["1200"]["windows_per_s"] / legacy["windows_per_s"]
        assert result["batched_over_legacy_windows_per_s"] > 1.0, "the batched call must be faster per window"


if __name__ == "__main__":
    B.main(__file__, __doc__, "carrier_survey.json", 300.0, "windows x bands x samples x 2",
           WORKLOADS, LIMITS["workload"], step_workload, show, steps={"legacy": step_legacy}, finish=finish)
