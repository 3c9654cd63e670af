#!/usr/bin/env python3
"""Time of the channel model (mifsk_impair_batch) on 1024 rows of 480 000 samples (10 s
at 48 kHz), against the measured FP64 vector FMA rate and the HBM rate of the same device, and beside
what the project did before it had the entry: `x += sigma * torch.randn(...)`.

    f32-inplace   float32 rows impaired in place
    s16-s16       PCM16 rows -> PCM16 rows
    f32-s16       float32 rows -> PCM16 rows
    noise         no input rows -> float32 rows (x = 0)
    torch-randn   the same float32 shape: x += sigma * torch.randn(x.shape)  (no entry of the library)
    fma64         tools/ubench/fma64_rate.hip: v_fma_f64 with nothing in the way

Every step is a process of its own under its own time limit; the first one that fails, is killed by a
signal or runs out of time ends the run.  A workload step: a preheat of untimed launches, then `rounds`
windows of K launches on one stream between two device events, K sized so that a window lasts
`window_ms`; the figure is the median of the rounds.  FMAs are counted as the definition has them, the
fused operations only: per PAIR of samples 12 in R, 19 in C and S, and 2 per sample in the element --
17.5 per sample; the pair's 13 other multiplications and additions, its division and its square root
(several instructions each) are not counted.  Bytes are the rows read once plus the rows written once,
and their share is of 8 TB/s.

    python tools/bench_impair.py [--out profiles/impair.json]

Needs the GPU: there is no other path.
"""
import json
import sys

import _benchsteps as B

sys.path.insert(0, B.ROOT)

ROWS, SAMPLES = 1024, 480000
WORKLOADS = {
    # name: (PCM16 in or None for no input rows, PCM16 out, in place)
    "f32-inplace": (False, False, True),
    "s16-s16": (True, True, False),
    "f32-s16": (False, True, False),
    "noise": (None, False, False),
    "torch-randn": (False, False, True),
}
FMA_PER_SAMPLE = 17.5
HBM_BYTES_PER_S = 8e12
LIMIT = 300                 # seconds a workload step may take
SIGMA = 0.1


def step_workload(name, rounds, window_ms, preheat_ms):
    import torch
    import minimodem_amd as M
    in_s16, out_s16, in_place = WORKLOADS[name]
    ctx = M.Context()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = None
    if in_s16 is not None:
        x = torch.rand((ROWS, SAMPLES), generator=g, device="cuda", dtype=torch.float32) - 0.5
        if in_s16:
            x = (x * 32767.0).to(torch.int16)
    out = x if in_place else torch.empty((ROWS, SAMPLES), dtype=torch.int16 if out_s16 else torch.float32, device="cuda")
    torch.cuda.synchronize()

    if name == "torch-randn":
        def call():
            x.add_(SIGMA * torch.randn(x.shape, generator=g, device="cuda", dtype=torch.float32))
    else:
        # gain 0.5 keeps rows that are impaired in place over and over inside the float range
        def call():
            M.impair(ctx, x, seed=7, sigma=SIGMA, gain=0.5, out=out)

    k, ms = B.timed_windows(call, rounds, window_ms, preheat_ms)
    head = out[:, :4096].float()
    assert bool(torch.isfinite(head).all()) and float(head.abs().max()) > 0.0
    med = ms["median"]
    n = ROWS * SAMPLES
    read = 0 if in_s16 is None else n * (2 if in_s16 else 4)
    written = n * (2 if out_s16 else 4)
    fma = 0.0 if name == "torch-randn" else n * FMA_PER_SAMPLE
    res = {"workload": {"rows": ROWS, "samples_per_row": SAMPLES, "pcm16_in": in_s16, "pcm16_out": out_s16,
                        "in_place": in_place, "library_entry": name != "torch-randn"},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds, "ms": ms,
           "samples_per_s": n / med * 1e3, "fma_per_s": fma / med * 1e3,
           "bytes_read": read, "bytes_written": written, "bytes_per_s": (read + written) / med * 1e3,
           "share_of_8TB_per_s": (read + written) / med * 1e3 / HBM_BYTES_PER_S}
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-12s %9.3f ms  %.3e samples/s  %.2f TB/s (%.0f %% of 8)  %.2f TFMA/s (%.0f %% of %.2f)" % (
        name, r["ms"]["median"], r["samples_per_s"], r["bytes_per_s"] * 1e-12, 100 * r["share_of_8TB_per_s"],
        r["fma_per_s"] * 1e-12, 100 * r["share_of_measured_fma64"], peak * 1e-12), flush=True)


def finish(result, _step):
    """the torch.randn path's time beside every workload of the library"""
    base = result["workloads"].get("torch-randn")
    for name, r in result["workloads"].items():
        if base and name != "torch-randn":
            r["torch_randn_ms"] = base["ms"]["median"]
            r["speedup_over_torch_randn"] = base["ms"]["median"] / r["ms"]["median"]


if __name__ == "__main__":
    B.main(__file__, __doc__, "impair.json", 600.0,
           "samples x 17.5: the definition's fused operations (12 in R and 19 in C, S per pair of samples, 2 per "
           "sample in the element); torch-randn: none counted",
           WORKLOADS, LIMIT, step_workload, show, finish=finish)
