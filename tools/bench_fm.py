#!/usr/bin/env python3
"""Time of the FM stage (mifsk_fm_demod_batch, mifsk_fm_modulate_batch) on 1024 rows of
480 000 complex samples (10 s at 48 kHz), against the measured FP64 vector FMA rate and the HBM rate of the
same device, and beside what a user did before the library had the entries.

    demod-f32     float32 I/Q rows -> float32 audio rows
    demod-s16     PCM16 I/Q rows -> float32 audio rows
    mod-f32       float32 audio rows -> float32 I/Q rows
    mod-s16       float32 audio rows -> PCM16 I/Q rows
    torch-angle   the discriminator in torch: torch.angle(z[:, 1:] * z[:, :-1].conj()) * gain / (2 pi)
    torch-polar   the modulator in torch: torch.polar(1, 2 pi cumsum(x * deviation)), float32 throughout
    fma64         tools/ubench/fma64_rate.hip: v_fma_f64 with nothing in the way

Every step is a process of its own under its own time limit; the first one that fails, is killed by a
signal or runs out of time ends the run.  A workload step: a preheat of untimed launches, then `rounds`
windows of K launches on one stream between two device events, K sized so that a window lasts
`window_ms`; the figure is the median of the rounds.  f64 operations are counted as the definition has
them, a division as one: the discriminator 26 per sample (4 in re and im, 21 in the angle -- one division
and 12 fused among them -- and the gain); the modulator 31 (3 in the step, made in two of the three
launches, 23 in C and S, 2 for the amplitude).  Bytes are what the launches read and write once each: 12 and
8 per sample for the discriminator, 16 and 12 for the modulator (its input rows are read twice); their
share is of 8 TB/s.

    python tools/bench_fm.py [--out profiles/fm.json]

Needs the GPU: there is no other path.
"""
import json
import math
import sys
import time

import _benchsteps as B

sys.path.insert(0, B.ROOT)

ROWS, SAMPLES = 1024, 480000
WORKLOADS = {
    # name: (entry, PCM16 side, f64 operations per sample, bytes per sample)
    "demod-f32": ("demod", False, 26, 12),
    "demod-s16": ("demod", True, 26, 8),
    "mod-f32": ("mod", False, 31, 16),
    "mod-s16": ("mod", True, 31, 12),
    "torch-angle": ("demod", False, 0, 12),
    "torch-polar": ("mod", False, 0, 12),
}
HBM_BYTES_PER_S = 8e12
LIMIT = 300                 # seconds a workload step may take
DEV, GAIN = 3000.0 / 48000.0, 48000.0 / 3000.0


def step_workload(name, rounds, window_ms, preheat_ms):
    import torch
    import minimodem_amd as M
    entry, s16, ops, nbytes = WORKLOADS[name]
    ctx = M.Context()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.rand((ROWS, SAMPLES), generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0
    if entry == "demod":
        # a modulated batch: what the discriminator meets
        iq = M.fm_modulate(ctx, x, deviation=DEV, s16=s16)
        del x
        out = torch.empty((ROWS, SAMPLES), dtype=torch.float32, device="cuda")
        if name == "torch-angle":
            z = torch.view_as_complex(iq)

            def call():
                return torch.angle(z[:, 1:] * z[:, :-1].conj()) * (GAIN / (2.0 * math.pi))
        else:
            def call():
                return M.fm_demod(ctx, iq, gain=GAIN, out=out)
    else:
        out = torch.empty((ROWS, SAMPLES, 2), dtype=torch.int16 if s16 else torch.float32, device="cuda")
        if name == "torch-polar":
            one = torch.ones((ROWS, SAMPLES), dtype=torch.float32, device="cuda")

            def call():
                return torch.polar(one, torch.cumsum(x * DEV, dim=1) * (2.0 * math.pi))
        else:
            def call():
                return M.fm_modulate(ctx, x, deviation=DEV, out=out)
    torch.cuda.synchronize()

    k, ms = B.timed_windows(call, rounds, window_ms, preheat_ms)
    head = call()[:, :4096]
    head = torch.view_as_real(head) if head.is_complex() else head.float()
    assert bool(torch.isfinite(head).all()) and float(head.abs().max()) > 0.0
    med = ms["median"]
    n = ROWS * SAMPLES
    res = {"workload": {"rows": ROWS, "complex_samples_per_row": SAMPLES, "entry": entry, "pcm16": s16,
                        "library_entry": not name.startswith("torch-")},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds, "ms": ms,
           "samples_per_s": n / med * 1e3, "fma_per_s": n * ops / med * 1e3, "f64_ops_per_sample": ops,
           "f64_ops_per_s": n * ops / med * 1e3, "bytes_per_sample": nbytes, "bytes_per_s": n * nbytes / med * 1e3,
           "share_of_8TB_per_s": n * nbytes / med * 1e3 / HBM_BYTES_PER_S}
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-12s %9.3f ms  %.3e samples/s  %.2f TB/s (%.0f %% of 8)  %.2f T f64 op/s (%.0f %% of the %.2f TFMA/s measured)" % (
        name, r["ms"]["median"], r["samples_per_s"], r["bytes_per_s"] * 1e-12, 100 * r["share_of_8TB_per_s"],
        r["f64_ops_per_s"] * 1e-12, 100 * r["share_of_measured_fma64"], peak * 1e-12), flush=True)


def finish(result, _step):
    """the day of the run, and the torch path's time beside every workload of the library"""
    result["date"] = time.strftime("%Y-%m-%d")
    for name, r in result["workloads"].items():
        base = result["workloads"].get("torch-angle" if r["workload"]["entry"] == "demod" else "torch-polar")
        if base and r["workload"]["library_entry"]:
            r["torch_ms"] = base["ms"]["median"]
            r["speedup_over_torch"] = base["ms"]["median"] / r["ms"]["median"]


if __name__ == "__main__":
    B.main(__file__, __doc__, "fm.json", 600.0,
           "f64 operations as the definition has them, a division as one: 26 per sample in the discriminator, 31 in "
           "the modulator; the torch paths: none counted",
           WORKLOADS, LIMIT, step_workload, show, finish=finish)
