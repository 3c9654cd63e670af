#!/usr/bin/env python3
"""Time of the multiplexer (mifsk_multiplex_batch) on two workloads, against the
measured FP64 vector FMA rate of the same device: the shapes of tools/bench_channel.py, run in the
other direction.

    iq-1.92M    8 streams x 64 Bell-202 rows x 10 s at 48 kHz -> complex PCM16 at 1.92 MHz (L = 40), 513 taps
    real-192k   8 streams x 16 Bell-202 rows x 60 s at 48 kHz -> real float32 at 192 kHz (L = 4), 385 taps
    fma64       tools/ubench/fma64_rate.hip: v_fma_f64 with nothing in the way

Every step is a process of its own under its own time limit; the first one that fails, is killed by a
signal or runs out of time ends the run.  A workload step: rows made on the device by
synthesize_batch, a preheat of untimed launches, then `rounds` windows of K launches on one stream
between two device events, K sized so that a window lasts `window_ms`; the figure is the median of
the rounds.  FMAs are counted as the definition has them for rows that are all inside:
outputs x channels x (2 ceil(T / L) + 2) for real rows, + 4 for complex ones; bytes as the rows read
once plus the outputs written once.

    python tools/bench_mux.py [--out profiles/multiplex.json]

Needs the GPU: there is no other path.
"""
import json
import sys

import _benchsteps as B

sys.path.insert(0, B.ROOT)

WORKLOADS = {
    # name: (streams, channels, seconds, input rate, L, complex, pcm16, taps, cutoff, phase steps)
    "iq-1.92M": (8, 64, 10.0, 48000, 40, True, True, 513, 1200.0, 19200),
    "real-192k": (8, 16, 60.0, 48000, 4, False, False, 385, 1200.0, 1920),
}
LIMIT = 300                 # seconds a workload step may take


def step_workload(name, rounds, window_ms, preheat_ms):
    import numpy as np
    import torch
    import minimodem_amd as M
    streams, K, secs, fs, L, cx, s16, T, cutoff, P = WORKLOADS[name]
    ctx = M.Context()
    cfg = M.rx_config("1200", sample_rate=fs)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    nwords = int(secs * 1200 / 10)                              # 10 bits per word at 1200 baud
    words = torch.randint(0x20, 0x7F, (streams * K, nwords), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    d, lens = M.synthesize_batch(ctx, cfg, words, amplitude=0.9 / K)
    fs_out = fs * L
    r = int(round(1700.0 * P / fs_out))
    step = P // (K if cx else 2 * K + 2)                        # the channels side by side over the band
    centres = (np.arange(K) - (K // 2 if cx else -1)) * step
    plan = M.MuxPlan(ctx, M.channel_taps(T, cutoff, float(fs_out), 2.0 * L), L, centres, r, P,
                     complex_output=cx, s16=s16)
    out = M.multiplex(plan, d, nsamples=lens)
    torch.cuda.synchronize()

    def call():
        M.multiplex(plan, d, nsamples=lens, out=out)

    k, ms = B.timed_windows(call, rounds, window_ms, preheat_ms)
    n = int(lens.max())
    nout = (n - 1) * L + T
    counts = out["nsamples"].cpu().numpy()
    assert counts.shape == (streams,) and (counts == nout).all(), (counts[:4], nout)
    head = out["rows"][:, :4096].float()
    assert bool(torch.isfinite(head).all()) and float(head.abs().max()) > 0.0
    med = ms["median"]
    outputs = streams * nout
    fma = outputs * K * (2 * -(-T // L) + (4 if cx else 2))
    read = streams * K * n * 4
    written = outputs * (2 if s16 else 4) * (2 if cx else 1)
    res = {"workload": {"streams": streams, "channels": K, "samples_per_row": n, "input_rate": fs, "interp": L,
                        "complex": cx, "pcm16": s16, "taps": T, "phase_steps": P, "outputs": outputs},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds,
           "ms": ms,
           "outputs_per_s": outputs / med * 1e3, "fma_per_s": fma / med * 1e3,
           "output_seconds_per_s": outputs / fs_out / med * 1e3,
           "bytes_read": read, "bytes_written": written,
           "read_bytes_per_s": read / med * 1e3, "written_bytes_per_s": written / med * 1e3}
    plan.close()
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-10s %9.3f ms  %.3e outputs/s  %.2f TFMA/s (%.0f %% of %.2f)  %.0f s of output per s" % (
        name, r["ms"]["median"], r["outputs_per_s"], r["fma_per_s"] * 1e-12,
        100 * r["share_of_measured_fma64"], peak * 1e-12, r["output_seconds_per_s"]), flush=True)


if __name__ == "__main__":
    B.main(__file__, __doc__, "multiplex.json", 600.0,
           "outputs x channels x (2 ceil(T / L) + 2 (real rows) or 4 (complex rows))",
           WORKLOADS, LIMIT, step_workload, show)
