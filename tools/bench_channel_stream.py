#!/usr/bin/env python3
"""Time of one feed of a channel stream (mifsk_channel_stream_feed) on the two workloads
of DESIGN.md 4.14 cut into pieces of 100 ms, against what the batch entry takes in the same process:

    iq-1.92M/100ms   8 complex PCM16 rows, pieces of 192 000 elements, 64 channels, 513 taps, D = 40
    real-48k/100ms   64 real float32 rows, pieces of 4 800 elements, 16 channels, 385 taps, D = 1

    feed   ChannelStream.feed of the piece, in steady state (the tails full: every feed does the same work)
    lone   channelize on the piece alone: the same FMAs less the seam's outputs, the floor
    cat    what a caller without the stream does: torch.cat of a kept tail of T - 1 elements and the piece,
           then channelize (right sums, wrong phase unless the cut is a multiple of D P): the cost to beat

One process per workload holds one plan, one piece and the three outputs; its rounds alternate a window of
each of the three (tools/_benchsteps.py: K launches on one stream between two device events, K sized so
that a window lasts `window_ms`, the median of the rounds).  FMAs are counted as outputs x taps x 2 (real
rows) or x 4 (complex rows).

    python tools/bench_channel_stream.py [--out profiles/channel_stream.json]

Needs the GPU: there is no other path.
"""
import json
import sys

import _benchsteps as B

sys.path.insert(0, B.ROOT)

WORKLOADS = {
    # name: (rows, elements per piece, input rate, complex, pcm16, channels, taps, cutoff, decimation, phase steps)
    "iq-1.92M/100ms": (8, 192000, 1920000.0, True, True, 64, 513, 9000.0, 40, 19200),
    "real-48k/100ms": (64, 4800, 48000.0, False, False, 16, 385, 400.0, 1, 4800),
}
LIMIT = 300                 # seconds a workload step may take


def step_workload(name, rounds, window_ms, preheat_ms):
    import numpy as np
    import torch
    import minimodem_amd as M
    rows, n, fs, cx, s16, K, T, cutoff, D, P = WORKLOADS[name]
    ctx = M.Context()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    shape = (rows, n, 2) if cx else (rows, n)
    if s16:
        d = torch.randint(-8000, 8000, shape, generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    else:
        d = 0.25 * torch.randn(shape, generator=g, device="cuda")
    centres = (np.arange(K) - (K // 2 if cx else -2)) * (P // (K if cx else 4 * K))
    plan = M.ChannelPlan(ctx, M.channel_taps(T, cutoff, fs, 1.0 if cx else 2.0), D, centres, 17, P,
                         complex_input=cx, s16=s16)
    cs = M.ChannelStream(plan, rows)
    tail = d[:, n - (T - 1):]                                       # the caller's kept tail: a view
    out_feed = cs.feed(d)
    out_feed = cs.feed(d, out=out_feed)                             # steady state from here on
    out_lone = M.channelize(plan, d)
    out_cat = M.channelize(plan, torch.cat([tail, d], dim=1))
    torch.cuda.synchronize()
    per_feed = M.channel_stream_outputs(T, D, n, n)
    assert per_feed == M.channel_stream_outputs(T, D, 5 * n, n)
    # the second feed's outputs are the cat's (same window sums) up to the phase: same counts
    assert (out_feed["nsamples"] == per_feed).all() and (out_cat["nsamples"] == M.carrier_windows(n + T - 1, T, D)).all()

    def feed():
        cs.feed(d, out=out_feed)

    def lone():
        M.channelize(plan, d, out=out_lone)

    def cat():
        M.channelize(plan, torch.cat([tail, d], dim=1), out=out_cat)

    (k, ms), (k_lone, ms_lone), (k_cat, ms_cat) = B.alternating_windows([feed, lone, cat], rounds, window_ms, preheat_ms)
    assert bool(torch.isfinite(out_feed["rows"][::max(1, rows * K // 8), :per_feed]).all())
    outputs = rows * K * per_feed
    fma = outputs * T * (4 if cx else 2)
    res = {"workload": {"rows": rows, "elements_per_piece": n, "input_rate": fs, "complex": cx, "pcm16": s16,
                        "channels": K, "taps": T, "decimation": D, "phase_steps": P, "outputs_per_feed": outputs},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds, "ms": ms,
           "fma_per_s": fma / ms["median"] * 1e3, "input_seconds_per_s": n / fs / ms["median"] * 1e3,
           "lone": {"launches_per_window": k_lone, "ms": ms_lone, "outputs": rows * K * M.carrier_windows(n, T, D)},
           "cat": {"launches_per_window": k_cat, "ms": ms_cat, "outputs": rows * K * M.carrier_windows(n + T - 1, T, D)},
           "feed_over_lone": ms["median"] / ms_lone["median"], "feed_over_cat": ms["median"] / ms_cat["median"],
           "seen": int(cs.seen()[0])}
    cs.close()
    plan.close()
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-15s feed %8.4f ms  lone %8.4f ms (x %.3f)  cat %8.4f ms (x %.3f)  %.2f TFMA/s (%.0f %% of %.2f)  %.0f s of "
          "input per s and row" % (name, r["ms"]["median"], r["lone"]["ms"]["median"], r["feed_over_lone"],
                                   r["cat"]["ms"]["median"], r["feed_over_cat"], r["fma_per_s"] * 1e-12,
                                   100 * r["share_of_measured_fma64"], peak * 1e-12, r["input_seconds_per_s"]), flush=True)


if __name__ == "__main__":
    B.main(__file__, __doc__, "channel_stream.json", 600.0, "outputs x taps x 2 (real rows) or 4 (complex rows)",
           WORKLOADS, LIMIT, step_workload, show)
