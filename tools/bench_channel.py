#!/usr/bin/env python3
"""Time of the channelizer (mifsk_channelize_batch) on two workloads, against the
measured FP64 vector FMA rate of the same device.

    real-48k    64 real float32 rows x 60 s at 48 kHz, 16 channels, 385 taps, D = 1
    iq-1.92M    8 complex PCM16 rows x 10 s at 1.92 MHz, 64 channels, 513 taps, D = 40
    fma64       tools/ubench/fma64_rate.hip: v_fma_f64 with nothing in the way

Every step is a process of its own under its own time limit; the first one that fails, is killed by a
signal or runs out of time ends the run.  A workload step: rows of noise made on the device, a
preheat of untimed launches, then `rounds` windows of K launches on one stream between two device
events, K sized so that a window lasts `window_ms`; the figure is the median of the rounds.  FMAs
are counted as outputs x taps x 2 (real rows) or x 4 (complex rows), bytes as the rows read once
plus the outputs written once.

    python tools/bench_channel.py [--out profiles/channelize.json]

--iq times the I/Q entry (mifsk_channelize_iq_batch) on the same shapes, next to the real
entry: one process per shape holds one plan and one input, and its rounds alternate a window of the real
entry with a window of the I/Q entry.  The result (profiles/channelize_iq.json) holds both times, their
ratio and the windows' spread; --parent FILE ... adds the real entry's time from results that the tool
of another commit wrote on the same machine (its own profiles/channelize.json), and what this commit's
real entry takes against each.

    python tools/bench_channel.py --iq [--parent FILE ... --parent-commit HASH] [--out profiles/channelize_iq.json]

Needs the GPU: there is no other path.
"""
import argparse
import json
import sys

import _benchsteps as B

sys.path.insert(0, B.ROOT)

WORKLOADS = {
    # name: (rows, elements per row, input rate, complex, pcm16, channels, taps, cutoff, decimation, phase steps)
    "real-48k": (64, 2880000, 48000.0, False, False, 16, 385, 400.0, 1, 4800),
    "iq-1.92M": (8, 19200000, 1920000.0, True, True, 64, 513, 9000.0, 40, 19200),
}
LIMIT = 300                 # seconds a workload step may take
IQ = "+iq"                  # a step name's tail: both entries, alternating


def step_workload(name, rounds, window_ms, preheat_ms):
    import numpy as np
    import torch
    import minimodem_amd as M
    both = name.endswith(IQ)
    rows, n, fs, cx, s16, K, T, cutoff, D, P = WORKLOADS[name[:-len(IQ)] if both else name]
    ctx = M.Context()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    shape = (rows, n, 2) if cx else (rows, n)
    if s16:
        d = torch.randint(-8000, 8000, shape, generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    else:
        d = torch.empty(shape, dtype=torch.float32, device="cuda")
        for r in range(rows):
            d[r] = 0.25 * torch.randn(shape[1:], generator=g, device="cuda")
    centres = (np.arange(K) - (K // 2 if cx else -2)) * (P // (K if cx else 4 * K))
    plan = M.ChannelPlan(ctx, M.channel_taps(T, cutoff, fs, 1.0 if cx else 2.0), D, centres, 17, P,
                         complex_input=cx, s16=s16)
    out = M.channelize(plan, d)
    torch.cuda.synchronize()

    def call():
        M.channelize(plan, d, out=out)

    nout = M.carrier_windows(n, T, D)
    outputs = rows * K * nout
    fma = outputs * T * (4 if cx else 2)
    read = rows * n * (2 if s16 else 4) * (2 if cx else 1)

    def figures(k, ms, o, bytes_per_output):
        counts = o["nsamples"].cpu().numpy()
        assert counts.shape == (rows * K,) and (counts == nout).all(), (counts[:4], nout)
        assert bool(torch.isfinite(o["rows"][::max(1, rows * K // 8), :4096]).all())
        med, written = ms["median"], outputs * bytes_per_output
        return {"launches_per_window": k, "rounds": rounds, "ms": ms,
                "outputs_per_s": outputs / med * 1e3, "fma_per_s": fma / med * 1e3,
                "input_seconds_per_s": rows * n / fs / med * 1e3,
                "bytes_read": read, "bytes_written": written,
                "read_bytes_per_s": read / med * 1e3, "written_bytes_per_s": written / med * 1e3}

    res = {"workload": {"rows": rows, "elements_per_row": n, "input_rate": fs, "complex": cx, "pcm16": s16,
                        "channels": K, "taps": T, "decimation": D, "phase_steps": P, "outputs": outputs},
           "device": ctx.device_name}
    if both:
        out_iq = M.channelize(plan, d, iq=True)
        torch.cuda.synchronize()
        # the I plane of the I/Q entry is the real entry's output, here too
        assert torch.equal(out_iq["rows"][::max(1, rows * K // 8), :4096, 0], out["rows"][::max(1, rows * K // 8), :4096])

        def call_iq():
            M.channelize(plan, d, out=out_iq, iq=True)

        (k, ms), (k_iq, ms_iq) = B.alternating_windows([call, call_iq], rounds, window_ms, preheat_ms)
        res.update(figures(k, ms, out, 4))
        res["iq"] = figures(k_iq, ms_iq, out_iq, 8)
        res["iq_over_real"] = ms_iq["median"] / ms["median"]
    else:
        res.update(figures(*B.timed_windows(call, rounds, window_ms, preheat_ms), out, 4))
    plan.close()
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-10s %9.3f ms  %.3e outputs/s  %.2f TFMA/s (%.0f %% of %.2f)  %.0f s of input per s" % (
        name, r["ms"]["median"], r["outputs_per_s"], r["fma_per_s"] * 1e-12,
        100 * r["share_of_measured_fma64"], peak * 1e-12, r["input_seconds_per_s"]), flush=True)
    if "iq" in r:
        print("%-10s %9.3f ms  I/Q entry: %.4f of the real entry's time (real windows %.3f .. %.3f ms)" % (
            "", r["iq"]["ms"]["median"], r["iq_over_real"], r["ms"]["min"], r["ms"]["max"]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--iq", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--parent-commit", default=None)
    mine, rest = ap.parse_known_args()
    sys.argv[1:] = rest
    if mine.iq:
        B.main(__file__, __doc__, "channelize_iq.json", 600.0, "outputs x taps x 2 (real rows) or 4 (complex rows)",
               {name + IQ: w for name, w in WORKLOADS.items()}, LIMIT, step_workload, show,
               finish=B.add_parents(mine.parent, mine.parent_commit, IQ))
    else:
        B.main(__file__, __doc__, "channelize.json", 600.0, "outputs x taps x 2 (real rows) or 4 (complex rows)",
               WORKLOADS, LIMIT, step_workload, show)
