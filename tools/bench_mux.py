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

--iq times the I/Q entry (mifsk_multiplex_iq_batch) on the same shapes, next to the real
entry: one process per shape holds one plan and one pair of inputs (the synthesize_batch rows, and
fm_modulate's I/Q rows of them), and its rounds alternate a window of the real entry with a window of the
I/Q entry, which does 4 ceil(T / L) + 2 or + 4 FMAs per output and channel.  A last step times what stood in
for the I/Q entry before there was one, once: one stream of the first shape as 64 fm_modulate launches at
1.92 MHz with per-row centres, summed in float32 in channel order, beside the one-launch path.  The result
(profiles/multiplex_iq.json) holds all of it, and with --parent FILE ... the real entry's time from plain runs
of another commit's library by its own tool.

    python tools/bench_mux.py --iq [--parent FILE ... --parent-commit HASH] [--out profiles/multiplex_iq.json]

Needs the GPU: there is no other path.
"""
import argparse
import json
import sys
import time

import _benchsteps as B

sys.path.insert(0, B.ROOT)

WORKLOADS = {
    # name: (streams, channels, seconds, input rate, L, complex, pcm16, taps, cutoff, phase steps)
    "iq-1.92M": (8, 64, 10.0, 48000, 40, True, True, 513, 1200.0, 19200),
    "real-192k": (8, 16, 60.0, 48000, 4, False, False, 385, 1200.0, 1920),
}
LIMIT = 300                 # seconds a workload step may take
IQ = "+iq"                  # a step name's tail: both entries, alternating
TODAY = "today"             # the step of --iq that times K fm_modulate launches and their sum


def rows_of(M, torch, ctx, streams, K, secs, fs):
    """streams * K Bell-202 rows from synthesize_batch -> (float32 [streams * K, n], int32 lengths)"""
    cfg = M.rx_config("1200", sample_rate=fs)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    nwords = int(secs * 1200 / 10)                              # 10 bits per word at 1200 baud
    words = torch.randint(0x20, 0x7F, (streams * K, nwords), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    return M.synthesize_batch(ctx, cfg, words, amplitude=0.9 / K)


def centres_of(np, K, P, cx):
    step = P // (K if cx else 2 * K + 2)                        # the channels side by side over the band
    return (np.arange(K) - (K // 2 if cx else -1)) * step


def step_workload(name, rounds, window_ms, preheat_ms):
    import numpy as np
    import torch
    import minimodem_amd as M
    both = name.endswith(IQ)
    streams, K, secs, fs, L, cx, s16, T, cutoff, P = WORKLOADS[name[:-len(IQ)] if both else name]
    ctx = M.Context()
    d, lens = rows_of(M, torch, ctx, streams, K, secs, fs)
    fs_out = fs * L
    r = int(round(1700.0 * P / fs_out))
    plan = M.MuxPlan(ctx, M.channel_taps(T, cutoff, float(fs_out), 2.0 * L), L, centres_of(np, K, P, cx), r, P,
                     complex_output=cx, s16=s16)
    out = M.multiplex(plan, d, nsamples=lens)
    torch.cuda.synchronize()

    def call():
        M.multiplex(plan, d, nsamples=lens, out=out)

    n = int(lens.max())
    nout = (n - 1) * L + T
    outputs = streams * nout
    written = outputs * (2 if s16 else 4) * (2 if cx else 1)

    def figures(k, ms, o, steps_per_tap, bytes_per_sample):
        counts = o["nsamples"].cpu().numpy()
        assert counts.shape == (streams,) and (counts == nout).all(), (counts[:4], nout)
        head = o["rows"][:, :4096].float()
        assert bool(torch.isfinite(head).all()) and float(head.abs().max()) > 0.0
        med = ms["median"]
        fma = outputs * K * (steps_per_tap * -(-T // L) + (4 if cx else 2))
        read = streams * K * n * bytes_per_sample
        return {"launches_per_window": k, "rounds": rounds, "ms": ms,
                "outputs_per_s": outputs / med * 1e3, "fma_per_s": fma / med * 1e3,
                "output_seconds_per_s": outputs / fs_out / med * 1e3,
                "bytes_read": read, "bytes_written": written,
                "read_bytes_per_s": read / med * 1e3, "written_bytes_per_s": written / med * 1e3}

    res = {"workload": {"streams": streams, "channels": K, "samples_per_row": n, "input_rate": fs, "interp": L,
                        "complex": cx, "pcm16": s16, "taps": T, "phase_steps": P, "outputs": outputs},
           "device": ctx.device_name}
    if both:
        # the rows as FM carriers at the narrow rate: what fm_modulate writes is what the I/Q entry reads
        diq = M.fm_modulate(ctx, d, nsamples=lens, deviation=M.fm_step(3000.0, fs), amplitude=0.9 / K)
        out_iq = M.multiplex(plan, diq, nsamples=lens, iq=True)
        torch.cuda.synchronize()

        def call_iq():
            M.multiplex(plan, diq, nsamples=lens, out=out_iq, iq=True)

        (k, ms), (k_iq, ms_iq) = B.alternating_windows([call, call_iq], rounds, window_ms, preheat_ms)
        res.update(figures(k, ms, out, 2, 4))
        res["iq"] = figures(k_iq, ms_iq, out_iq, 4, 8)
        res["iq_over_real"] = ms_iq["median"] / ms["median"]
    else:
        res.update(figures(*B.timed_windows(call, rounds, window_ms, preheat_ms), out, 2, 4))
    plan.close()
    ctx.close()
    print(json.dumps(res))


def step_today():
    """One stream of the first shape, both ways, once each after one untimed pass: K fm_modulate launches at the
    wide rate with per-row centres and the float32 sum in channel order, against fm_modulate at the narrow rate
    and one multiplex(iq=True).  Wall time with a synchronisation at both ends; bytes as torch's allocator
    counts its peak above the audio rows, whose own bytes (at the wide rate for the launches, at the narrow
    rate for the one-launch path) stand beside them."""
    import numpy as np
    import torch
    import minimodem_amd as M
    _streams, K, secs, fs, L, cx, _s16, T, _cutoff, P = WORKLOADS["iq-1.92M"]
    ctx = M.Context()
    fs_out = fs * L
    narrow, lens = rows_of(M, torch, ctx, 1, K, secs, fs)
    wide, wlens = rows_of(M, torch, ctx, 1, K, secs, fs_out)    # the same words as audio at the wide rate
    centres = centres_of(np, K, P, cx)
    plan = M.MuxPlan(ctx, M.channel_taps(T, 12000.0, float(fs_out), float(L)), L, centres, 0, P, complex_output=True)
    amp = 0.9 / K

    def launches():
        total = None
        for k in range(K):
            row = M.fm_modulate(ctx, wide[k:k + 1], nsamples=wlens[k:k + 1], deviation=M.fm_step(3000.0, fs_out),
                                centre=M.fm_step(float(centres[k]) * fs_out / P, fs_out), amplitude=amp)
            total = row if total is None else total + row
        return total

    def one_launch():
        iq = M.fm_modulate(ctx, narrow, nsamples=lens, deviation=M.fm_step(3000.0, fs), amplitude=amp)
        return M.multiplex(plan, iq, nsamples=lens, iq=True)["rows"]

    res = {"workload": {"streams": 1, "channels": K, "seconds": secs, "output_rate": fs_out}, "device": ctx.device_name,
           "audio_bytes": {"launches": wide.numel() * 4, "one_launch": narrow.numel() * 4}}
    for key, fn in (("launches", launches), ("one_launch", one_launch)):
        try:
            fn()                                                # untimed: code objects, the allocator's blocks
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            assert bool(torch.isfinite(got[..., :4096, :]).all())
            res[key] = {"wall_ms": wall, "bytes_peak": torch.cuda.max_memory_allocated() - base,
                        "elements_out": int(got.shape[-2])}
            del got
        except torch.cuda.OutOfMemoryError as e:
            res[key] = {"does_not_fit": str(e)[:200]}
    res["launches"]["launch_count"] = 2 * K - 1
    res["one_launch"]["launch_count"] = 2
    plan.close()
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-10s %9.3f ms  %.3e outputs/s  %.2f TFMA/s (%.0f %% of %.2f)  %.0f s of output per s" % (
        name, r["ms"]["median"], r["outputs_per_s"], r["fma_per_s"] * 1e-12,
        100 * r["share_of_measured_fma64"], peak * 1e-12, r["output_seconds_per_s"]), flush=True)
    if "iq" in r:
        print("%-10s %9.3f ms  I/Q entry: %.4f of the real entry's time (real windows %.3f .. %.3f ms), %.2f TFMA/s" % (
            "", r["iq"]["ms"]["median"], r["iq_over_real"], r["ms"]["min"], r["ms"]["max"], r["iq"]["fma_per_s"] * 1e-12),
            flush=True)


def finish_iq(paths, commit):
    parents = B.add_parents(paths, commit, IQ)

    def finish(result, step):
        peak = result["fma64"]["fma64_per_s"]
        for r in result["workloads"].values():
            r["iq"]["share_of_measured_fma64"] = r["iq"]["fma_per_s"] / peak
        parents(result, step)
        try:
            result[TODAY] = step(TODAY, LIMIT)
        except SystemExit as e:                                 # the last step: the timings above are still written
            result[TODAY] = {"failed": str(e)}
        print("%-10s %s" % (TODAY, json.dumps(result[TODAY])[:600]), flush=True)
    return finish


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--iq", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--parent-commit", default=None)
    mine, rest = ap.parse_known_args()
    sys.argv[1:] = rest
    if mine.iq:
        B.main(__file__, __doc__, "multiplex_iq.json", 600.0,
               "outputs x channels x (2 ceil(T / L) (real rows in) or 4 ceil(T / L) (I/Q rows in) + 2 (real rows out) "
               "or 4 (complex rows out))",
               {name + IQ: w for name, w in WORKLOADS.items()}, LIMIT, step_workload, show, steps={TODAY: step_today},
               finish=finish_iq(mine.parent, mine.parent_commit))
    else:
        B.main(__file__, __doc__, "multiplex.json", 600.0,
               "outputs x channels x (2 ceil(T / L) + 2 (real rows) or 4 (complex rows))",
               WORKLOADS, LIMIT, step_workload, show, steps={TODAY: step_today})
