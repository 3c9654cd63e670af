#!/usr/bin/env python3
"""Time of one feed of a multiplexer stream (mifsk_mux_stream_feed) on the two workloads of
DESIGN.md 4.15 cut into pieces of 100 ms, against what the batch entry takes in the same process:

    iq-1.92M/100ms    8 streams x 64 rows, pieces of 4 800 samples at 48 kHz -> complex PCM16 at 1.92 MHz (L = 40), 513 taps
    real-192k/100ms   8 streams x 16 rows, pieces of 4 800 samples at 48 kHz -> real float32 at 192 kHz (L = 4), 385 taps

    feed   MuxStream.feed of the piece, in steady state (the tails full: every feed does the same work)
    lone   multiplex on the piece alone, the unchanged batch entry: the floor
    cat    what a caller without the stream does: torch.cat of a kept tail of H samples per row and the piece,
           then multiplex (right sums, wrong phase unless the cut is a multiple of P / gcd(L, P)): the cost to beat

One process per workload holds one plan, one piece and the three outputs; its rounds alternate a window of
each of the three (tools/_benchsteps.py: K launches on one stream between two device events, K sized so
that a window lasts `window_ms`, the median of the rounds).  FMAs are counted as in tools/bench_mux.py, for the
feed's k L outputs per stream.

With --parent-tree DIR the batch path is timed too, by tools/bench_mux.py's own workload steps, once from DIR
(a built checkout of another commit: its tool, its package, its library) and once from this tree, in turn for
each workload in this run: the medians may differ by no more than the larger of the two runs' own min-max
spreads.

    python tools/bench_mux_stream.py [--parent-tree DIR --parent-commit HASH] [--out profiles/mux_stream.json]

Needs the GPU: there is no other path.
"""
import argparse
import json
import os
import subprocess
import sys

import _benchsteps as B

sys.path.insert(0, B.ROOT)

WORKLOADS = {
    # name: (streams, channels, samples per piece, input rate, L, complex, pcm16, taps, cutoff, phase steps)
    "iq-1.92M/100ms": (8, 64, 4800, 48000, 40, True, True, 513, 1200.0, 19200),
    "real-192k/100ms": (8, 16, 4800, 48000, 4, False, False, 385, 1200.0, 1920),
}
BATCH = ("iq-1.92M", "real-192k")       # tools/bench_mux.py's workloads
LIMIT = 300                 # seconds a workload step may take


def step_workload(name, rounds, window_ms, preheat_ms):
    import numpy as np
    import torch
    import minimodem_amd as M
    import bench_mux as Bm
    streams, K, n, fs, L, cx, s16, T, cutoff, P = WORKLOADS[name]
    ctx = M.Context()
    d, lens = Bm.rows_of(M, torch, ctx, streams, K, 1.2 * n / fs, fs)
    d = d[:, :n].contiguous()                                       # whole rows: every row n samples
    assert d.shape == (streams * K, n) and int(lens.min()) >= n
    fs_out = fs * L
    H = M.mux_stream_drain(T, L)
    plan = M.MuxPlan(ctx, M.channel_taps(T, cutoff, float(fs_out), 2.0 * L), L, Bm.centres_of(np, K, P, cx),
                     int(round(1700.0 * P / fs_out)), P, complex_output=cx, s16=s16)
    ms_obj = M.MuxStream(plan, streams)
    tail = d[:, n - H:]                                             # the caller's kept tail: a view
    out_feed = ms_obj.feed(d)
    out_feed = ms_obj.feed(d, out=out_feed)                         # steady state from here on
    out_lone = M.multiplex(plan, d)
    out_cat = M.multiplex(plan, torch.cat([tail, d], dim=1))
    torch.cuda.synchronize()
    assert (out_feed["nsamples"] == n * L).all() and (out_lone["nsamples"] == (n - 1) * L + T).all()
    assert (out_cat["nsamples"] == (n + H - 1) * L + T).all()

    def feed():
        ms_obj.feed(d, out=out_feed)

    def lone():
        M.multiplex(plan, d, out=out_lone)

    def cat():
        M.multiplex(plan, torch.cat([tail, d], dim=1), out=out_cat)

    (k, ms), (k_lone, ms_lone), (k_cat, ms_cat) = B.alternating_windows([feed, lone, cat], rounds, window_ms, preheat_ms)
    assert bool(torch.isfinite(out_feed["rows"][:, :4096].float()).all())
    outputs = streams * n * L
    fma = outputs * K * (2 * -(-T // L) + (4 if cx else 2))
    res = {"workload": {"streams": streams, "channels": K, "samples_per_piece": n, "input_rate": fs, "interp": L,
                        "complex": cx, "pcm16": s16, "taps": T, "phase_steps": P, "tail_samples": H,
                        "outputs_per_feed": outputs},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds, "ms": ms,
           "fma_per_s": fma / ms["median"] * 1e3, "output_seconds_per_s": n / fs / ms["median"] * 1e3,
           "lone": {"launches_per_window": k_lone, "ms": ms_lone, "outputs": streams * ((n - 1) * L + T)},
           "cat": {"launches_per_window": k_cat, "ms": ms_cat, "outputs": streams * ((n + H - 1) * L + T)},
           "feed_over_lone": ms["median"] / ms_lone["median"], "feed_over_cat": ms["median"] / ms_cat["median"],
           "seen": int(ms_obj.seen()[0])}
    ms_obj.close()
    plan.close()
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-16s feed %8.4f ms  lone %8.4f ms (x %.3f)  cat %8.4f ms (x %.3f)  %.2f TFMA/s (%.0f %% of %.2f)  %.0f s of "
          "output per s and stream" % (name, r["ms"]["median"], r["lone"]["ms"]["median"], r["feed_over_lone"],
                                       r["cat"]["ms"]["median"], r["feed_over_cat"], r["fma_per_s"] * 1e-12,
                                       100 * r["share_of_measured_fma64"], peak * 1e-12, r["output_seconds_per_s"]), flush=True)


def batch_against(tree, commit, argv):
    """finish(): tools/bench_mux.py's workload steps from `tree` and from this one, in turn"""
    def run(name, root):
        env = dict(os.environ)
        env.pop("MIFSK_LIBRARY", None)                              # each tree its own library
        cmd = [sys.executable, os.path.join(root, "tools", "bench_mux.py"), "--step", name] + argv
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT, text=True, env=env,
                               cwd=root)
        except subprocess.TimeoutExpired:
            sys.exit("%s: no result within %d s; nothing further is started" % (" ".join(cmd), LIMIT))
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("%s: exit status %d; nothing further is started" % (" ".join(cmd), p.returncode))
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])

    def finish(result, _step):
        batch = {"parent_commit": commit, "workloads": {}}
        for name in BATCH:
            theirs, ours = run(name, os.path.abspath(tree)), run(name, B.ROOT)
            spread = max(r["ms"]["max"] - r["ms"]["min"] for r in (theirs, ours))
            diff = abs(ours["ms"]["median"] - theirs["ms"]["median"])
            batch["workloads"][name] = {"parent": {"ms": theirs["ms"], "launches_per_window": theirs["launches_per_window"]},
                                        "this": {"ms": ours["ms"], "launches_per_window": ours["launches_per_window"]},
                                        "this_over_parent": ours["ms"]["median"] / theirs["ms"]["median"],
                                        "median_difference_ms": diff, "larger_spread_ms": spread,
                                        "within_spread": diff <= spread}
            print("%-16s batch entry: parent %.4f ms (%.4f .. %.4f), this %.4f ms (%.4f .. %.4f): x %.5f, %s the spread" % (
                name, theirs["ms"]["median"], theirs["ms"]["min"], theirs["ms"]["max"], ours["ms"]["median"],
                ours["ms"]["min"], ours["ms"]["max"], ours["ms"]["median"] / theirs["ms"]["median"],
                "within" if diff <= spread else "OUTSIDE"), flush=True)
        result["batch_against_parent"] = batch
    return finish


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-commit", default=None)
    mine, rest = ap.parse_known_args()
    sys.argv[1:] = rest
    fwd = argparse.ArgumentParser(add_help=False)
    fwd.add_argument("--rounds", type=int, default=5)
    fwd.add_argument("--window-ms", type=float, default=600.0)
    fwd.add_argument("--preheat-ms", type=float, default=300.0)
    f, _ = fwd.parse_known_args(rest)
    argv = ["--rounds", str(f.rounds), "--window-ms", str(f.window_ms), "--preheat-ms", str(f.preheat_ms)]
    B.main(__file__, __doc__, "mux_stream.json", 600.0,
           "outputs x channels x (2 ceil(T / L) + 2 (real rows out) or 4 (complex rows out))",
           WORKLOADS, LIMIT, step_workload, show,
           finish=batch_against(mine.parent_tree, mine.parent_commit, argv) if mine.parent_tree else None)
