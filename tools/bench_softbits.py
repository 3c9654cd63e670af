#!/usr/bin/env python3
"""Time of the soft-bits pass (mifsk_frame_softbits) beside the decode it annotates.

Workload: BASELINE.json configs[1], bench.py's own batch -- 1024 Bell-202 streams of 480 000
samples, float32, resident in HBM -- decoded once with "frames", then

    soft    mifsk_frame_softbits over all its frames into arrays made beforehand (the C entry)
    soft_py minimodem_amd.frame_softbits, which also allocates and zero-fills its outputs
    demod   mifsk_demod_batch on the same batch, bench.py's outputs ("bytes", "episodes")

After 0.3 s of untimed launches and a warm-up of every call, the three are timed in turn, `rounds`
times over, each as K launches on one stream between two device events, K sized so that a window
lasts `window_ms`; the figure of a call is the median of its rounds, the spread their range.

The bytes model: every sample is read once, 8 bytes are written per bit (and 8 per frame for the raw
bits), 32 bytes are read per frame record; the floor is those bytes at 8 TB/s.  `share_of_hbm_peak`
is that floor over the measured time of `soft`.

    python tools/bench_softbits.py [--streams 1024] [--mode 1200] [--out profiles/softbits.json]

Needs the GPU: there is no other path.  `--resources FILE`: the text tools/kernel_resources.sh
prints (registers, LDS, scratch of the instantiations), copied into the result.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def resources(path):
    import re
    rows = []
    pat = re.compile(r"^\S+\s+(\S*softbits\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) vgpr_spill\s+(\d+) sgpr\s+(\d+) "
                     r"sgpr_spill\s+(\d+) scratch\s+(\d+) B static_lds\s+(\d+)")
    if path and os.path.exists(path):
        for line in open(path):
            m = pat.match(line)
            if m:
                rows.append(dict(zip(("kernel", "vgpr", "agpr", "vgpr_spill", "sgpr", "sgpr_spill", "scratch_bytes",
                                      "static_lds_bytes"), [m.group(1)] + [int(v) for v in m.groups()[1:]])))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--mode", default="1200")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--preheat-ms", type=float, default=300.0)
    ap.add_argument("--resources", default=os.path.join(ROOT, "profiles", "softbits_kernel_resources.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softbits.json"))
    a = ap.parse_args()
    import bench                                                # (the batch is bench.py's own)
    import torch
    import minimodem_amd as M
    from minimodem_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("bench_softbits.py measures on the GPU; none is visible")
    ctx = M.Context()
    cfg = M.rx_config(a.mode)
    n, S = bench.NSAMPLES, a.streams
    host = np.zeros((S, n), np.float32)

    def gen(i):
        if a.mode == "1200":
            x = bench.make_stream(M, cfg, i)[0]
        else:
            words, lead = bench.stream_words(a.mode, cfg, i, n)
            x = M.synthesize(cfg, words, leading_silence=lead)[:n]
        host[i, :len(x)] = x

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(gen, range(S)))
    d = torch.from_numpy(host).cuda()
    del host
    cap = M.max_frames(cfg, n)
    nb = int(cfg.expect_n_bits)
    frames = M.demod_batch(ctx, cfg, d, want=("frames",), frames_cap=cap)
    torch.cuda.synchronize()
    nframes = int(frames["nframes"].clamp(max=cap).sum())
    out_demod = M.demod_batch(ctx, cfg, d, want=("bytes", "episodes"), frames_cap=cap)
    mag = torch.zeros((S, cap, nb, 2), dtype=torch.float32, device="cuda")
    raw = torch.zeros((S, cap), dtype=torch.int64, device="cuda")
    io = _lib.SoftbitsIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = d.data_ptr(), d.stride(0), n, S
    io.kind = _lib.FEED_F32
    io.d_frames, io.d_nframes, io.frames_cap = frames["frames"].data_ptr(), frames["nframes"].data_ptr(), cap
    io.d_mag, io.d_rawbits = mag.data_ptr(), raw.data_ptr()
    lib = _lib.load()
    sp = M._stream_ptr(torch, None)

    def soft():
        rc = lib.mifsk_frame_softbits(ctx.handle, C.byref(cfg), C.byref(io), sp)
        assert rc == 0, rc

    calls = {"soft": soft,
             "soft_py": lambda: M.frame_softbits(ctx, cfg, d, frames),
             "demod": lambda: M.demod_batch(ctx, cfg, d, want=("bytes", "episodes"), frames_cap=cap, out=out_demod)}

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.preheat_ms:
        calls["demod"]()
        soft()
        torch.cuda.synchronize()
    reps = {}
    for name, fn in calls.items():                              # warm-up, and K for the window
        ms = timed(fn, 5)
        reps[name] = max(5, int(a.window_ms / max(ms, 1e-3)))
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):                                   # alternating, in one process
        for name, fn in calls.items():
            ms[name].append(timed(fn, reps[name]))
    # the answer is the binding's, and sane
    chk = M.frame_softbits(ctx, cfg, d, frames)
    torch.cuda.synchronize()
    assert torch.equal(chk["mag"].view(torch.int32), mag.view(torch.int32)) and torch.equal(chk["rawbits"], raw)
    assert bool(torch.isfinite(mag).all()) and float(mag.max()) > 0.1

    bytes_read = S * n * 4 + nframes * 32
    bytes_written = nframes * nb * 8 + nframes * 8
    floor_ms = (bytes_read + bytes_written) / HBM_PEAK * 1e3
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {
        "workload": {"mode": a.mode, "streams": S, "samples_per_stream": n, "frames": nframes,
                     "expect_n_bits": nb, "bit_nsamples": int(cfg.bit_nsamples), "frames_cap": cap},
        "device": ctx.device_name,
        "method": {"events": "one pair around K launches on one stream", "rounds": a.rounds,
                   "launches_per_window": reps, "preheat_ms": a.preheat_ms, "order": "soft, soft_py, demod alternating"},
        "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in ms.items()},
        "soft_over_demod": med["soft"] / med["demod"],
        "bytes_model": {"read": bytes_read, "written": bytes_written, "f64_fma": nframes * nb * int(cfg.bit_nsamples) * 4,
                        "floor_ms_at_8TBps": floor_ms},
        "share_of_hbm_peak": floor_ms / med["soft"],
        "achieved_GBps": (bytes_read + bytes_written) / med["soft"] / 1e6,
        "kernel_resources": resources(a.resources),
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
