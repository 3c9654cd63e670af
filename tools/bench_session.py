#!/usr/bin/env python3
"""Wall time of a batch of streams fed in pieces, by way of feeding.

Workload: 1024 Bell-202 streams of 2 s at 20 dB, fed in 100 ms pieces (20 feeds of 4800 samples).
Paths: the host-tail session (mifsk_session_feed), then the resident session
(MIFSK_SESSION_RESIDENT) from host float32, host PCM16, a device float32 tensor and a device PCM16
tensor.  Every path is run once untimed (code objects, pinned and device buffers), then three
times; the figures are those of the fastest run: wall ms per feed -- Session.feed() blocks until
the feed's results are on the host -- and samples per second, with the session's
h2d_bytes_total beside them.  All paths must decode the same bytes.

    python tools/bench_session.py [--streams 1024] [--feeds 20] [--piece 4800] [--out profiles/session_resident.json]

Needs the GPU: there is no other path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_streams(M, cfg, n, total, seed=2024):
    """n streams of `total` samples as PCM16 and as the floats the device makes of that PCM16"""
    rng = np.random.default_rng(seed)
    nwords = max(1, (total - 4000) // (10 * (cfg.sample_rate // 1200)))
    base = []
    for _ in range(8):                                          # eight payloads, noisy copies of each
        y = M.synthesize(cfg, rng.integers(32, 127, size=nwords, dtype=np.uint8), amplitude=0.5,
                         leading_silence=int(rng.integers(0, 2000)))
        base.append(np.concatenate([y, np.zeros(total, np.float32)])[:total])
    sigma = np.float32(0.5 / np.sqrt(2.0) / 10.0)               # 20 dB below the tone's power
    pcm = np.empty((n, total), np.int16)
    for i in range(n):
        noise = rng.standard_normal(total, dtype=np.float32) * sigma
        pcm[i] = np.rint((base[i % 8] + noise) * 32768.0).astype(np.int16)
    return pcm, pcm.astype(np.float32) / np.float32(32768)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--feeds", type=int, default=20)
    ap.add_argument("--piece", type=int, default=4800)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "session_resident.json"))
    a = ap.parse_args()
    import torch
    import minimodem_amd as M
    if not torch.cuda.is_available():
        sys.exit("bench_session.py measures on the GPU; none is visible")
    ctx = M.Context()
    cfg = M.rx_config("1200")
    n, total = a.streams, a.feeds * a.piece
    pcm, f32 = make_streams(M, cfg, n, total)
    d_pcm, d_f32 = torch.from_numpy(pcm).cuda(), torch.from_numpy(f32).cuda()
    torch.cuda.synchronize()

    def run(resident, data):
        sess = M.Session(ctx, cfg, n, want_frames=False, resident=resident)
        out, dt = [b""] * n, 0.0
        for k in range(a.feeds):
            lo, hi = k * a.piece, (k + 1) * a.piece
            new = data[:, lo:hi] if hasattr(data, "is_cuda") else [data[i, lo:hi] for i in range(n)]
            t0 = time.perf_counter()
            res = sess.feed(new, final=(k == a.feeds - 1))
            dt += time.perf_counter() - t0
            for i, r in enumerate(res):
                out[i] += r["bytes"]
        info = sess.info()
        sess.close()
        return dt, out, info

    paths = [("host_tail", False, f32), ("resident_host_f32", True, f32), ("resident_host_s16", True, pcm),
             ("resident_device_f32", True, d_f32), ("resident_device_s16", True, d_pcm)]
    outs, infos = {}, {}
    for name, resident, data in paths:
        _, outs[name], infos[name] = run(resident, data)
    for name in outs:
        assert outs[name] == outs["host_tail"], "%s decodes differently" % name
    result = {"workload": {"mode": "1200", "streams": n, "feeds": a.feeds, "piece": a.piece,
                           "seconds_per_stream": total / cfg.sample_rate, "snr_db": 20,
                           "bytes_decoded": sum(len(o) for o in outs["host_tail"])},
              "device": ctx.device_name, "repeats": a.repeats, "paths": {}}
    for name, resident, data in paths:
        best = min(run(resident, data)[0] for _ in range(a.repeats))
        result["paths"][name] = {"ms_per_feed": best * 1e3 / a.feeds, "samples_per_s": n * total / best,
                                 "h2d_bytes_total": infos[name]["h2d_bytes_total"],
                                 "row_capacity": infos[name]["row_capacity"],
                                 "x_host_tail": None}
    t0 = result["paths"]["host_tail"]["ms_per_feed"]
    for p in result["paths"].values():
        p["x_host_tail"] = p["ms_per_feed"] / t0
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
