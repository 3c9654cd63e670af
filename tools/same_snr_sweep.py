#!/usr/bin/env python3
"""BASELINE configs[4]: NOAA SAME with an additive-noise SNR sweep and the reference's
DC-offset sweep (tests/40-noise.test), on one GPU.  Reports, per condition, the share
of streams whose whole payload is decoded without a single byte error, and checks
a sample of streams against the oracle (identical buffers -> identical bytes).
    python tools/same_snr_sweep.py [--streams N] [--noise torch|library]
--noise torch (the default): torch.randn per condition, and the noisy batch is copied back for the
oracle.  --noise library: the library's channel model (mifsk_impair_batch) -- every condition's noise
is a per-row sigma of one impair call over the conditions' rows side by side, and the oracle's
sample is made on the CPU from the clean row by the restatement tools/impair_ref.c: no noisy sample
crosses PCIe."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import _oracle as O          # the checker
import minimodem_amd as M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512)
    ap.add_argument("--noise", choices=("torch", "library"), default="torch")
    args = ap.parse_args()
    ctx = M.Context(0)
    cfg = M.rx_config("same")
    ocfg = O.oracle_config("same")
    rng = np.random.default_rng(40)
    n, nwords = args.streams, 120
    words = rng.integers(32, 127, size=(n, nwords), dtype=np.uint8)
    clean, lens = M.synthesize_batch(ctx, cfg, torch.from_numpy(words).cuda(), amplitude=0.5)
    nsamp = int(lens[0])
    p_sig = 0.5 ** 2 / 2
    conds = [("clean", None, 0.0)] + [("SNR %2d dB" % s, s, 0.0) for s in (20, 12, 9, 6, 3)] \
        + [("DC offset %.2f" % d, None, d) for d in (0.05, 0.10, 0.50)]
    print("%-16s %12s %14s" % ("condition", "error-free", "== oracle"))
    if args.noise == "library":
        return library_sweep(ctx, cfg, ocfg, words, clean, lens, conds)
    for name, snr, dc in conds:
        x = clean.clone()
        if snr is not None:
            sigma = float(np.sqrt(p_sig / 10 ** (snr / 10)))
            g = torch.Generator(device="cuda"); g.manual_seed(1000 + snr)
            x[:, :nsamp] += sigma * torch.randn((n, nsamp), generator=g, device="cuda")
        if dc:
            M.ingest_rxnoise(ctx, x, dc, nsamples=lens)     # the reference's --Xrxnoise term
        res = M.results_to_host(M.demod_batch(ctx, cfg, x, nsamples=lens, want=("bytes",)))
        ok = 0
        for i in range(n):
            got = res["bytes"][i, :int(res["nbytes"][i])].tobytes()
            ok += words[i].tobytes() in got                 # the whole 120-byte payload, no error
        same = 0
        host = x.cpu().numpy()
        sample = range(0, n, max(1, n // 16))
        for i in sample:
            ref = O.oracle_rx_stream(ocfg, host[i, :nsamp])
            same += ref["bytes"] == res["bytes"][i, :int(res["nbytes"][i])].tobytes()
        print("%-16s %7d/%-4d %9d/%d" % (name, ok, n, same, len(sample)))


def library_sweep(ctx, cfg, ocfg, words, clean, lens, conds):
    """The conditions as blocks of rows of ONE batch: block c is the clean batch again, its rows' sigma
    condition c's, its field rows first_stream = c * n onwards; then the DC conditions' --Xrxnoise term
    and one demod_batch per block."""
    import _impair as Im        # the restatement, for the oracle's samples
    n, nsamp = clean.shape[0], int(lens[0])
    seed = 40
    sig = np.array([M.snr_sigma(0.5, float("inf") if snr is None else snr) for _name, snr, _dc in conds], np.float32)
    batch = clean.repeat(len(conds), 1)
    M.impair(ctx, batch, nsamples=lens.repeat(len(conds)), seed=seed, out=batch,
             sigma=torch.from_numpy(np.repeat(sig, n)).cuda())
    host_clean = clean.cpu().numpy()
    for c, (name, snr, dc) in enumerate(conds):
        x = batch[c * n:(c + 1) * n]
        if dc:
            M.ingest_rxnoise(ctx, x, dc, nsamples=lens)
        res = M.results_to_host(M.demod_batch(ctx, cfg, x, nsamples=lens, want=("bytes",)))
        ok = sum(words[i].tobytes() in res["bytes"][i, :int(res["nbytes"][i])].tobytes() for i in range(n))
        same = 0
        sample = range(0, n, max(1, n // 16))
        for i in sample:
            row = Im.ref_impair(host_clean[i:i + 1], None, False, host_clean.shape[1], seed=seed,
                                first_stream=c * n + i, sigma=float(sig[c]), nsamples=nsamp)[0, :nsamp]
            if dc:
                row = row - np.float32(dc)                  # the --Xrxnoise term: the constant -factor
            ref = O.oracle_rx_stream(ocfg, row)
            same += ref["bytes"] == res["bytes"][i, :int(res["nbytes"][i])].tobytes()
        print("%-16s %7d/%-4d %9d/%d" % (name, ok, n, same, len(sample)))


if __name__ == "__main__":
    main()
