#!/usr/bin/env python3
"""Time of the power squelch (mifsk_fm_squelch_batch) on 1024 rows of 480 000 complex samples
(10 s at 48 kHz), against the HBM rate of the device, beside what a user writes in torch without the entry, and
beside the discriminator on the same rows, all in one run.

    f32-B96, f32-B4800, s16-B96, s16-B4800      energies, gates, spans and state of float32 / PCM16 I/Q rows
    ...-mute                                    the same with the discriminator's audio muted in place
    torch-B96, torch-B4800                      (z.real**2 + z.imag**2).view(rows, -1, B).sum(-1) >= level
    demod-f32, demod-s16                        mifsk_fm_demod_batch on the same rows

The rows are an FM carrier at full scale that is keyed for the first half of every row, in noise at -40 dBFS:
half of the audio is muted.  Every step is a process of its own under its own time limit; the first one that
fails, is killed by a signal or runs out of time ends the run.  A workload step: a preheat of untimed launches,
then `rounds` windows of K launches on one stream between two device events, K sized so that a window lasts
`window_ms`; the figure is the median of the rounds.  Bytes are what the launches must read and write once
each: 8 or 4 per sample of I/Q, 4 per muted sample of audio (half of them), 12 and 8 for the discriminator; the
windows' outputs and the scratch are below 2 % of that and not counted.  Their share is of 8 TB/s.  f64
operations: 4 per sample (a product, an fma, the scaling and the rounding add).

    python tools/bench_squelch.py [--out profiles/squelch.json]

Needs the GPU: there is no other path.
"""
import json
import sys
import time

import _benchsteps as B

sys.path.insert(0, B.ROOT)

ROWS, SAMPLES = 1024, 480000
KEYED = SAMPLES // 2
OPEN_DB, CLOSE_DB, HANG = -6.0, -10.0, 1
DEV, GAIN = 3000.0 / 48000.0, 48000.0 / 3000.0
HBM_BYTES_PER_S = 8e12
LIMIT = 300                 # seconds a workload step may take
WORKLOADS = {}              # name: (what, PCM16 rows, window, muting, f64 operations per sample, bytes per sample)
for _kind, _s16 in (("f32", False), ("s16", True)):
    for _window in (96, 4800):
        WORKLOADS["%s-B%d" % (_kind, _window)] = ("squelch", _s16, _window, False, 4, 4 if _s16 else 8)
        WORKLOADS["%s-B%d-mute" % (_kind, _window)] = ("squelch", _s16, _window, True, 4, (4 if _s16 else 8) + 2)
for _window in (96, 4800):
    WORKLOADS["torch-B%d" % _window] = ("torch", False, _window, False, 0, 8)
WORKLOADS["demod-f32"] = ("demod", False, 0, False, 26, 12)
WORKLOADS["demod-s16"] = ("demod", True, 0, False, 26, 8)


def step_workload(name, rounds, window_ms, preheat_ms):
    import torch
    import minimodem_amd as M
    what, s16, window, mute, ops, nbytes = WORKLOADS[name]
    ctx = M.Context()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.rand((ROWS, SAMPLES), generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0
    iq = M.fm_modulate(ctx, x, deviation=DEV)
    del x
    iq[:, KEYED:] = 0.0
    iq = M.impair(ctx, iq.view(ROWS, 2 * SAMPLES), seed=7, sigma=M.snr_sigma(1.0, 40.0), s16_out=s16).view(ROWS, SAMPLES, 2)
    audio = torch.empty((ROWS, SAMPLES), dtype=torch.float32, device="cuda")
    check = None
    if what == "demod":
        def call():
            return M.fm_demod(ctx, iq, gain=GAIN, out=audio)
    elif what == "torch":
        z = torch.view_as_complex(iq)
        level = float(M.squelch_level(OPEN_DB, window)) * 2.0 ** -40

        def call():
            return (z.real ** 2 + z.imag ** 2).view(ROWS, -1, window).sum(-1) >= level

        def check():
            gate = call()
            return float(gate[:, :KEYED // window].float().mean()), float(gate[:, KEYED // window + 1:].float().mean())
    else:
        M.fm_demod(ctx, iq, gain=GAIN, out=audio)
        state = torch.zeros((ROWS, 32), dtype=torch.uint8, device="cuda")
        out = M.fm_squelch(ctx, iq, window=window, open_db=OPEN_DB, close_db=CLOSE_DB, hang=HANG, state=state,
                           audio=audio if mute else None)

        def call():
            return M.fm_squelch(ctx, iq, window=window, open_db=OPEN_DB, close_db=CLOSE_DB, hang=HANG, state=state,
                                audio=audio if mute else None, out=out)

        def check():
            gate = call()["gate"][:, :SAMPLES // window]
            return float(gate[:, :KEYED // window].float().mean()), float(gate[:, KEYED // window + HANG + 1:].float().mean())
    torch.cuda.synchronize()

    k, ms = B.timed_windows(call, rounds, window_ms, preheat_ms)
    res = {"workload": {"rows": ROWS, "complex_samples_per_row": SAMPLES, "what": what, "pcm16": s16, "window": window,
                        "mute": mute, "library_entry": what != "torch"},
           "device": ctx.device_name, "launches_per_window": k, "rounds": rounds, "ms": ms}
    if check:
        keyed, idle = check()
        assert keyed > 0.99 and idle < 0.01, (keyed, idle)      # the gate follows the keying
        res["gate_open_keyed_and_idle"] = [keyed, idle]
    if mute:
        muted = float((audio == 0).float().mean())
        assert 0.48 < muted < 0.52, muted                      # half, less hang + 1 windows of tail, plus the first window
        res["muted_share_of_audio"] = muted
    med = ms["median"]
    n = ROWS * SAMPLES
    res.update({"samples_per_s": n / med * 1e3, "fma_per_s": n * ops / med * 1e3, "f64_ops_per_sample": ops,
                "f64_ops_per_s": n * ops / med * 1e3, "bytes_per_sample": nbytes, "bytes_per_s": n * nbytes / med * 1e3,
                "share_of_8TB_per_s": n * nbytes / med * 1e3 / HBM_BYTES_PER_S})
    ctx.close()
    print(json.dumps(res))


def show(name, r, peak):
    print("%-16s %9.3f ms (%.3f - %.3f)  %.3e samples/s  %.2f TB/s (%.0f %% of 8)" % (
        name, r["ms"]["median"], r["ms"]["min"], r["ms"]["max"], r["samples_per_s"], r["bytes_per_s"] * 1e-12,
        100 * r["share_of_8TB_per_s"]), flush=True)


def finish(result, _step):
    """the day of the run; beside every workload of the squelch the torch path at its window and the
    discriminator on its kind of rows"""
    result["date"] = time.strftime("%Y-%m-%d")
    w = result["workloads"]
    for name, r in w.items():
        if r["workload"]["what"] != "squelch":
            continue
        base = w.get("torch-B%d" % r["workload"]["window"])
        if base:
            r["torch_ms"] = base["ms"]["median"]
            r["speedup_over_torch"] = base["ms"]["median"] / r["ms"]["median"]
        demod = w.get("demod-s16" if r["workload"]["pcm16"] else "demod-f32")
        if demod:
            r["demod_ms"] = demod["ms"]["median"]
            r["share_of_demod_bytes_per_s"] = r["bytes_per_s"] / demod["bytes_per_s"]


if __name__ == "__main__":
    B.main(__file__, __doc__, "squelch.json", 600.0,
           "f64 operations as the definition has them: 4 per sample in the squelch, 26 in the discriminator; the torch "
           "path: none counted",
           WORKLOADS, LIMIT, step_workload, show, finish=finish)
