"""What tools/bench_carrier.py, bench_channel.py and bench_mux.py share: a step is a process of its own
under its own time limit, and the first one that fails, is killed by a signal or runs out of time ends
the run; a workload is timed as `rounds` windows of K launches on one stream between two device
events, K sized so that a window lasts `window_ms`; the FP64 FMA rate they compare against is
tools/ubench/fma64_rate.hip, measured first."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMA64_LIMIT = 120           # seconds


def run_step(argv, limit):
    """one step in a process of its own: its last line of output as JSON, or the run ends here"""
    try:
        p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit, text=True)
    except subprocess.TimeoutExpired:
        sys.exit("%s: no result within %d s; nothing further is started" % (" ".join(argv), limit))
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit("%s: exit status %d; nothing further is started" % (" ".join(argv), p.returncode))
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]), p.stdout


def timed_windows(call, rounds, window_ms, preheat_ms):
    """preheat_ms of untimed calls, then `rounds` windows of K calls -> (K, {"median", "min", "max"} of
    the windows' milliseconds per call)"""
    import torch

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < preheat_ms:
        call()
        torch.cuda.synchronize()
    k = max(2, int(window_ms / max(timed(2), 1e-3)))
    ms = [timed(k) for _ in range(rounds)]
    return k, {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def alternating_windows(calls, rounds, window_ms, preheat_ms):
    """timed_windows for several calls at once: each preheated and its K chosen alone, then `rounds`
    rounds of one window of each, in turn -> [(K, {"median", "min", "max"} ms per call)] in calls' order"""
    import torch

    def timed(call, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    ks = []
    for call in calls:
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < preheat_ms:
            call()
            torch.cuda.synchronize()
        ks.append(max(2, int(window_ms / max(timed(call, 2), 1e-3))))
    ms = [[] for _ in calls]
    for _ in range(rounds):
        for i, call in enumerate(calls):
            ms[i].append(timed(call, ks[i]))
    return [(k, {"median": statistics.median(m), "min": min(m), "max": max(m)}) for k, m in zip(ks, ms)]


def step_fma64():
    """the fma64 step (built first where it is missing) -> what goes under "fma64" of the result"""
    ub = os.path.join(ROOT, "tools", "ubench", "fma64_rate")
    if not os.path.exists(ub):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", ub, ub + ".hip"], check=True)
    fma, text = run_step([ub], FMA64_LIMIT)
    return dict(fma, output=text.splitlines()[:-1])


def main(script, doc, out_name, window_ms, fma_count, workloads, limit, step_workload, show, steps=None, finish=None):
    """A tool's command line.  --step NAME runs one step in this process: steps[NAME](), or
    step_workload(NAME, rounds, window_ms, preheat_ms).  Otherwise: the fma64 step, every workload (or
    those of --only) as a step of `limit` seconds with show(name, result, fma64 rate) after each, then
    finish(result, step), where step(name, seconds) runs a further step; the result goes to --out."""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--step", help="(internal) run one step in this process")
    ap.add_argument("--only", nargs="*", help="workloads to run (default: all)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=window_ms)
    ap.add_argument("--preheat-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    a = ap.parse_args()
    if a.step in (steps or {}):
        return steps[a.step]()
    if a.step:
        return step_workload(a.step, a.rounds, a.window_ms, a.preheat_ms)

    result = {"method": {"events": "one pair around K launches on one stream", "rounds": a.rounds,
                         "window_ms": a.window_ms, "preheat_ms": a.preheat_ms, "fma_count": fma_count}}
    result["fma64"] = step_fma64()
    peak = result["fma64"]["fma64_per_s"]
    me = [sys.executable, os.path.abspath(script), "--rounds", str(a.rounds), "--window-ms", str(a.window_ms),
          "--preheat-ms", str(a.preheat_ms)]

    def step(name, seconds):
        return run_step(me + ["--step", name], seconds)[0]

    result["workloads"] = {}
    for name in (a.only or list(workloads)):
        r = step(name, limit)
        r["share_of_measured_fma64"] = r["fma_per_s"] / peak
        result["workloads"][name] = r
        show(name, r, peak)
    if finish:
        finish(result, step)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def add_parents(paths, commit, tail):
    """finish() of an --iq run, whose workloads are named NAME + `tail`: the real entry's time of other
    commits' results (their plain runs: workloads named NAME) beside this one's"""
    def finish(result, _step):
        if commit:
            result["parent_commit"] = commit
        result["parents"] = []
        for path in paths:
            with open(path) as f:
                theirs = json.load(f)["workloads"]
            entry = {"file": os.path.basename(path), "workloads": {}}
            for name, r in result["workloads"].items():
                p = theirs[name[:-len(tail)]]
                assert p["workload"] == r["workload"], name
                entry["workloads"][name] = {"ms": p["ms"], "this_over_parent": r["ms"]["median"] / p["ms"]["median"]}
            result["parents"].append(entry)
    return finish
