"""Every launch plan, without a device.  A plan (mifsk::LaunchPlan: engine, kernel instantiation,
LDS geometry, chain cut) is a pure function of the configuration, the batch shape, the call's flags
and the CU count (plan_launch in minimodem_amd/csrc/mifsk_plan.cpp), so tools/launch_plans.cpp runs
the planner alone -- mifsk_plan.cpp and mifsk_config.cpp, nothing else linked or loaded -- under
the address and undefined-behaviour sanitizers over

  the 953 configurations of test_gpu_bitlengths.py, twelve named modes and the 6 x 187 frame shapes
  of test_gpu_frameshapes.py (1 .. 64 bit windows a frame; labels like 240/raw43, 1200/7-13-1.5)
  x nstreams 1, 5, 256, 1024, 3000, 4096, 8192, 65536  x nsamples 0, 96000, 1440000  at 256 CUs
  x {plain, RING, --auto-carrier, with loop state, with counters}
  x {library's choice, forced wavefront engine, forced workgroup engine where it is accepted}
  + the named modes once more under MIFSK_EXPERIMENT=1 MIFSK_CHAIN=2,3,

checks the invariants of a plan on each (LDS within a CU's, the chain's bounds, a resumable kernel
wherever there is state or a chain, no chain with state / RING / counters, the geometry's own
bounds) and prints a line per case.  tests/golden/launch_plans.txt holds one digest per configuration
over its cases' lines and, for the named modes of both legs, each distinct plan in full: a plan
that changes shows here, with its configuration's lines.  (The named modes' 3 744 case lines in full
are 0.7 MB per leg, too large a file to commit and to read in a diff: the digest pins every one of
them, and which case gets which plan is read with `launch_plans --named` or `--only LABEL`.)"""
import os
import re
import subprocess

import pytest

import _shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")
SHAPED = len(S.RATES) * len(S.SHAPES)   # the frame-shape leg: 6 x 187
CASES = (953 + 2 * 12 + SHAPED) * 8 * 3 * 13     # 13: the variants x engines that are accepted


# (the sanitizers' runtimes in the program: nothing to load first)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def build_tool(directory, sanitize=True):
    """sanitize=False: the plain program, for the GPU test that only needs the tool's plans (sanitizers
    are for the CPU runs)"""
    exe = os.path.join(str(directory), "launch_plans")
    csrc = os.path.join(ROOT, "minimodem_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + (SANITIZE if sanitize else []) +
                   ["-o", exe, os.path.join(ROOT, "tools", "launch_plans.cpp"),
                    os.path.join(csrc, "mifsk_plan.cpp"), os.path.join(csrc, "mifsk_config.cpp")], check=True)
    return exe


def run_tool(exe, *args, sanitize=True):
    """-> (stdout lines, the summary on stderr); the tool must exit 0: no violation"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIFSK_")}
    if sanitize:
        env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-4000:]
    return r.stdout.decode().splitlines(), err


def parse(line):
    """'rtty n=4096 ns=96000 plain/lib : rc=0 engine=wave ... kernel=NAME' -> (case key, {field: value})"""
    key, rest = line.split(" : ", 1)
    rest, kernel = rest.split(" kernel=", 1)
    d = dict(kv.split("=", 1) for kv in rest.split())
    d["kernel"] = kernel
    return key, d


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build_tool(tmp_path_factory.mktemp("launch_plans"))


def test_every_plan_is_the_recorded_one_and_keeps_the_invariants(tool):
    lines, err = run_tool(tool)
    m = re.search(r"^launch_plans: (\d+) cases, (\d+) distinct plans, (\d+) chained, 0 violations$", err, re.M)
    assert m and int(m.group(1)) == CASES and int(m.group(3)) > 0, err[-2000:]
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    assert sum(" digest=" in w for w in want) == 2 * 12 + 953 + SHAPED and all(w.endswith(" lines=312") for w in want if " digest=" in w)
    # no frame shape is refused: every configuration of the shape sweep has its digest line
    shaped = [label for rate in S.RATE_IDS for label, _mode, _kw, _seed in S.configs(rate)]
    assert [g.split(" digest=")[0] for g in lines if " digest=" in g][-SHAPED:] == shaped
    if lines == want:
        return
    recorded = dict(w.split(" digest=") for w in want if " digest=" in w)
    bad = [g for g in lines if " digest=" in g and recorded.get(g.split(" digest=")[0]) != g.split(" digest=")[1]]
    report = ["- " + w for w in want if w not in lines] + ["+ " + g for g in lines if g not in want]
    for got in bad[:4]:             # the configurations whose cases changed: their lines in full
        report += run_tool(tool, "--only", got.split()[0])[0]
    pytest.fail("%d configurations differ from tests/golden/launch_plans.txt:\n%s" % (len(bad), "\n".join(report[:2000])))


def test_which_batches_are_cut(tool):
    """The library's own rule (tests/test_gpu_chain.py asks the same of a device's context): flat
    wavefront-engine batches of more streams than the chip holds at once, streams long enough to
    cut, an instantiation with a resumable twin."""
    import minimodem_amd as M
    rtty = M.rx_config("rtty")
    n = int(30 * rtty.sample_rate)
    named = dict(parse(line) for line in run_tool(tool, "--named")[0])
    p = named["rtty n=4096 ns=%d plain/lib" % n]
    assert p["chain"] == "2x8" and p["kernel"].endswith("<10, -1, true>")
    assert named["rtty n=1024 ns=%d plain/lib" % n]["chain"] == "0x0"               # one round: nothing to fill
    assert named["rtty n=4096 ns=%d ring/lib" % n]["chain"] == "0x0"
    # (12000 baud runs demod_wave_kernel<4, 1>: the resumable instantiations are the generic ones)
    p = named["12000 n=8192 ns=96000 plain/lib"]
    assert p["chain"] == "0x0" and p["kernel"].endswith("<4, 1>")
    # rows too short to cut: a chunk holds at least 8 of the reference's buffers
    one = lambda ns: parse(run_tool(tool, "--one", "rtty", 4096, ns, "plain", "lib")[0][0])[1]
    assert one(8 * rtty.samplebuf_size)["chain"] == "0x0" and one(16 * rtty.samplebuf_size)["chain"] == "2x2"
