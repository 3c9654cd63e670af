"""The host logic of the time split, without a device.  Which rows are settled, dropped or run again
(settle_round), the row table of a planned call (RowLayout), where the tails go (place_tails) and
the planner are plain C++ in minimodem_amd/csrc/mifsk_timesplit_plan.cpp, so tools/timesplit_rounds.cpp
runs them alone -- that file and mifsk_config.cpp, nothing else linked or loaded -- under the address
and undefined-behaviour sanitizers:

  rounds      25 000 tables of 1 .. 5 streams of 1 .. 12 chunks over a model of the device half (pass A
              guesses right with probability q; a row run from a wrong state pauses in the right one
              with probability p; one row a table may finish its stream), q and p from 0 to 1, both
              ends included: the loop ends, the marks lie in [lo, hi], every row is settled, a row is
              dropped exactly behind a finished row of its own stream, every kept row started from
              the right state, and the accepted / rerun / rounds / samples_rerun figures add up
  row table   plans of the eight modes of test_time_split_plan.py for batches of 1 .. 4 streams of 0 to
              2 h, by the library's choice and with the least chunk and warmup, and their tails
  planner     lengths around W, 4 W, 2^31, 2^32, 2^62 and 2^64, chunks 1 and 2^32 - 1, warmups at the
              limits: 0, -EINVAL or -ENOTSUP, no overflow, and a cut that covers its stream"""
import os
import re
import subprocess

from test_launch_plans import ROCM_INCLUDE, ROOT, SANITIZE


def test_rounds_row_table_tails_and_planner_edges_under_sanitizers(tmp_path):
    exe = str(tmp_path / "timesplit_rounds")
    csrc = os.path.join(ROOT, "minimodem_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + SANITIZE +
                   ["-o", exe, os.path.join(ROOT, "tools", "timesplit_rounds.cpp"),
                    os.path.join(csrc, "mifsk_timesplit_plan.cpp"), os.path.join(csrc, "mifsk_config.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    m = re.search(r"^timesplit_rounds: (\d+) cases, 0 failed$", out, re.M)
    assert m and int(m.group(1)) >= 25000 + 8 * (80 + 6 * 3 * 6 * 3 * 3), out[-2000:]
