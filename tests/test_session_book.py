"""The per-stream book of a session, without a device.  What a session holds of every stream, where
that starts, what a feed adds, how wide the rows get, what the loop passed and who is done is plain
C++ in minimodem_amd/csrc/mifsk_session_book.cpp, for both kinds of session (the differences are the
members of one policy value), so tools/session_book.cpp runs it alone -- that file, nothing else
linked or loaded -- under the address and undefined-behaviour sanitizers:

  sessions   20 000 per policy, of 1 .. 5 streams and 1 .. 10 feeds of pieces of 0, 1, 3, 4, 5 and
             thousands of samples, from host pointers or (resident) a device array, float32 or PCM16,
             over a model of the loop (the cursor moves to any point of [origin, origin + held], both
             ends included; any stream may finish at any feed): origin + held is everything fed, the
             origin is the cursor and never goes back, the width is the least multiple of 4 (4 at
             least) that holds every row, the pieces lie at ascending, disjoint, 16-byte aligned
             offsets, a resident stream that is done holds 0 and ignores what comes, a host-tail
             stream that is done keeps growing, a plan cannot be committed twice; and at one feed of
             each the refusals -- a pointer missing at every position, no pointers, no device array,
             k > stride, an unknown kind, a piece beyond the limit, a feed after the final one --
             leave every field of the book as it was
  limits     rows of limit - 1, limit and limit + 1 samples, of one piece or on top of 7, limit / 2,
             limit - 1 or limit held ones, from both sources, and two sums that wrap in 32 bits"""
import os
import re
import subprocess

from test_launch_plans import ROOT, SANITIZE


def test_plans_commits_and_refusals_under_sanitizers(tmp_path):
    exe = str(tmp_path / "session_book")
    csrc = os.path.join(ROOT, "minimodem_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + SANITIZE +
                   ["-o", exe, os.path.join(ROOT, "tools", "session_book.cpp"),
                    os.path.join(csrc, "mifsk_session_book.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    m = re.search(r"^session_book: (\d+) cases, 0 failed$", out, re.M)
    # per policy: the sessions; limit - 1 on top of 0, 7, limit / 2 and limit - 1 held samples, limit and
    # limit + 1 on top of those and of limit, each from two sources; the two sums
    assert m and int(m.group(1)) >= 2 * (20000 + 2 * (4 + 5 + 5) + 2), out[-2000:]
