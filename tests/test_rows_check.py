"""What the batch entries refuse of a batch of rows (minimodem_amd/csrc/mifsk_batch.h: kind_check,
out_rows_check, feed_rows_check, rows_in), without a device: tools/rows_check.cpp calls them with the
argument ladders of the channel model and the FM stage -- aligned and unaligned bases, strides 0, 4, 6,
8, 0xFFFFFFF8 and 0xFFFFFFFC, both kinds and unknown ones -- under the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows") / "rows_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "minimodem_amd", "csrc"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",     # (the runtimes in the program: nothing to load first)
                    "-o", exe, os.path.join(ROOT, "tools", "rows_check.cpp")], check=True)
    return exe


def test_the_checks_of_a_batch_of_rows(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    m = re.search(r"^rows_check: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 100, out
