"""The host side's owners of device and page-locked memory (minimodem_amd/csrc/mifsk_hostmem.h), the
gather's receive sets over them (mifsk_gather_sets.h) and the table of mifsk_demod_io's result
arrays (mifsk_outputs.h), without a device: tools/hostmem_check.cpp defines the allocation calls
over malloc(), lets each allocation of each scenario fail in turn, and runs under the address and
undefined-behaviour sanitizers with leak detection -- growth and head-room, the state after a
failure, moves and releases, a failed fit of a receive set leaving an empty set, outputs_advance
and outputs_assign field by field."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostmem") / "hostmem_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "minimodem_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "tools"),         # (fake_hip.h: the runtime made of malloc())
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",     # (the runtimes in the program: nothing to load first)
                    "-o", exe,
                    os.path.join(ROOT, "tools", "hostmem_check.cpp")], check=True)
    return exe


def test_owners_free_once_and_the_output_table_moves_every_array(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    m = re.search(r"^hostmem_check: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 100, out
