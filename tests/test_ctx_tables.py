"""The context's device tables, its collector and its streams and events (minimodem_amd/csrc/
mifsk_ctx.cpp, mifsk_tables.cpp, the stream and event owners of mifsk_hostmem.h), without a device:
tools/ctx_tables_check.cpp links them with the planner over a HIP made of malloc() (tools/fake_hip.h)
and runs under the address and undefined-behaviour sanitizers with leak detection --

  every double of the bit tables (Bell-202, B = 3, B = 320, SAME, RTTY), of RTTY's and B = 320's
  rotation tables and of the spectrum tables (N = 240, RTTY's) against the oracle's ofsk_twiddle,
  +0.0 everywhere else, the sizes and strides as the kernels read them;
  the first lookup of Bell-202, of RTTY (several rotation tables in one entry) and of a spectrum
  table with every allocation and every copy failing in turn: -ENOMEM / -EIO, nothing of the
  half-made entry held, the same lookup again succeeds, a third returns the same pointers;
  the collector at 64 configurations, 64 tables and 64 MB: no flush one short of a bound, one
  device synchronisation and nothing held after it, what was used before rebuilt with the same bytes;
  a context with a full cache, a made chain and the host pipeline's work destroyed once, the chain's
  state array after its streams are synchronised; the chain and host_work_init with every stream and
  event creation failing in turn, then again: nothing made twice, nothing leaked.

oracle/fsk_oracle.c is compiled in with the flags of the oracle's own library (no sanitizer: its
cos and -sin are one sincos call, which is what the tables must reproduce)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
CSRC = os.path.join(ROOT, "minimodem_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ctx_tables")
    oracle, exe = str(tmp / "fsk_oracle.o"), str(tmp / "ctx_tables_check")
    subprocess.run(["gcc", "-O2", "-g", "-std=gnu11", "-fPIC", "-mfma", "-ffp-contract=off", "-c",     # (oracle/Makefile's)
                    os.path.join(ROOT, "oracle", "fsk_oracle.c"), "-o", oracle], check=True)
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROOT, "tools"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",     # (the runtimes in the program: nothing to load first)
                    "-o", exe, os.path.join(ROOT, "tools", "ctx_tables_check.cpp")] +
                   [os.path.join(CSRC, s) for s in ("mifsk_ctx.cpp", "mifsk_tables.cpp", "mifsk_plan.cpp", "mifsk_config.cpp")] +
                   [oracle, "-lm"], check=True)
    return exe


def test_tables_equal_the_oracles_and_the_cache_frees_everything_once(checker):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIFSK_")}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    m = re.search(r"^ctx_tables_check: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 2000, out[-4000:]
