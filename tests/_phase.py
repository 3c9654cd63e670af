"""What tests/_channel.py and tests/_mux.py share: how a host restatement from tools/ becomes a shared
object, the restatements' kind bits, and the comparison of bit patterns."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
COMPLEX, S16 = 1, 2                 # channel_ref.c's and mux_ref.c's kind bits
KINDS = {"real-f32": 0, "real-s16": S16, "complex-f32": COMPLEX, "complex-s16": COMPLEX | S16}


@functools.lru_cache(maxsize=None)
def ref_lib(name, prototypes):
    """tools/<name>.c as a shared object in a temporary directory: the machine's C compiler, ROCm's
    clang where there is none; -O2 -ffp-contract=off.  prototypes: ((function, restype, argtypes), ...)"""
    cc = shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/lib/llvm/bin/clang"
    so = os.path.join(tempfile.mkdtemp(prefix=name), name + ".so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tools", name + ".c"), "-lm"], check=True)
    lib = C.CDLL(so)
    for function, restype, argtypes in prototypes:
        getattr(lib, function).restype = restype
        getattr(lib, function).argtypes = list(argtypes)
    return lib


def vec_of(kind):
    """elements in 16 bytes"""
    return 16 // ((2 if kind & S16 else 4) * (2 if kind & COMPLEX else 1))


def same_bits(a, b):
    """equal bit patterns of two arrays of one type (float32, float64, int16), any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    bits = np.dtype("u%d" % a.itemsize)
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))
