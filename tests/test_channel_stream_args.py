"""The channel stream (include/mifsk/channel_stream.h, minimodem_amd/csrc/mifsk_channel_stream.hip) without a
device: where it is declared and how it is bound, what its entries refuse before they look into an object,
the counting of outputs against a count done one by one, the tail's bound, the consistency of the host
restatement -- a row fed in pieces through channel_ref_stream[_iq] and a tail equals channel_ref[_iq] on the
whole row bit for bit, which is the proof of the definition -- and the host logic under the sanitizers
(tools/channel_stream_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _abi as A
import _channel as Ch
import _channel_iq as Iq
import _channel_stream as Cs
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# the header's prototypes, in its order: name -> (return type, arguments)
PROTOTYPES = {
    "mifsk_channel_stream_create": ("int", 3),
    "mifsk_channel_stream_destroy": ("void", 1),
    "mifsk_channel_stream_feed": ("int", 4),
    "mifsk_channel_stream_seek": ("int", 3),
    "mifsk_channel_stream_seen": ("int", 3),
    "mifsk_channel_stream_outputs": ("uint64_t", 4),
}
TS = (1, 2, 63, 64, 65, 385)


def test_the_header_declares_these_prototypes_and_the_abi_tables_do_not():
    """the header's declarations are the opaque type, the flag and the six prototypes, eight in all, and none
    of them has moved into the tables that tests/test_abi.py and tests/test_mux_iq_args.py pin"""
    path = os.path.join(A.ROOT, "include", _lib.STREAM_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert '#include "../mifsk.h"' in text
    code = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    found = re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", code)
    assert [(name, (" ".join(ret.split()), args.count(",") + 1)) for ret, name, args in found] == list(PROTOTYPES.items())
    assert re.findall(r"\btypedef\s+struct\s+(\w+)\s+(\w+)\s*;", code) == [("mifsk_channel_stream",) * 2]
    assert re.findall(r"^#define[ \t]+(MIFSK_\w+)[ \t]+(\S+)", text, re.M) == [("MIFSK_CHANNEL_STREAM_IQ", "1u")]
    assert not re.search(r"\bstruct\s+\w+\s*\{", code)              # no struct body: the io is mifsk_channel_io
    assert _lib.CHANNEL_STREAM_IQ == 1
    assert list(_lib.STREAM_SIGNATURES) == list(PROTOTYPES)
    extensions = [n for table in _lib.EXTENSIONS.values() for n in table]
    for name in PROTOTYPES:
        assert name not in _lib.SIGNATURES and name not in _lib.EXPORTS and name not in _lib.EXT_SIGNATURES
        assert name not in extensions and name not in A.header_functions()
    assert _lib.STREAM_HEADER not in _lib.EXTENSIONS


def test_the_library_exports_and_binds_them(lib):
    vp, u32, u64, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)
    want = {
        "mifsk_channel_stream_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "mifsk_channel_stream_destroy": (None, [vp]),
        "mifsk_channel_stream_feed": (C.c_int, [vp, C.POINTER(_lib.ChannelIO), u32, vp]),
        "mifsk_channel_stream_seek": (C.c_int, [vp, pu64, vp]),
        "mifsk_channel_stream_seen": (C.c_int, [vp, pu64, vp]),
        "mifsk_channel_stream_outputs": (u64, [u32, u32, u64, u64]),
    }
    for name, (restype, argtypes) in want.items():
        assert _lib.STREAM_SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert len(argtypes) == PROTOTYPES[name][1]
    assert _lib.STREAM_SIGNATURES["mifsk_channel_stream_feed"][1][1] is C.POINTER(_lib.ChannelIO)     # no new struct


def test_the_entries_refuse_before_they_look_into_an_object(lib, fake_ctx):
    """the refusals that need no device: NULL arguments to every entry (a block of zeroed host memory stands in
    for a plan or an object that is then never looked into)"""
    fake = fake_ctx[0]
    h = C.c_void_p()
    assert lib.mifsk_channel_stream_create(None, 2, C.byref(h)) == EINVAL
    assert lib.mifsk_channel_stream_create(fake, 2, None) == EINVAL
    assert lib.mifsk_channel_stream_create(None, 2, None) == EINVAL
    for nstreams in (0, -1, -(1 << 31)):
        assert lib.mifsk_channel_stream_create(fake, nstreams, C.byref(h)) == EINVAL, nstreams
    assert not h.value
    lib.mifsk_channel_stream_destroy(None)
    io = _lib.ChannelIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = A.BASE, 4000, 4000, 2
    io.d_rows, io.out_stride, io.nout_cap, io.d_nout = A.BASE + (1 << 24), 4000, 4000, A.BASE + (1 << 26)
    for flags in (0, 1, 2):
        assert lib.mifsk_channel_stream_feed(None, None, flags, None) == EINVAL
        assert lib.mifsk_channel_stream_feed(None, C.byref(io), flags, None) == EINVAL
        assert lib.mifsk_channel_stream_feed(fake, None, flags, None) == EINVAL
    seen = (C.c_uint64 * 2)(5, 6)
    assert lib.mifsk_channel_stream_seek(None, None, None) == EINVAL
    assert lib.mifsk_channel_stream_seek(None, seen, None) == EINVAL
    assert lib.mifsk_channel_stream_seen(None, seen, None) == EINVAL
    assert lib.mifsk_channel_stream_seen(fake, None, None) == EINVAL
    assert lib.mifsk_channel_stream_seen(None, None, None) == EINVAL
    assert list(seen) == [5, 6]
    assert M.channel_stream_outputs(0, 4, 100, 100) == 0 and M.channel_stream_outputs(4, 0, 100, 100) == 0


def _d_values(T):
    return tuple(dict.fromkeys(Ch.d_rules(T) + (3 * T + 8,)))      # the rules, and one D > 2 T


def _sweep():
    for T in TS:
        for D in _d_values(T):
            for seen in (0, 1, T - 1, T, T + D - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63):
                yield T, D, seen


def test_the_count_of_outputs_against_a_count_one_by_one():
    n = 0
    for T, D, seen in _sweep():
        for k in (0, 1, D - 1, D, T, 1000):
            got = M.channel_stream_outputs(T, D, seen, k)
            assert got == Cs.brute_outputs(T, D, seen, k), (T, D, seen, k)
            assert got == Cs.outputs_upto(T, D, seen + k) - Cs.outputs_upto(T, D, seen)
            assert got <= -(-k // D)                                # what the feed's two capacity rules rest on
            n += 1
    assert n >= 6 * 6 * 8 * 6


def test_the_sum_over_any_cut_is_the_whole():
    rng = np.random.default_rng(20)
    for i in range(200):
        T = int(rng.choice(TS))
        D = int(rng.choice(_d_values(T)))
        total = int(rng.integers(0, 5 * (T + D)))
        cuts = np.sort(rng.integers(0, total + 1, int(rng.integers(0, 12))))
        edges = [0] + [int(c) for c in cuts] + [total]
        got = sum(M.channel_stream_outputs(T, D, a, b - a) for a, b in zip(edges, edges[1:]))
        assert got == Cs.outputs_upto(T, D, total), (T, D, edges)


def test_the_tail_never_holds_more_than_ntaps_less_one():
    """seen - min(seen, M(seen) D) <= T - 1, the bound the tail's room rests on"""
    for T, D, seen in _sweep():
        for more in (0, 1, D - 1, D, T, 1000):
            n = seen + more
            kept = n - min(n, M.channel_stream_outputs(T, D, 0, n) * D)
            assert 0 <= kept <= T - 1, (T, D, n, kept)


# ---------------------------------------------------------------------------
# the restatement's consistency: pieces through the tail loop == the whole row
# ---------------------------------------------------------------------------
def _consistency_cases():
    """three (T, D, K, P) of size_cases() -- a short filter, D = T, a long one with many channels -- and one
    D > T, each with all four kinds"""
    shapes = [(2, 4, 2, 4799), (64, 64, 63, 65536), (385, 1, 65, 4799)]
    assert all(any(c[1:] == shape for c in Ch.size_cases()) for shape in shapes)
    shapes.append((5, 13, 3, 4799))                                 # D > 2 T: gaps that nobody reads
    return [pytest.param(name, *shape, id="%s-T%d-D%d-K%d-P%d" % ((name,) + shape))
            for shape in shapes for name in Ch.KINDS]


@pytest.mark.parametrize("name,T,D,K,P", _consistency_cases())
def test_pieces_through_the_tail_loop_equal_the_whole_row(name, T, D, K, P):
    kind = Ch.KINDS[name]
    rng = np.random.default_rng(7000 + 10 * T + K + kind)
    K = min(K, 5)                                                   # (the host's three loops are slow; K is not the point)
    n = 5 * T + 12 * D + 17                                         # room for every cut of Cs.cut_points
    assert n <= 2000
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
    centres = Iq.centres_of(rng, K, P)
    x = Iq.random_rows(rng, kind, 1, n)[0]
    cuts = Cs.cut_points(rng, n, T, D)
    assert {0, 1, T - 1} <= set(cuts)
    for iq in (False, True):
        whole = (Iq.ref_channelize_iq if iq else Ch.ref_channelize)(x, kind, P, taps, D, centres, int(centres[-1]))
        assert whole.shape[1] >= 12
        hs = Cs.HostStream(kind, P, taps, D, centres, int(centres[-1]), iq=iq)
        got, at = [], 0
        for k in cuts:
            out = hs.feed(x[at:at + k])
            assert out.shape[1] == M.channel_stream_outputs(T, D, at, k)
            assert len(hs.tail) <= T - 1
            got.append(out)
            at += k
        got = np.concatenate(got, axis=1)
        assert got.shape == whole.shape and Ch.same_f32(got, whole), (name, iq)
        assert hs.seen == n and hs.next == whole.shape[1]


def test_the_restatement_joins_a_capture_beyond_two_to_the_32():
    """first_output far beyond 2^32: where the phase index is 0 again (first_output D a multiple of D P) the
    outputs are the row's from 0, and one output later they are that row's from 1 on"""
    T, D, P, K = 9, 4, 4800, 3
    rng = np.random.default_rng(33)
    taps, centres = M.channel_taps(T, 400.0, 48000.0, 2.0), Iq.centres_of(rng, K, P)
    x = Iq.random_rows(rng, 0, 1, 200)[0]
    n0 = D * P * -(-2 ** 32 // (D * P))
    assert n0 > 2 ** 32 and n0 % (D * P) == 0
    whole = Ch.ref_channelize(x, 0, P, taps, D, centres, 117)
    hs = Cs.HostStream(0, P, taps, D, centres, 117, seen=n0)
    assert hs.next == n0 // D
    got = np.concatenate([hs.feed(x[:77]), hs.feed(x[77:])], axis=1)
    assert Ch.same_f32(got, whole)
    hs.seek(n0 + 3)                                                 # 3 elements are read by nobody
    assert hs.next == n0 // D + 1
    got = np.concatenate([hs.feed(x[:77]), hs.feed(x[77:])], axis=1)
    shifted = Ch.ref_channelize(np.concatenate([np.zeros(3, F32), x]), 0, P, taps, D, centres, 117)
    assert got.shape[1] == shifted.shape[1] - 1 and Ch.same_f32(got, shifted[:, 1:])
    assert not Ch.same_f32(got[:, :40], whole[:, :40])              # (the phase does matter)


# ---------------------------------------------------------------------------
# the host logic under the sanitizers, stand-alone
# ---------------------------------------------------------------------------
def test_the_host_logic_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "channel_stream_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(A.ROOT, "include"), "-I" + os.path.join(A.ROOT, "minimodem_amd", "csrc"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",     # (the runtimes in the program: nothing to load first)
                    "-o", exe, os.path.join(A.ROOT, "tools", "channel_stream_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    m = re.search(r"^channel_stream_check: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 1000, out
