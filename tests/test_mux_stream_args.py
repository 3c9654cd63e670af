"""The multiplexer stream (include/mifsk/mux_stream.h, minimodem_amd/csrc/mifsk_mux_stream.hip) without a device:
where it is declared and how it is bound, what its entries refuse before they look into an object, H against its
definition, the consistency of the host restatement -- rows fed in pieces through mux_ref_stream[_iq] and the
tails equal mux_ref[_iq] on the whole rows bit for bit, which is the proof of the definition --, the drain, ragged
rows, seeks, and the host logic under the sanitizers (tools/mux_stream_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _abi as A
import _mux_stream as Ms
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
# the header's prototypes, in its order: name -> (return type, arguments)
PROTOTYPES = {
    "mifsk_mux_stream_create": ("int", 4),
    "mifsk_mux_stream_destroy": ("void", 1),
    "mifsk_mux_stream_feed": ("int", 3),
    "mifsk_mux_stream_seek": ("int", 3),
    "mifsk_mux_stream_seen": ("int", 3),
    "mifsk_mux_stream_drain": ("uint32_t", 2),
}


def test_the_header_declares_these_prototypes_and_the_other_tables_do_not():
    """the header's declarations are the opaque type, the flag and the six prototypes, and none of them has moved
    into the five tables that the other ABI tests pin"""
    path = os.path.join(A.ROOT, "include", _lib.MUX_STREAM_HEADER)
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert '#include "../mifsk.h"' in text
    code = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    found = re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", code)
    assert [(name, (" ".join(ret.split()), args.count(",") + 1)) for ret, name, args in found] == list(PROTOTYPES.items())
    assert re.findall(r"\btypedef\s+struct\s+(\w+)\s+(\w+)\s*;", code) == [("mifsk_mux_stream",) * 2]
    assert re.findall(r"^#define[ \t]+(MIFSK_\w+)[ \t]+(\S+)", text, re.M) == [("MIFSK_MUX_STREAM_IQ", "1u")]
    assert not re.search(r"\bstruct\s+\w+\s*\{", code)              # no struct body: the io is mifsk_mux_io
    assert _lib.MUX_STREAM_IQ == 1
    assert list(_lib.MUX_STREAM_SIGNATURES) == list(PROTOTYPES)
    extensions = [n for table in _lib.EXTENSIONS.values() for n in table]
    for name in PROTOTYPES:
        assert name not in _lib.SIGNATURES and name not in _lib.EXPORTS and name not in _lib.EXT_SIGNATURES
        assert name not in extensions and name not in _lib.STREAM_SIGNATURES and name not in A.header_functions()
    assert _lib.MUX_STREAM_HEADER not in _lib.EXTENSIONS and _lib.MUX_STREAM_HEADER != _lib.STREAM_HEADER


def test_the_library_exports_and_binds_them(lib):
    vp, u32, pu64 = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)
    want = {
        "mifsk_mux_stream_create": (C.c_int, [vp, C.c_int, u32, C.POINTER(vp)]),
        "mifsk_mux_stream_destroy": (None, [vp]),
        "mifsk_mux_stream_feed": (C.c_int, [vp, C.POINTER(_lib.MuxIO), vp]),
        "mifsk_mux_stream_seek": (C.c_int, [vp, pu64, vp]),
        "mifsk_mux_stream_seen": (C.c_int, [vp, pu64, vp]),
        "mifsk_mux_stream_drain": (u32, [u32, u32]),
    }
    for name, (restype, argtypes) in want.items():
        assert _lib.MUX_STREAM_SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert len(argtypes) == PROTOTYPES[name][1]
    assert _lib.MUX_STREAM_SIGNATURES["mifsk_mux_stream_feed"][1][1] is C.POINTER(_lib.MuxIO)      # no new struct
    assert callable(M.MuxStream.feed) and callable(M.MuxStream.seek) and callable(M.MuxStream.seen)


def test_the_entries_refuse_before_they_look_into_an_object(lib, fake_ctx):
    """the refusals that need no device: NULL arguments to every entry, a number of streams and a flag that
    create refuses (a block of zeroed host memory stands in for a plan or an object that is then never looked
    into)"""
    fake = fake_ctx[0]
    h = C.c_void_p()
    for flags in (0, 1):
        assert lib.mifsk_mux_stream_create(None, 2, flags, C.byref(h)) == EINVAL
        assert lib.mifsk_mux_stream_create(fake, 2, flags, None) == EINVAL
        assert lib.mifsk_mux_stream_create(None, 2, flags, None) == EINVAL
        for nstreams in (0, -1, -(1 << 31)):
            assert lib.mifsk_mux_stream_create(fake, nstreams, flags, C.byref(h)) == EINVAL, nstreams
    for flags in (2, 3, 4, 1 << 31):
        assert lib.mifsk_mux_stream_create(fake, 2, flags, C.byref(h)) == EINVAL, flags
    assert not h.value
    lib.mifsk_mux_stream_destroy(None)
    io = _lib.MuxIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = A.BASE, 400, 400, 2
    io.d_out, io.out_stride, io.nout_cap, io.d_nout = A.BASE + (1 << 24), 1600, 1600, A.BASE + (1 << 26)
    assert lib.mifsk_mux_stream_feed(None, None, None) == EINVAL
    assert lib.mifsk_mux_stream_feed(None, C.byref(io), None) == EINVAL
    assert lib.mifsk_mux_stream_feed(fake, None, None) == EINVAL
    seen = (C.c_uint64 * 2)(5, 6)
    assert lib.mifsk_mux_stream_seek(None, None, None) == EINVAL
    assert lib.mifsk_mux_stream_seek(None, seen, None) == EINVAL
    assert lib.mifsk_mux_stream_seen(None, seen, None) == EINVAL
    assert lib.mifsk_mux_stream_seen(fake, None, None) == EINVAL
    assert lib.mifsk_mux_stream_seen(None, None, None) == EINVAL
    assert list(seen) == [5, 6]


def test_the_drain_against_its_definition():
    for L in (1, 2, 3, 40, 64, 300):
        for T in (1, L - 1, L, L + 1, 2 * L + 1, 4096):
            if T < 1:
                continue
            assert M.mux_stream_drain(T, L) == -(-T // L) - 1 == Ms.drain_of(T, L), (T, L)
            assert lib_drain(T, L) == M.mux_stream_drain(T, L)
        assert M.mux_stream_drain(L, 0) == 0 and M.mux_stream_drain(4096, 0) == 0
    assert M.mux_stream_drain(1, 1) == 0 and M.mux_stream_drain(39, 40) == 0 and M.mux_stream_drain(4096, 1) == 4095


def lib_drain(T, L):
    return int(_lib.load().mifsk_mux_stream_drain(T, L))


# ---------------------------------------------------------------------------
# the restatement's consistency: pieces through the tails == the whole rows
# ---------------------------------------------------------------------------
# (L, T, K, P): three of _mux.size_cases() with a tail, one T < L (no tail: the phase alone continues, and the
# phases phi >= T are exact zeros), one H >= 20
SHAPES = [(63, 633, 65, 7), (1, 13, 1, 1), (64, 643, 1, 4800), (40, 17, 3, 4800), (4, 100, 3, 4800)]


def _consistency_cases():
    assert all(any(c[1:] == shape for c in Ms.size_cases()) for shape in SHAPES[:3])
    assert Ms.drain_of(17, 40) == 0 and Ms.drain_of(100, 4) >= 20
    return [pytest.param(name, iq, gains, *shape, id="%s-%s-%s-L%d-T%d-K%d-P%d" % ((name, "iq" if iq else "real",
                         "gains" if gains else "plain") + shape))
            for shape in SHAPES for name in Ms.KINDS for iq in (False, True) for gains in (False, True)]


def make_case(rng, L, T, K, P, gains):
    K = min(K, 4)                                           # (the host's loops are slow; K is not the point)
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0 * L) if T > 2 else rng.standard_normal(T).astype(F32)
    centres = rng.integers(-(P - 1), P, K).astype(np.int32)
    r = int(rng.integers(-(P - 1), P))
    g = (rng.uniform(0.25, 1.5, K) * rng.choice([-1.0, 1.0], K)).astype(F32) if gains else None
    return K, taps, centres, r, g


def feed_pieces(hs, x, cuts, lens=None):
    """row k of x cut at `cuts` (cut to lens[k] where the row ends sooner) through the host model -> the
    concatenated outputs"""
    got, at = [], 0
    for k in cuts:
        ends = [x.shape[1]] * x.shape[0] if lens is None else lens
        got.append(hs.feed([x[row, min(at, ends[row]):min(at + k, ends[row])] for row in range(x.shape[0])]))
        at += k
    return np.concatenate(got, axis=0)


@pytest.mark.parametrize("name,iq,gains,L,T,K,P", _consistency_cases())
def test_pieces_through_the_tails_equal_the_whole_rows(name, iq, gains, L, T, K, P):
    kind = Ms.KINDS[name]
    rng = np.random.default_rng(9000 + 10 * T + K + kind + 100 * iq)
    H = Ms.drain_of(T, L)
    K, taps, centres, r, g = make_case(rng, L, T, K, P, gains)
    n = 26 + 5 * H + 75
    x = Ms.random_rows(rng, iq, K, n, 0.3)
    cuts = Ms.cut_points(rng, n, H)
    assert {0, 1, 7, 8, 9, H, H + 1} <= set(cuts) and max(H - 1, 0) in cuts
    whole, count = Ms.ref_whole(x, None, kind, P, taps, L, centres, r, gains=g, iq=iq, out_stride=(n + H) * L + 8)
    assert count == (n - 1) * L + T
    hs = Ms.HostMuxStream(kind, P, taps, L, centres, r, gains=g, iq=iq)
    got = feed_pieces(hs, x, cuts)
    assert hs.seen == n and got.shape[0] == n * L
    assert Ms.same_bits(got, whole[:n * L]), (name, iq)
    if T < L:                                               # the phases phi >= T: exact zeros
        assert not np.any(got.reshape((n, L) + got.shape[1:])[:, T:])
    # the drain: H samples of +0.0 bring the rest of the row, the zero fill behind its count included
    rest = hs.feed([np.zeros((H, 2) if iq else (H,), F32)] * K)
    assert Ms.same_bits(rest, whole[n * L:(n + H) * L])
    assert count <= (n + H) * L and not np.any(whole[count:])


@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_special_values_and_non_finite_taps_with_rows_equally_long(iq):
    """NaN, +-Inf, -0.0 and subnormals in the samples, NaN and Inf among taps and gains: with rows equally long
    no term beyond a row's end is read, and the pieces are the whole bit for bit"""
    L, T, K, P = 4, 100, 3, 4800
    H = Ms.drain_of(T, L)
    for kind in Ms.KINDS.values():
        rng = np.random.default_rng(77 + kind)
        _K, taps, centres, r, g = make_case(rng, L, T, K, P, True)
        n = 26 + 5 * H + 75
        x = Ms.random_rows(rng, iq, K, n, 0.3)
        flat = x.reshape(K, n, -1)
        flat[0, 40], flat[1, 90], flat[1, 131], flat[2, 60] = np.nan, np.inf, -np.inf, -0.0
        flat[2, 100:100 + H] = np.uint32(12345).view(F32)   # subnormals: a whole tail
        for bad_taps in (False, True):
            if bad_taps:
                taps = taps.copy()
                taps[5], taps[50], taps[97] = np.inf, np.nan, -np.inf
                g = g.copy()
                g[1] = np.inf
            whole, _count = Ms.ref_whole(x, None, kind, P, taps, L, centres, r, gains=g, iq=iq, out_stride=n * L)
            hs = Ms.HostMuxStream(kind, P, taps, L, centres, r, gains=g, iq=iq)
            got = feed_pieces(hs, x, Ms.cut_points(rng, n, H))
            assert Ms.same_bits(got, whole[:n * L]), (kind, bad_taps)
            if not kind & Ms.S16:
                assert np.isnan(got).any()


@pytest.mark.parametrize("iq", [False, True], ids=["real", "iq"])
def test_ragged_rows_equal_the_batch_with_finite_taps(iq):
    """rows that end at different lengths: the stream continues them with +0.0 where the batch skips the terms,
    which is the same sum for finite taps and gains, up to the drain's end and the zero fill"""
    L, T, K, P = 4, 100, 3, 4800
    H = Ms.drain_of(T, L)
    for kind in Ms.KINDS.values():
        rng = np.random.default_rng(55 + kind)
        _K, taps, centres, r, g = make_case(rng, L, T, K, P, True)
        n = 26 + 5 * H + 75
        lens = [n, n - 37, 11]
        x = Ms.random_rows(rng, iq, K, n, 0.3)
        whole, count = Ms.ref_whole(x, lens, kind, P, taps, L, centres, r, gains=g, iq=iq, out_stride=(n + H) * L)
        assert count == (n - 1) * L + T
        hs = Ms.HostMuxStream(kind, P, taps, L, centres, r, gains=g, iq=iq)
        got = feed_pieces(hs, x, Ms.cut_points(rng, n, H), lens=lens)
        got = np.concatenate([got, hs.feed([np.zeros((H, 2) if iq else (H,), F32)] * K)], axis=0)        # the drain
        assert hs.seen == n + H and Ms.same_bits(got, whole), kind


def test_a_stream_joined_beyond_two_to_the_32():
    """a seek to n0 = P ceil(2^32 / P), where the phase index is 0 again: the row's outputs from 0; to n0 + 1: the
    outputs from L on of the row with one +0.0 in front"""
    L, T, K, P = 4, 100, 3, 4800
    rng = np.random.default_rng(32)
    _K, taps, centres, r, g = make_case(rng, L, T, K, P, True)
    n = 300
    x = Ms.random_rows(rng, False, K, n, 0.3)
    n0 = P * -(-2 ** 32 // P)
    assert n0 > 2 ** 32 and n0 % P == 0
    whole, _ = Ms.ref_whole(x, None, 0, P, taps, L, centres, r, gains=g)
    hs = Ms.HostMuxStream(0, P, taps, L, centres, r, gains=g)
    first = feed_pieces(hs, x, [77, 0, 223])
    assert Ms.same_bits(first, whole[:n * L])
    hs.seek(n0)                                             # (the tails still hold the first run's samples)
    assert hs.tails.any()
    got = feed_pieces(hs, x, [77, 0, 223])
    assert hs.seen == n0 + n and Ms.same_bits(got, whole[:n * L])
    hs.seek(n0 + 1)
    got = feed_pieces(hs, x, [5, 295])
    shifted, _ = Ms.ref_whole(np.concatenate([np.zeros((K, 1), F32), x], axis=1), None, 0, P, taps, L, centres, r, gains=g)
    assert Ms.same_bits(got, shifted[L:(n + 1) * L])
    assert not Ms.same_bits(got[:40 * L], whole[:40 * L])   # (the phase does matter)
    hs.seek(0)
    assert Ms.same_bits(feed_pieces(hs, x, [300]), first)


# ---------------------------------------------------------------------------
# the host logic under the sanitizers, stand-alone
# ---------------------------------------------------------------------------
def test_the_host_logic_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "mux_stream_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    "-I" + os.path.join(A.ROOT, "include"), "-I" + os.path.join(A.ROOT, "minimodem_amd", "csrc"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan",     # (the runtimes in the program: nothing to load first)
                    "-o", exe, os.path.join(A.ROOT, "tools", "mux_stream_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    m = re.search(r"^mux_stream_check: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 1000, out
