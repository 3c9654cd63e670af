"""The power squelch (include/mifsk/squelch.h, minimodem_amd/csrc/mifsk_squelch.hip) without a device: what the
header declares and how it is bound, the structs against their ctypes mirrors, what the entry refuses -- before
any HIP call, so every code below comes back on a machine without a device: the context is a block of zeroed
host memory and the device pointers are numbers -- and the level helper."""
import ctypes as C
import os
import re

import _abi as A
import _squelch as Sq
import minimodem_amd as M
from _abi import BASE, EINVAL, fake_ctx, ladder, lib  # noqa: F401
from minimodem_amd import _lib

PROTOTYPES = {"mifsk_fm_squelch_batch": ("int", 3), "mifsk_fm_squelch_level": ("uint64_t", 2)}
STRUCT_NAMES = ["mifsk_fm_squelch_state", "mifsk_fm_squelch_span", "mifsk_fm_squelch_io"]


def _header():
    path = os.path.join(A.ROOT, "include", _lib.SQUELCH_HEADER)
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _header_structs():
    """{name: [(field, kind, bytes)]} of the header's structs, by _abi's reader of include/*.h"""
    structs = {}
    for name, body in re.findall(r"\bstruct\s+(\w+)\s*\{([^{}]*)\}", _header()):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            ctype, declarator = re.fullmatch(r"(.*?)(\**\s*\w+)", decl).groups()
            stars, field = re.fullmatch(r"(\**)\s*(\w+)", declarator).groups()
            ctype = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
            kind, size = ("pointer", 8) if stars or ctype.endswith("*") else A.SCALARS[ctype]
            fields.append((field, kind, size))
        structs[name] = fields
    return structs


def test_the_header_declares_these_prototypes_and_structs_and_the_other_tables_do_not():
    text = _header()
    assert '#include "../mifsk.h"' in text
    code = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    found = re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", code)
    assert [(name, (" ".join(ret.split()), args.count(",") + 1)) for ret, name, args in found] == list(PROTOTYPES.items())
    assert re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{[^{}]*\}\s*(\w+)\s*;", code) == [(n, n) for n in STRUCT_NAMES]
    assert re.findall(r"^#define[ \t]+(\w+)", text, re.M) == ["MIFSK_SQUELCH_H"]         # the include guard alone
    assert list(_lib.SQUELCH_SIGNATURES) == list(PROTOTYPES) and list(_lib.SQUELCH_STRUCTS) == STRUCT_NAMES
    extensions = [n for table in _lib.EXTENSIONS.values() for n in table]
    for name in PROTOTYPES:
        assert name not in _lib.SIGNATURES and name not in _lib.EXPORTS and name not in _lib.EXT_SIGNATURES
        assert name not in extensions and name not in _lib.STREAM_SIGNATURES and name not in _lib.MUX_STREAM_SIGNATURES
        assert name not in A.header_functions()
    for name in STRUCT_NAMES:
        assert name not in _lib.STRUCTS and name not in A.header_structs()
    assert "squelch" not in A._headers()                    # include/*.h is as it was
    assert _lib.SQUELCH_HEADER not in _lib.EXTENSIONS
    assert _lib.SQUELCH_HEADER not in (_lib.STREAM_HEADER, _lib.MUX_STREAM_HEADER)
    assert A.header_constants()["MIFSK_ABI_VERSION"] == _lib.load().mifsk_abi_version()


def test_the_library_exports_and_binds_them(lib):
    vp = C.c_void_p
    want = {"mifsk_fm_squelch_batch": (C.c_int, [vp, C.POINTER(_lib.FmSquelchIO), vp]),
            "mifsk_fm_squelch_level": (C.c_uint64, [C.c_double, C.c_uint32])}
    for name, (restype, argtypes) in want.items():
        assert _lib.SQUELCH_SIGNATURES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes and len(argtypes) == PROTOTYPES[name][1], name
    for name in ("FmSquelchIO", "fm_squelch", "squelch_level"):
        assert name in M.__all__ and hasattr(M, name), name
    assert M.FmSquelchIO is _lib.FmSquelchIO


def test_the_structs_match_their_mirrors():
    """field for field: name, order, width, offset under natural alignment, pointer or not; the sizes"""
    structs = _header_structs()
    assert list(structs) == STRUCT_NAMES
    for name, fields in structs.items():
        mirror = _lib.SQUELCH_STRUCTS[name]
        assert [f[0] for f in fields] == [f[0] for f in mirror._fields_], name
        end = 0
        for (field, kind, size), (_f, ctype) in zip(fields, mirror._fields_):
            end = -(-end // size) * size
            desc = getattr(mirror, field)
            assert (desc.offset, desc.size) == (end, size), (name, field)
            assert (kind == "pointer") == (ctype is C.c_void_p), (name, field)
            if kind != "pointer":
                assert kind == ("float" if ctype in (C.c_float, C.c_double) else
                                "signed" if ctype in (C.c_int, C.c_int32, C.c_int64) else "unsigned"), (name, field)
            end += size
        assert C.sizeof(mirror) == -(-end // 8) * 8, name
    assert [C.sizeof(_lib.SQUELCH_STRUCTS[n]) for n in STRUCT_NAMES] == [32, 16, 152]
    assert Sq.STATE.itemsize == 32 and [Sq.STATE.fields[f][1] for f in Sq.STATE.names] == [0, 8, 16, 24, 28]
    assert list(Sq.STATE.names) == [f[0] for f in _lib.FmSquelchState._fields_]
    head = [f[0] for f in _lib.ROWS_FIELDS]
    assert [f[0] for f in _lib.FmSquelchIO._fields_][:len(head)] == head      # the rows, as in every io


def _io(**kw):
    io = _lib.FmSquelchIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = BASE, 96000, 96000, 2
    io.kind, io.flags, io.window, io.hang = _lib.FEED_F32, 0, 96, 3
    io.open_level, io.close_level = 1 << 40, 1 << 38
    io.d_energy, io.d_gate, io.win_stride = BASE + (1 << 24), BASE + (1 << 25), 1001
    io.d_nwindows, io.d_spans, io.d_nspans, io.span_cap = BASE + (1 << 26), BASE + (1 << 27), BASE + (1 << 28), 8
    io.d_audio, io.audio_stride = BASE + (1 << 29), 96000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_the_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx

    def rc(ctx=ctx, io=True, **kw):
        return lib.mifsk_fm_squelch_batch(ctx, C.byref(_io(**kw)) if io else None, None)

    # 1: a NULL ctx, io, d_samples or d_nwindows
    assert rc(ctx=None) == EINVAL and rc(io=False) == EINVAL
    assert rc(d_samples=None) == EINVAL and rc(d_nwindows=None) == EINVAL
    # 2: the rows
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    # 3: the kind
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    # 4: flags
    assert rc(flags=1) == EINVAL and rc(flags=0x80000000) == EINVAL
    # 5: the input base, and rows of whole 16-byte vectors of complex elements: 2 of float32, 4 of PCM16
    assert rc(d_samples=BASE + 8) == EINVAL and rc(kind=_lib.FEED_S16, d_samples=BASE + 4) == EINVAL
    assert rc(stream_stride=96001) == EINVAL and rc(kind=_lib.FEED_S16, stream_stride=96002) == EINVAL
    # 6: the window
    assert rc(window=0) == EINVAL and rc(window=32769) == EINVAL and rc(window=0xFFFFFFFF) == EINVAL
    # 7: the levels
    assert rc(close_level=(1 << 40) + 1) == EINVAL and rc(open_level=0, close_level=1) == EINVAL
    # 8: the hang time
    assert rc(hang=(1 << 31) + 1) == EINVAL and rc(hang=0xFFFFFFFF) == EINVAL
    # 9: the capacity rule, kmax / B + 1 entries: kmax is the stride with per-row lengths, else min(nsamples, stride)
    assert rc(win_stride=1000) == EINVAL and rc(win_stride=0) == EINVAL
    assert rc(win_stride=1000, d_energy=None) == EINVAL and rc(win_stride=1000, d_gate=None) == EINVAL
    assert rc(nsamples=9600, d_nsamples=BASE + (1 << 30), win_stride=1000) == EINVAL
    assert rc(window=1, win_stride=96000) == EINVAL
    assert rc(stream_stride=1 << 40, nsamples=0xFFFFFFFF, window=1, win_stride=0xFFFFFFFF) == EINVAL
    # 10: spans want their count
    assert rc(d_nspans=None) == EINVAL
    # 11: the audio rows
    assert rc(audio_stride=95999) == EINVAL and rc(audio_stride=0) == EINVAL
    assert rc(d_audio=BASE + (1 << 29) + 4) == EINVAL and rc(d_audio=BASE + (1 << 29) + 8) == EINVAL
    ladder(rc, dict(audio_stride=95999),
           [dict(d_nwindows=None), dict(nstreams=0), dict(kind=9), dict(flags=2), dict(d_samples=BASE + 8),
            dict(stream_stride=96001), dict(window=0), dict(close_level=1 << 41), dict(hang=0xFFFFFFFF),
            dict(win_stride=7), dict(d_nspans=None)])
    ladder(rc, dict(d_audio=BASE + 4), [dict(d_samples=None), dict(window=40000), dict(win_stride=1000)])
    # what is data, or optional, is not among the checks: the late violation still decides
    late = dict(audio_stride=95999)
    assert rc(win_stride=0, d_energy=None, d_gate=None, **late) == EINVAL
    assert rc(d_spans=None, d_nspans=None, span_cap=0, **late) == EINVAL
    assert rc(d_state=BASE + 4, d_state_out=BASE + 4, **late) == EINVAL
    assert rc(hang=1 << 31, open_level=(1 << 64) - 1, close_level=(1 << 64) - 1, window=32768, **late) == EINVAL
    assert rc(hang=0, open_level=0, close_level=0, window=1, win_stride=96001, **late) == EINVAL


def test_the_level_helper(lib):
    """rint(10^(dbfs / 10) 2^40 B) in double, clamped to [1, B 2^48]; the restatement's, and the library's"""
    for window in (1, 96, 4800, 32768):
        for dbfs in (-120.0, -40.0, 0.0, 30.0, -3.0, -17.25):
            want = int(round(10.0 ** (dbfs / 10.0) * 2.0 ** 40 * window))
            want = min(max(want, 1), window << 48)
            assert M.squelch_level(dbfs, window) == want == Sq.ref_level(dbfs, window), (dbfs, window)
            assert lib.mifsk_fm_squelch_level(dbfs, window) == want
        assert M.squelch_level(0.0, window) == window << 40
        assert M.squelch_level(20.0, window) == 100 * window << 40           # 10^2 is exact
        assert M.squelch_level(30.0, window) == window << 48                 # 1000 is above 256: the clamp
        # the clamps: 256 |z|^2 is full scale; nothing, and a NaN, is 1
        top = window << 48
        for dbfs in (24.1, 60.0, 3000.0, float("inf")):
            assert M.squelch_level(dbfs, window) == top == Sq.ref_level(dbfs, window), dbfs
        for dbfs in (-400.0, -3000.0, float("-inf"), float("nan")):
            assert M.squelch_level(dbfs, window) == 1 == Sq.ref_level(dbfs, window), dbfs
    assert M.squelch_level(-120.0, 1) == 1 and M.squelch_level(-120.0, 96) == 106     # 1.0995, 105.55
    assert M.squelch_level(0.0, 0) == 0 == Sq.ref_level(0.0, 0)
