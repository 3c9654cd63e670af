"""The C ABI as Python states it (minimodem_amd/_lib.py: STRUCTS, SIGNATURES and the constants;
minimodem_amd/__init__.py: DTYPES) against include/*.h as _abi.py reads them and against the library's own
mifsk_abi_sizeof: every struct, every function, every integer macro with a Python name.  No device, no
compute call."""
import ctypes as C

import _abi as A
import _oracle as O
import minimodem_amd as M
from _abi import lib  # noqa: F401
from minimodem_amd import _lib

# Every size, offset and value that is pinned by number (the rest of this file compares three statements
# of the ABI with each other; this table is what none of them may move to together).
PINNED = {
    "abi_version": 8,
    "sizeof": {
        "fsk_plan": 64, "mifsk_search": 32, "mifsk_search_result": 24, "mifsk_time_split": 24,
        "mifsk_time_split_stats": 64, "mifsk_session_info": 56, "mifsk_softbits_io": 88, "mifsk_carrier_io": 88,
        "mifsk_channel_params": 48, "mifsk_channel_io": 64, "mifsk_mux_params": 56, "mifsk_mux_io": 64,
        "mifsk_impair_io": 120, "mifsk_fm_demod_io": 80, "mifsk_fm_mod_io": 96,
    },
    "offsetof": {
        "fsk_plan": {"fftplan": 40},
        "mifsk_session_info": {"row_capacity": 8, "h2d_bytes_last": 24, "reserved": 40},
        "mifsk_softbits_io": {"kind": 32, "d_origin": 40},
        "mifsk_carrier_io": {"kind": 32, "first": 40, "d_band": 64},
        "mifsk_channel_params": {"centres": 32},
        "mifsk_channel_io": {"d_rows": 32, "d_nout": 56},
        "mifsk_mux_params": {"centres": 32, "gains": 48},
        "mifsk_mux_io": {"d_out": 32, "d_nout": 56},
        "mifsk_impair_io": {"kind": 32, "out_kind": 36, "d_out": 40, "seed": 56, "first_sample": 72, "d_gain": 80,
                            "gain": 104, "flags": 116},
        "mifsk_fm_demod_io": {"kind": 32, "flags": 36, "d_out": 40, "out_stride": 48, "d_prev": 56, "d_last": 64,
                              "gain": 72, "reserved": 76},
        "mifsk_fm_mod_io": {"out_kind": 32, "flags": 36, "d_out": 40, "out_stride": 48, "deviation": 56,
                            "centre": 64, "d_phase0": 72, "d_phase_out": 80, "amplitude": 88, "reserved": 92},
    },
    "constants": {
        "MIFSK_ABI_VERSION": 8, "MIFSK_FEED_F32": 0, "MIFSK_FEED_S16": 1, "MIFSK_CARRIER_NONE": -1,
        "MIFSK_CARRIER_NO_WINDOW": -2, "MIFSK_CHANNEL_COMPLEX": 1, "MIFSK_MUX_COMPLEX": 1,
        "MIFSK_SESSION_RESIDENT": 0x2000,
    },
}

# the header macros Python mirrors under the same name (less the MIFSK_), in _lib or in the package
MIRRORED = ["MIFSK_IO_RING_EXACT", "MIFSK_IO_ENGINE_WORKGROUP", "MIFSK_IO_ENGINE_WAVE", "MIFSK_IO_HOST_S16",
            "MIFSK_NCOUNTERS", "MIFSK_WANT_BYTES", "MIFSK_WANT_BITS", "MIFSK_WANT_FRAMES", "MIFSK_WANT_EPISODES",
            "MIFSK_GATHER_ID_BYTES", "MIFSK_GATHER_LOOPBACK", "MIFSK_STATE_FINISHED", "MIFSK_TIME_SPLIT_REJECT_ALL",
            "MIFSK_SESSION_WANT_FRAMES", "MIFSK_SESSION_RESIDENT", "MIFSK_FEED_F32", "MIFSK_FEED_S16",
            "MIFSK_CARRIER_NONE", "MIFSK_CARRIER_NO_WINDOW", "MIFSK_CHANNEL_COMPLEX", "MIFSK_MUX_COMPLEX",
            "MIFSK_TEXT_PRINT_FILTER", "MIFSK_TEXT_QUIET", "MIFSK_FILES_WANT_FRAMES"]

STRUCT_NAMES = {cls: name for name, cls in _lib.STRUCTS.items()}


def _python_constants(name):
    """the values Python gives header macro `name`: _lib's and the package's, where they have one"""
    return [getattr(mod, name[len("MIFSK_"):]) for mod in (_lib, M) if hasattr(mod, name[len("MIFSK_"):])]


def _ctypes_field(t):
    """(kind, bytes, count) of a ctypes field type, in _abi.header_structs' terms"""
    count = 1
    if issubclass(t, C.Array):
        t, count = t._type_, t._length_
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        kind = "pointer"
    elif issubclass(t, C.Structure):
        kind = "struct " + STRUCT_NAMES[t]
    elif t in (C.c_float, C.c_double):
        kind = "float"
    else:
        kind = {True: "signed", False: "unsigned"}[t._type_ in "cbhilq"]
        assert t._type_ in "cbhilqBHILQ", t
    return kind, C.sizeof(t), count


def _mirror_fields(cls):
    return [(name,) + _ctypes_field(t) for name, t in cls._fields_]


def _dtype_fields(dtype):
    kinds = {"u": "unsigned", "i": "signed", "f": "float"}
    return [(name, kinds[dtype[name].kind], dtype[name].itemsize, 1) for name in dtype.names]


def test_every_header_struct_has_a_mirror_and_every_mirror_a_header_struct():
    header = A.header_structs()
    assert set(header) == set(_lib.STRUCTS) | set(M.DTYPES)
    assert len(_lib.STRUCTS) == 26 and len(M.DTYPES) == 5 and len(header) == 29
    assert len(STRUCT_NAMES) == len(_lib.STRUCTS)                    # no mirror under two names


def test_the_mirrors_fields_are_the_headers_in_name_order_kind_and_width():
    header = A.header_structs()
    for name, cls in _lib.STRUCTS.items():
        assert [f[0] for f in cls._fields_] == [f[0] for f in header[name]], name
        assert _mirror_fields(cls) == header[name], name
        assert C.sizeof(cls) == A.header_sizeof(name), name
    for name, dtype in M.DTYPES.items():
        assert list(dtype.names) == [f[0] for f in header[name]], name
        assert _dtype_fields(dtype) == header[name], name
        assert dtype.itemsize == A.header_sizeof(name), name


def test_the_library_was_built_with_the_mirrors_sizes(lib):
    """mifsk_abi_sizeof knows every public struct, and says what the mirror says"""
    for name, cls in _lib.STRUCTS.items():
        assert lib.mifsk_abi_sizeof(name.encode()) == C.sizeof(cls) != 0, name
    for name, dtype in M.DTYPES.items():
        assert lib.mifsk_abi_sizeof(name.encode()) == dtype.itemsize != 0, name
    assert lib.mifsk_abi_sizeof(b"no such struct") == 0 and lib.mifsk_abi_sizeof(b"") == 0
    # the oracle's own mirrors of the two configuration structs
    assert C.sizeof(_lib.RxConfig) == C.sizeof(O.RxConfig)
    assert C.sizeof(_lib.ModemArgs) == C.sizeof(O.ModemArgs)


def test_every_prototype_is_bound_with_its_argument_count_and_return_class(lib):
    declared = A.header_functions()
    assert len(declared) == 107
    assert list(declared) == list(_lib.SIGNATURES) == _lib.EXPORTS, set(declared) ^ set(_lib.SIGNATURES)
    classes = {None: "void", C.c_int: "int", C.c_float: "float", C.c_double: "double", C.c_long: "long",
               C.c_uint: "unsigned", C.c_size_t: "u64", C.c_uint64: "u64", C.c_void_p: "pointer",
               C.c_char_p: "pointer"}
    for name, (kind, nargs) in declared.items():
        fn = getattr(lib, name)                                       # the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name     # load() bound it so
        assert len(argtypes) == nargs, name
        if restype is not None and issubclass(restype, C._Pointer):
            assert kind == "pointer", name
        else:
            assert kind == classes[restype], name


def test_every_mirrored_macro_has_the_headers_value():
    header = A.header_constants()
    mirrored = [name for name in header if _python_constants(name)]
    assert sorted(mirrored) == sorted(MIRRORED)
    for name in mirrored:
        for value in _python_constants(name):
            assert value == header[name] and type(value) is int, name
    assert _lib.MAX_BITS == header["MIFSK_MAX_FRAME_BITS"]
    assert sorted(n for n in header if n.startswith("MIFSK_FEED_")) == ["MIFSK_FEED_F32", "MIFSK_FEED_S16"]
    # the work counters: Python's name is the macro's tail, but for the one renamed since
    renamed = {"cyc_parallel": "cyc_scan"}
    counters = {n[len("MIFSK_CNT_"):].lower(): v for n, v in header.items() if n.startswith("MIFSK_CNT_")}
    assert len(counters) == 15
    for tail, value in counters.items():
        assert M.COUNTER_NAMES[value] == renamed.get(tail, tail), tail
    assert max(M.COUNTER_NAMES) < M.NCOUNTERS
    routines = {n[len("MIFSK_SELFTEST_CORR_"):].lower(): v for n, v in header.items()
                if n.startswith("MIFSK_SELFTEST_CORR_")}
    assert routines == _lib.CORR_ROUTINES


def test_the_pinned_numbers(lib):
    header = A.header_constants()
    assert lib.mifsk_abi_version() == PINNED["abi_version"] == header["MIFSK_ABI_VERSION"]
    for name, size in PINNED["sizeof"].items():
        mirrors = [C.sizeof(_lib.STRUCTS[name])] if name in _lib.STRUCTS else []
        mirrors += [M.DTYPES[name].itemsize] if name in M.DTYPES else []
        assert mirrors and all(m == size for m in mirrors), name
    for name, offsets in PINNED["offsetof"].items():
        for field, offset in offsets.items():
            assert getattr(_lib.STRUCTS[name], field).offset == offset, (name, field)
    for name, value in PINNED["constants"].items():
        assert header[name] == value, name
        assert all(v == value for v in _python_constants(name)), name
