"""The resident session's entries (mifsk_session_feed_ex, mifsk_session_feed_device,
mifsk_session_info_get; include/mifsk.h "the resident session"): the symbols, the struct's layout
and what is refused before any HIP call, so everything below runs on a machine without a device."""
import ctypes as C

import pytest

from minimodem_amd import _lib

EINVAL = -22
NEW = ("mifsk_session_feed_ex", "mifsk_session_feed_device", "mifsk_session_info_get")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_new_symbols_resolve_and_the_abi_version_stays_8(lib):
    assert lib.mifsk_abi_version() == 8
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_the_header_declares_the_flag_the_kinds_and_the_entries():
    import os
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mifsk.h")).read()
    for name in NEW + ("mifsk_session_info",):
        assert name in hdr, name
    assert "#define MIFSK_SESSION_RESIDENT\t0x2000u" in hdr and _lib.SESSION_RESIDENT == 0x2000
    assert "#define MIFSK_FEED_F32\t0u" in hdr and "#define MIFSK_FEED_S16\t1u" in hdr
    assert (_lib.FEED_F32, _lib.FEED_S16) == (0, 1)
    # no flag of mifsk_session_create shares a bit with another
    flags = [_lib.IO_RING_EXACT, _lib.IO_ENGINE_WORKGROUP, _lib.IO_ENGINE_WAVE, _lib.SESSION_WANT_FRAMES,
             _lib.SESSION_RESIDENT]
    assert sum(flags) == flags[0] | flags[1] | flags[2] | flags[3] | flags[4]


def test_session_info_layout_matches_the_library(lib):
    assert lib.mifsk_abi_sizeof(b"mifsk_session_info") == C.sizeof(_lib.SessionInfo) == 56
    names = [f[0] for f in _lib.SessionInfo._fields_]
    assert names == ["resident", "feeds", "row_capacity", "device_bytes", "h2d_bytes_last", "h2d_bytes_total",
                     "reserved"]
    assert _lib.SessionInfo.row_capacity.offset == 8 and _lib.SessionInfo.reserved.offset == 40
    # the struct beside it did not move
    assert lib.mifsk_abi_sizeof(b"mifsk_session_result") == C.sizeof(_lib.SessionResult)


def test_a_null_session_is_refused(lib):
    cnt = (C.c_uint32 * 1)(4)
    buf = (C.c_float * 4)()
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    info = _lib.SessionInfo()
    assert lib.mifsk_session_feed_ex(None, ptrs, cnt, _lib.FEED_F32, C.c_float(0.0), 0) == EINVAL
    assert lib.mifsk_session_feed_ex(None, None, None, _lib.FEED_S16, C.c_float(0.05), 1) == EINVAL
    assert lib.mifsk_session_feed_device(None, C.c_void_p(1 << 20), 4, cnt, _lib.FEED_F32, C.c_float(0.0), 0,
                                         _lib.PIPELINE_NO_PRODUCER) == EINVAL
    assert lib.mifsk_session_feed_device(None, None, 0, None, _lib.FEED_S16, C.c_float(0.0), 1, None) == EINVAL
    assert lib.mifsk_session_info_get(None, C.byref(info)) == EINVAL
    assert lib.mifsk_session_info_get(None, None) == EINVAL
