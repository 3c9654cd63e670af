"""The resident session's entries (mifsk_session_feed_ex, mifsk_session_feed_device,
mifsk_session_info_get; include/mifsk.h "the resident session"): the flags and what is refused before any
HIP call, so everything below runs on a machine without a device."""
import ctypes as C

from _abi import EINVAL, lib  # noqa: F401
from minimodem_amd import _lib


def test_no_flag_of_session_create_shares_a_bit_with_another():
    flags = [_lib.IO_RING_EXACT, _lib.IO_ENGINE_WORKGROUP, _lib.IO_ENGINE_WAVE, _lib.SESSION_WANT_FRAMES,
             _lib.SESSION_RESIDENT]
    assert sum(flags) == flags[0] | flags[1] | flags[2] | flags[3] | flags[4]


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
