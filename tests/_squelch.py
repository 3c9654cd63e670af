"""What tests/test_squelch_args.py, tests/test_squelch_ref.py and tests/test_gpu_squelch.py share: the power
squelch's host restatement (tools/squelch_ref.c) as a temporary shared object (_phase.ref_lib), the state
record as a numpy dtype, the values that mark cells a call must not write, rows cut into pieces, and spans
merged on their first window."""
import ctypes as C

import numpy as np

import _phase
from _phase import F32, ROOT, same_bits  # noqa: F401 (for the tests)

F32K, S16K = 0, 1                       # MIFSK_FEED_F32 / MIFSK_FEED_S16
U32, U64, VP = C.c_uint32, C.c_uint64, C.c_void_p
TILE = 2048                             # the energy launch's samples per workgroup: 256 threads x 8
FULL = 1 << 48                          # the energy of a sample that is out of range
STATE = np.dtype([("seen", "<u8"), ("acc", "<u8"), ("span_first", "<u8"), ("open", "<u4"), ("low", "<u4")])
assert STATE.itemsize == 32
# what a cell holds that no call has written (the same bits as int64 / uint64, uint8, int32 / uint32)
FILL64, FILL8, FILL32 = 0x7E7E7E7E7E7E7E7E, 0x7E, 0x7E7E7E7E


def ref_lib():
    """tools/squelch_ref.c as a shared object"""
    return _phase.ref_lib("squelch_ref", (
        ("squelch_ref_scale", U64, (C.c_double,)),
        ("squelch_ref_energy", U64, (C.c_float, C.c_float)),
        ("squelch_ref_energies", None, (VP, U64, VP)),
        ("squelch_ref_level", U64, (C.c_double, U32)),
        ("squelch_ref_rows", None, (VP, U64, VP, U32, C.c_int, U32, U32, U32, U64, U64, VP, VP, VP, VP, U64, VP, VP, VP,
                                    U32, VP, U64))))


def ref_energies(iq):
    """the energy of every sample of float32 [..., 2] -> uint64 [...]"""
    iq = np.ascontiguousarray(iq, F32)
    out = np.empty(iq.shape[:-1], np.uint64)
    ref_lib().squelch_ref_energies(iq.ctypes.data, out.size, out.ctypes.data)
    return out


def ref_level(dbfs, window):
    return int(ref_lib().squelch_ref_level(dbfs, window))


def win_stride_of(kmax, window):
    """the capacity rule: entries a row of energies and gates needs"""
    return kmax // window + 1


def ref_squelch(iq, lens, window, open_level, close_level=None, hang=0, state=None, audio=None, span_cap=8,
                nsamples=None, win_stride=None, want=("energy", "gate", "spans", "state")):
    """The restatement on host arrays.  iq: float32 or int16 [nstreams, stride, 2]; lens: uint32 [nstreams] or None
    (then `nsamples` for all, default the width); state: STATE [nstreams] or None; audio: float32 [nstreams,
    audio_stride] or None (a copy is muted) -> {"energy": uint64 [nstreams, win_stride], "gate": uint8 likewise,
    "nwindows": uint32 [nstreams], "spans": uint64 [nstreams, span_cap, 2], "nspans": uint32 [nstreams], "state":
    STATE [nstreams], "audio"}; cells that the definition leaves alone hold FILL64, FILL8, FILL32.  want: the optional
    arrays that are given ("nspans": the count without the spans); the others stay as they were filled."""
    iq = np.ascontiguousarray(iq)
    assert iq.dtype in (np.float32, np.int16) and iq.ndim == 3 and iq.shape[2] == 2
    nstreams, stride = iq.shape[:2]
    if lens is not None:
        lens = np.ascontiguousarray(lens, np.uint32)
        assert lens.shape == (nstreams,)
    nsamples = stride if nsamples is None else nsamples
    kmax = stride if lens is not None else min(nsamples, stride)
    win_stride = win_stride_of(kmax, window) if win_stride is None else win_stride
    if state is not None:
        state = np.ascontiguousarray(state, STATE)
        assert state.shape == (nstreams,)
    out = {"energy": np.full((nstreams, win_stride), FILL64, np.uint64), "gate": np.full((nstreams, win_stride), FILL8, np.uint8),
           "nwindows": np.full(nstreams, FILL32, np.uint32), "spans": np.full((nstreams, span_cap, 2), FILL64, np.uint64),
           "nspans": np.full(nstreams, FILL32, np.uint32), "state": np.zeros(nstreams, STATE),
           "audio": None if audio is None else np.array(audio, F32, order="C")}
    ptr = lambda name: out[name].ctypes.data if name in want else None      # noqa: E731
    ref_lib().squelch_ref_rows(
        iq.ctypes.data, stride, None if lens is None else lens.ctypes.data, nsamples, nstreams,
        S16K if iq.dtype == np.int16 else F32K, window, hang, open_level, open_level if close_level is None else close_level,
        None if state is None else state.ctypes.data, ptr("state"), ptr("energy"), ptr("gate"), win_stride,
        out["nwindows"].ctypes.data, ptr("spans"), out["nspans"].ctypes.data if {"spans", "nspans"} & set(want) else None, span_cap,
        None if audio is None else out["audio"].ctypes.data, 0 if audio is None else out["audio"].shape[1])
    return out


def merge_spans(calls):
    """the spans of consecutive calls ((spans, nspans) of one row each, none cut by span_cap) merged on
    first_window -> [(first, end)]"""
    merged = {}
    for spans, n in calls:
        assert n <= len(spans)
        for first, end in spans[:n]:
            merged[int(first)] = int(end)
    return sorted(merged.items())


def ref_pieces(iq, cuts, window, open_level, close_level=None, hang=0, audio=None, state=None, span_cap=8):
    """One row (float32 or int16 [n, 2]) fed to the restatement in pieces of `cuts` elements, the state handed on ->
    (energies, gates, merged spans, the last state, the muted audio or None)"""
    at, energy, gate, calls = 0, [], [], []
    audio = None if audio is None else np.array(audio, F32)
    vec = 4 if iq.dtype == np.int16 else 2
    for k in cuts:
        piece = np.zeros((1, max(vec, -(-k // vec) * vec), 2), iq.dtype)
        piece[0, :k] = iq[at:at + k]
        r = ref_squelch(piece, [k], window, open_level, close_level, hang, state=state, span_cap=span_cap,
                        audio=None if audio is None else np.concatenate([audio[at:at + k], np.zeros(piece.shape[1] - k, F32)])[None])
        nw = int(r["nwindows"][0])
        energy.append(r["energy"][0, :nw])
        gate.append(r["gate"][0, :nw])
        calls.append((r["spans"][0], int(r["nspans"][0])))
        if audio is not None:
            audio[at:at + k] = r["audio"][0, :k]
        state, at = r["state"], at + k
    return np.concatenate(energy), np.concatenate(gate), merge_spans(calls), state, audio
