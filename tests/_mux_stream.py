"""What tests/test_mux_stream_args.py and tests/test_gpu_mux_stream.py share: the multiplexer stream's host
restatement (mux_ref_stream[_iq] of tools/mux_ref.c, compiled by _phase.ref_lib), the Python loop around it that
keeps the record and the tails and is the host model of the whole object, the whole-row restatements of both
input kinds behind one name, and the cuts of a row."""
import ctypes as C

import numpy as np

import _mux as Mx
import _mux_iq as Mq
import _phase
from _mux import COMPLEX, F32, KINDS, S16, full_outputs, same_bits, size_cases, vec_of  # noqa: F401 (for the tests)

_ARGS = (C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32,
         C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


def ref_lib():
    return _phase.ref_lib("mux_ref", (("mux_ref_stream", C.c_uint64, _ARGS), ("mux_ref_stream_iq", C.c_uint64, _ARGS)))


def drain_of(T, L):
    """H = ceil(T / L) - 1, in Python's integers"""
    return -(-T // L) - 1


def random_rows(rng, iq, nrows, n, scale=1.0):
    """float32 [nrows, n] or, iq, [nrows, n, 2]"""
    return (rng.standard_normal((nrows, n, 2) if iq else (nrows, n)) * scale).astype(F32)


def ref_whole(x, lens, kind, P, taps, L, centres, r, gains=None, iq=False, out_stride=None):
    """mux_ref / mux_ref_iq on one stream's whole rows -> (out [out_stride(, 2)], count)"""
    fn = Mq.ref_multiplex_iq if iq else Mx.ref_multiplex
    return fn(x, lens, kind, P, taps, L, centres, r, gains=gains, out_stride=out_stride)


class HostMuxStream:
    """One stream of the object on the host: a record (seen, first) and the tails [K, H(, 2)], around
    mux_ref_stream[_iq].  feed(pieces) -> the k * L outputs of this feed, [k L] or [k L, 2] of the kind."""

    def __init__(self, kind, P, taps, L, centres, r, gains=None, iq=False, seen=0):
        self.kind, self.P, self.L, self.r, self.iq = kind, int(P), int(L), int(r), iq
        self.taps = np.ascontiguousarray(taps, F32)
        self.centres = np.ascontiguousarray(centres, np.int32)
        self.gains = None if gains is None else np.ascontiguousarray(gains, F32)
        self.K, self.H = self.centres.size, drain_of(self.taps.size, self.L)
        self.tails = np.zeros((self.K, self.H) + ((2,) if iq else ()), F32)       # zeroed at create
        self.seek(seen)

    def seek(self, seen=0):
        """(the tails stay as they are: the index compare excludes them, not their contents)"""
        self.seen = self.first = int(seen)

    def feed(self, pieces):
        """pieces: one array per row, [n_k] or [n_k, 2]; the stream advances by the longest"""
        assert len(pieces) == self.K
        K, H, L, T = self.K, self.H, self.L, self.taps.size
        k = max(p.shape[0] for p in pieces)
        if k == 0:
            return np.zeros((0, 2) if self.kind & COMPLEX else (0,), np.int16 if self.kind & S16 else F32)
        buf = np.zeros((K, H + k) + ((2,) if self.iq else ()), F32)               # +0.0 behind a shorter piece
        buf[:, :H] = self.tails
        for row, p in enumerate(pieces):
            assert p.dtype == F32 and p.ndim == (2 if self.iq else 1)
            buf[row, H:H + p.shape[0]] = p
        out = np.full((k * L, 2) if self.kind & COMPLEX else (k * L,), 99, np.int16 if self.kind & S16 else F32)
        g = np.empty((T, 2), np.float64)
        fn = ref_lib().mux_ref_stream_iq if self.iq else ref_lib().mux_ref_stream
        got = fn(buf.ctypes.data, H + k, H, k, self.seen, self.first, self.kind, self.P, T, self.taps.ctypes.data, L, K,
                 self.centres.ctypes.data, self.r, None if self.gains is None else self.gains.ctypes.data,
                 out.ctypes.data, k * L, g.ctypes.data)
        assert got == k * L
        self.tails = buf[:, k:].copy()                      # the last H of [old tail | piece continued to k]
        self.seen += k
        return out


def cut_points(rng, n, H, extra=()):
    """Lengths that sum to n: pieces of 0, 1, 7, 8, 9, H - 1, H and H + 1, three consecutive pieces shorter than H
    (the tail is then made of several pieces), `extra` lengths, and seeded random ones for the rest, shuffled but
    for the short run, which stays together."""
    short = [max(1, H // 3)] * 3 if H > 3 else [1, 0, 1]
    fixed = [0, 1, 7, 8, 9, max(H - 1, 0), H, H + 1] + list(extra)
    rest = n - sum(short) - sum(fixed)
    assert rest > 0, "the row is too short for its cuts"
    parts = []
    while rest > 0:
        k = int(min(rest, rng.integers(1, max(2, n // 4))))
        parts.append(k)
        rest -= k
    groups = [[k] for k in fixed + parts] + [short]
    order = rng.permutation(len(groups))
    cuts = [k for i in order for k in groups[i]]
    assert sum(cuts) == n
    return cuts


def even_feeds(cuts):
    """every stream as many pieces: the shorter lists get pieces of 0 at their ends"""
    n = max(len(c) for c in cuts)
    return [c + [0] * (n - len(c)) for c in cuts]
