"""What tests/test_channel_stream_args.py and tests/test_gpu_channel_stream.py share: the channel stream's host
restatement (channel_ref_stream[_iq] of tools/channel_ref.c, compiled by _phase.ref_lib), the Python loop
around it that keeps a tail and is the host model of the whole object, the counting of outputs done the
slow way, and the cuts of a row."""
import ctypes as C

import numpy as np

import _phase
from _channel import COMPLEX, F32, KINDS, S16, d_rules, same_f32, size_cases  # noqa: F401 (for the tests)
from _channel_iq import centres_of, random_rows  # noqa: F401 (for the tests)

_ARGS = (C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
         C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p)


def ref_lib():
    return _phase.ref_lib("channel_ref", (("channel_ref_stream", C.c_uint64, _ARGS),
                                          ("channel_ref_stream_iq", C.c_uint64, _ARGS)))


def outputs_upto(T, D, n):
    """M(n), in Python's integers"""
    return (n - T) // D + 1 if n >= T else 0


def brute_outputs(T, D, seen, k):
    """the m whose last element, m D + T - 1, is one of elements seen .. seen + k: counted one by one, from the
    first candidate on (no output below M(seen) - 1 or above M(seen + k) can qualify)"""
    lo = max(0, (seen - T) // D - 1)
    count, m = 0, lo
    while m * D + T - 1 < seen + k:
        count += m * D + T - 1 >= seen
        m += 1
    return count


class HostStream:
    """One stream of the object on the host: a record (seen, next) and a tail, around channel_ref_stream[_iq].
    feed(piece) -> float32 [K, count] ([K, count, 2] with iq): what this piece completes."""

    def __init__(self, kind, P, taps, D, centres, r, iq=False, seen=0):
        self.kind, self.P, self.D, self.r, self.iq = kind, int(P), int(D), int(r), iq
        self.taps = np.ascontiguousarray(taps, F32)
        self.centres = np.ascontiguousarray(centres, np.int32)
        self.seek(seen)

    def seek(self, seen=0):
        self.seen, self.next = int(seen), -(-int(seen) // self.D)
        self.tail = None

    def feed(self, piece):
        piece = np.ascontiguousarray(piece)
        assert piece.dtype == (np.int16 if self.kind & S16 else F32) and piece.ndim == (2 if self.kind & COMPLEX else 1)
        T, D, K = self.taps.size, self.D, self.centres.size
        first = self.next * D                               # the absolute index of the buffer's element 0
        if self.tail is not None and len(self.tail):
            assert first + len(self.tail) == self.seen and len(self.tail) <= T - 1
            x = np.concatenate([self.tail, piece])
        else:
            assert first >= self.seen
            x = piece[first - self.seen:]                   # (elements in front of `first`: read by nobody)
        x = np.ascontiguousarray(x)
        n = x.shape[0]
        M = outputs_upto(T, D, n)
        out = np.zeros((K, max(M, 1)) + ((2,) if self.iq else ()), F32)
        g = np.empty((T, 2), np.float64)
        fn = ref_lib().channel_ref_stream_iq if self.iq else ref_lib().channel_ref_stream
        got = fn(x.ctypes.data, n, self.next, self.kind, self.P, T, self.taps.ctypes.data, D, K,
                 self.centres.ctypes.data, self.r, out.ctypes.data, out.shape[1], g.ctypes.data)
        assert got == M
        self.seen += piece.shape[0]
        self.next += M
        self.tail = x[M * D:].copy()
        return out[:, :M]


def cut_points(rng, n, T, D, extra=()):
    """Lengths that sum to n: pieces of 0, 1, D - 1, D, T - 1 and T, three consecutive pieces shorter than T
    (the tail grows across feeds that deliver nothing once it is short of T), `extra` lengths, and seeded
    random ones for the rest, shuffled but for the short run, which stays together."""
    short = [max(1, (T - 1) // 3)] * 3 if T > 3 else [1, 0, 1]
    fixed = [0, 1, max(D - 1, 0), D, T - 1, T] + list(extra)
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
