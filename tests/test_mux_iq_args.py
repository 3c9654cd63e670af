"""The multiplexer's I/Q entry (include/mifsk/mux_iq.h, minimodem_amd/csrc/mifsk_mux.hip) without a device:
where it is declared and how it is bound, what it refuses without a plan or an io, its host restatement
mux_ref_iq (tools/mux_ref.c) against a float64 evaluation of the definition, against the real entry's
restatement where Q is +0.0, and through the PCM16 conversion, and the condition the GPU test's end-to-end
case relies on: the host chain's audio rows decode through the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _abi as A
import _channel_iq as Iq
import _mux as Mx
import _mux_iq as Mq
import _oracle as O
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32
ENTRY = "mifsk_multiplex_iq_batch"
HEADER = "mifsk/mux_iq.h"


def test_the_extension_header_declares_that_one_prototype_and_the_abi_tables_do_not():
    path = os.path.join(A.ROOT, "include", *HEADER.split("/"))
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert '#include "../mifsk.h"' in text
    code = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    found = re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", code)
    assert [(" ".join(ret.split()), name, args.count(",") + 1) for ret, name, args in found] == [("int", ENTRY, 3)]
    assert not re.search(r"\bstruct\s+\w+\s*\{", code)              # no struct body
    assert not re.findall(r"^#define[ \t]+MIFSK_\w+[ \t]+\S", text, re.M)   # no macro with a value
    # the tables tests/test_abi.py and tests/test_channel_iq_args.py pin stay as they are
    assert ENTRY not in list(_lib.SIGNATURES) and ENTRY not in _lib.EXPORTS and ENTRY not in A.header_functions()
    assert ENTRY not in _lib.EXT_SIGNATURES
    assert A.header_constants()["MIFSK_ABI_VERSION"] == 8
    # one table per extension header, no name twice
    assert list(_lib.EXTENSIONS) == ["mifsk/channel_iq.h", HEADER]
    assert _lib.EXTENSIONS["mifsk/channel_iq.h"] is _lib.EXT_SIGNATURES and list(_lib.EXTENSIONS[HEADER]) == [ENTRY]
    for header in _lib.EXTENSIONS:
        assert os.path.exists(os.path.join(A.ROOT, "include", *header.split("/"))), header
    names = [n for table in _lib.EXTENSIONS.values() for n in table]
    assert len(names) == len(set(names)) and not set(names) & set(_lib.SIGNATURES)


def test_the_entry_is_bound_with_the_real_entrys_arguments(lib):
    restype, argtypes = _lib.EXTENSIONS[HEADER][ENTRY]
    fn = getattr(lib, ENTRY)
    assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(_lib.MuxIO), C.c_void_p]
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert argtypes == _lib.SIGNATURES["mifsk_multiplex_batch"][1]          # the real entry's io: no new struct


def test_the_entry_refuses_without_a_plan_or_an_io(lib, fake_ctx):
    """the two refusals that need no plan: a NULL plan (with or without an io), and a NULL io behind a plan
    that is then never looked into (a block of zeroed host memory stands in for it)"""
    fn = getattr(lib, ENTRY)
    io = _lib.MuxIO()
    io.d_samples, io.stream_stride, io.d_nsamples, io.nsamples, io.nstreams = A.BASE, 4000, None, 4000, 2
    io.d_out, io.out_stride, io.nout_cap, io.d_nout = A.BASE + (1 << 24), 16000, 16000, A.BASE + (1 << 26)
    assert fn(None, None, None) == EINVAL
    assert fn(None, C.byref(io), None) == EINVAL
    assert fn(fake_ctx[0], None, None) == EINVAL


def test_the_python_surface_has_the_switch():
    import inspect
    assert list(inspect.signature(M.multiplex).parameters) == ["plan", "samples", "nsamples", "nout_cap", "stream",
                                                               "out", "iq"]
    assert inspect.signature(M.multiplex).parameters["iq"].default is False


def _small_case(name, L, T, K, P, gains):
    """one stream of K rows of ceil(T / L) + 12 elements at most, ragged -> (kind, taps, centres, x, lens, gains)"""
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + L + 7 * gains)
    n = -(-T // L) + 12
    taps = M.channel_taps(T, 1200.0, 192000.0, float(L)) if T > 2 else rng.standard_normal(T).astype(F32)
    centres = Iq.centres_of(rng, K, P) if P > 1 else np.zeros(K, np.int32)
    centres = np.array([q if abs(q) < P else 0 for q in centres], np.int32)
    gv = (rng.standard_normal(K) * 2).astype(F32) if gains else None
    x = Mq.iq_rows(rng, K, n, 0.02 if kind & Mq.S16 else 1.0)          # PCM16: inside the range, mostly
    lens = [n] + [int(v) for v in rng.integers(0, n + 1, K - 1)]
    return kind, taps, centres, x, lens, gv


def _cases():
    return [pytest.param(*c, id="%s-L%d-T%d-K%d-P%d" % c) for c in Mq.size_cases()]


@pytest.mark.parametrize("gains", [False, True], ids=["plain", "gains"])
@pytest.mark.parametrize("name,L,T,K,P", _cases())
def test_the_restatement_against_float64(name, L, T, K, P, gains):
    """tests/test_mux_args.py::test_the_restatement_against_float64's bound, the same expression with |x|
    replaced by |I| + |Q|: E = (2 J + 2 K + 40) 2^-52 S[n], S[n] = sum_k |gain_k| sum_j |h[t]| (|I| + |Q|).  It
    still holds: A_k, now with |I| + |Q|, bounds |re|, |im| and every partial sum; re and im each carry 2 J FMA
    roundings where they carried J (J 2^-52 A_k each instead of J / 2), the table, gain, W and channel-chain
    terms are as they were: (2 J + 18 + 16 + 2 K) 2^-52 S <= E.  Derived, not measured."""
    kind, taps, centres, x, lens, gv = _small_case(name, L, T, K, P, gains)
    for r in sorted({0, int(centres[-1])}):
        got, cnt = Mq.ref_multiplex_iq(x, lens, kind, P, taps, L, centres, r, gv)
        want, mag = Mq.numpy_multiplex_iq(x, lens, P, taps, L, centres, r, gv)
        assert cnt == want.size == (x.shape[1] - 1) * L + T and not np.any(got[cnt:])
        J = -(-T // L)
        E = (2 * J + 2 * K + 40) * 2.0 ** -52 * mag
        parts = (want.real, want.imag) if kind & Mq.COMPLEX else (want.real,)
        got = got[:cnt].reshape(cnt, -1).astype(np.float64)
        for c, v in enumerate(parts):
            if kind & Mq.S16:
                t = np.clip(v * 32767.0, -32768.0, 32767.0)
                bound = 0.5 + 2.0 ** -24 * np.abs(t) + 32767.0 * (E + 2.0 ** -24 * np.abs(v) + 2.0 ** -149)
                err = np.abs(got[:, c] - t)
            else:
                bound = E + 2.0 ** -24 * np.abs(v) + 2.0 ** -149
                err = np.abs(got[:, c] - v)
            assert np.all(err <= bound), (name, L, T, K, P, r, c, float((err / bound).max()))


def test_the_restatement_where_there_is_nothing_to_sum():
    for name, kind in Mq.KINDS.items():
        # no output where every row is empty; phases without a tap are exact zeros
        out, cnt = Mq.ref_multiplex_iq(np.ones((2, 8, 2), F32), [0, 0], kind, 7, np.ones(3, F32), 5, [1, 2], 0, None, 16)
        assert cnt == 0 and not np.any(out), name
        out, cnt = Mq.ref_multiplex_iq(np.ones((1, 8, 2), F32), None, kind, 7, np.ones(2, F32), 5, [3], 1, None, 40)
        rows, phase = out.reshape(40, -1)[:37], np.arange(37) % 5
        assert cnt == 37 and not np.any(rows[phase >= 2]) and np.all(rows[phase == 0, 0] != 0), name


@pytest.mark.parametrize("name", list(Mq.KINDS))
def test_with_q_zero_the_restatement_is_the_real_entrys_bit_for_bit(name):
    """Q = +0.0 everywhere, finite samples and taps: the two fma()s that Q adds to each tap step have a product
    of +-0, and neither chain can hold -0 (it starts at +0.0, and a sum that is zero is +0 in round-to-nearest
    unless both terms are -0), so they change nothing: mux_ref_iq == mux_ref on the I plane."""
    kind = Mq.KINDS[name]
    rng = np.random.default_rng(kind + 5)
    for L, T, K, P, n in ((1, 33, 2, 7, 120), (4, 129, 3, 1920, 90), (40, 401, 5, 4800, 30), (65, 64, 2, 1 << 16, 20)):
        taps = M.channel_taps(T, 1200.0, 192000.0, float(L))
        centres = np.array([0, 1, -1, P // 2, -(P - 1)][:K], np.int32)
        gains = (rng.standard_normal(K) * 2).astype(F32)
        x = np.zeros((K, n, 2), F32)
        x[..., 0] = rng.standard_normal((K, n)) * (0.02 if kind & Mq.S16 else 1.0)
        x[0, 5:9, 0] = [0.0, -0.0, 1e-40, -1e-40]                  # zeros of both signs and subnormals in I
        lens = [n] + [int(v) for v in rng.integers(0, n + 1, K - 1)]
        assert not np.any(x[..., 1].view(np.uint32))
        for r in (0, int(centres[-1])):
            got, cnt = Mq.ref_multiplex_iq(x, lens, kind, P, taps, L, centres, r, gains)
            want, wcnt = Mx.ref_multiplex(np.ascontiguousarray(x[..., 0]), lens, kind, P, taps, L, centres, r, gains)
            assert cnt == wcnt and Mq.same_bits(got, want), (name, L, T, r)


@pytest.mark.parametrize("cx", [False, True])
def test_pcm16_rows_are_the_float_rows_through_the_conversion(cx):
    rng = np.random.default_rng(16)
    L, T, P, K, n = 40, 401, 4800, 5, 30
    taps = M.channel_taps(T, 1200.0, 192000.0, float(L))
    centres = Iq.centres_of(rng, K, P)
    x = Mq.iq_rows(rng, K, n, 1.5)                                  # the sum clamps now and then
    x[3, 20, 1] = np.nan
    base = Mq.COMPLEX if cx else 0
    stride = (Mq.full_outputs(n, L, T) + 7) // 8 * 8
    f, nf = Mq.ref_multiplex_iq(x, None, base, P, taps, L, centres, 170, out_stride=stride)
    s, ns = Mq.ref_multiplex_iq(x, None, base | Mq.S16, P, taps, L, centres, 170, out_stride=stride)
    assert nf == ns and np.array_equal(s, Mq.numpy_s16(f))
    assert (s == 32767).any() and (s == -32768).any() and np.isnan(f).any()


@pytest.mark.parametrize("cnr_db", [None, 14.0], ids=["clean", "cnr14"])
def test_the_host_chains_audio_rows_decode_every_fm_channel(cnr_db):
    """The precondition of tests/test_gpu_mux_iq.py's end-to-end case, from the host transmitter's audio at
    48 kHz: fm_ref.c at centre 0, mux_ref_iq (L = 4, 129 taps at 12 kHz that sum to 4, centres -300, 30 and 410 of
    1920), impair_ref.c, channel_ref_iq, fm_ref.c, then the oracle gives each channel's 16 bytes exactly."""
    words, audio, lens = Mq.fm_tx_audio(M)
    host = Mq.fm_host_chain(M, audio, lens, Iq.fm_sigma(M, cnr_db))
    assert host["count"] == (int(lens.max()) - 1) * Mq.L_FM + Mq.TX_NTAPS and host["capture"].shape[0] <= 40000
    assert host["nout"] == (host["count"] - Iq.NTAPS) // Iq.D_FM + 1
    # unit gain with taps that sum to L: every carrier goes through both filters at 0.3 (taps that sum to
    # 2 L would give 0.6; the 6 kHz receive filter's edge ripples the envelope by some per cent)
    env = np.hypot(host["ch"][..., 0], host["ch"][..., 1])
    if cnr_db is None:
        assert np.all(np.abs(env[:, 200:host["nout"] - 200].max(axis=1) / Iq.CARRIER - 1.0) < 0.15)
    ocfg = O.oracle_config("1200")
    for k in range(3):
        assert O.oracle_rx_stream(ocfg, host["audio"][k, :host["nout"]])["bytes"] == words[k].tobytes(), k
