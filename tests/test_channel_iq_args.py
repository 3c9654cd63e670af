"""The channelizer's I/Q entry (include/mifsk/channel_iq.h, minimodem_amd/csrc/mifsk_channel.hip) without a
device: its host restatement channel_ref_iq (tools/channel_ref.c) against the real entry's restatement and
against a float64 evaluation of the definition, what the entry refuses without a plan or an io, how it is
bound, where it is declared, and the condition the GPU test's end-to-end case relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _abi as A
import _channel as Ch
import _channel_iq as Iq
import _oracle as O
import minimodem_amd as M
from _abi import EINVAL, fake_ctx, lib  # noqa: F401
from minimodem_amd import _lib

F32 = np.float32
ENTRY = "mifsk_channelize_iq_batch"


def _cases():
    return [pytest.param(*c, id="%s-T%d-D%d-K%d-P%d" % c) for c in Iq.size_cases()]


def _small_case(name, T, D, K, P):
    """one row of n = T + 40 D + 3 elements, rounded up to the kind's vector -> (kind, taps, centres, row)"""
    kind = Iq.KINDS[name]
    rng = np.random.default_rng(1000 * T + 10 * K + D)
    vec = 16 // ((2 if kind & Iq.S16 else 4) * (2 if kind & Iq.COMPLEX else 1))
    n = (T + 40 * D + 3 + vec - 1) // vec * vec
    taps = M.channel_taps(T, 400.0, 48000.0, 2.0) if T > 2 else rng.standard_normal(T).astype(F32)
    return kind, taps, Iq.centres_of(rng, K, P), Iq.random_rows(rng, kind, 1, n)[0]


@pytest.mark.parametrize("name,T,D,K,P", _cases())
def test_the_i_plane_is_the_real_entrys_restatement_bit_for_bit(name, T, D, K, P):
    kind, taps, centres, x = _small_case(name, T, D, K, P)
    for r in (0, int(centres[-1])):
        iq = Iq.ref_channelize_iq(x, kind, P, taps, D, centres, r)
        real = Ch.ref_channelize(x, kind, P, taps, D, centres, r)
        assert iq.shape == real.shape + (2,) and real.shape[1] >= 41
        assert Iq.same_f32(np.ascontiguousarray(iq[..., 0]), real), (name, r)


@pytest.mark.parametrize("name,T,D,K,P", _cases())
def test_the_q_plane_against_float64(name, T, D, K, P):
    """|restatement - float64| <= 2^-24 |v| + 2^-149 + (2 T + 8) 2^-52 sum_t |h[t]| (|xr| + |xi|): the bound
    tests/test_channel_args.py::test_the_restatement_against_float64 derives for the real plane, the same
    expression: Q has I's operations, with C and S exchanged in the last fma."""
    kind, taps, centres, x = _small_case(name, T, D, K, P)
    for r in (0, int(centres[-1])):
        got = Iq.ref_channelize_iq(x, kind, P, taps, D, centres, r)[..., 1]
        want, mag = Iq.numpy_channelize_q(x, kind, P, taps, D, centres, r)
        assert got.shape == want.shape
        bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -149 + (2 * T + 8) * 2.0 ** -52 * mag[None, :]
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), (name, T, D, P, r, float((err / bound).max()))
        # (and the evaluation this one borrows gives the I plane's value for the I plane)
        want_i, mag_i = Iq.numpy_channelize(x, kind, P, taps, D, centres, r)
        assert np.array_equal(mag, mag_i)
        err = np.abs(Iq.ref_channelize_iq(x, kind, P, taps, D, centres, r)[..., 0].astype(np.float64) - want_i)
        assert np.all(err <= 2.0 ** -24 * np.abs(want_i) + 2.0 ** -149 + (2 * T + 8) * 2.0 ** -52 * mag[None, :])


def test_the_restatement_writes_nothing_behind_its_outputs():
    x = np.ones(64, F32)
    assert Iq.ref_channelize_iq(x, 0, 4800, np.ones(65, F32), 1, [3], 0).shape == (1, 0, 2)
    assert Iq.ref_channelize_iq(x, 0, 4800, np.ones(60, F32), 2, [3, 5], 0).shape == (2, 3, 2)


def test_the_entry_refuses_without_a_plan_or_an_io(lib, fake_ctx):
    """the two refusals that need no plan: a NULL plan (with or without an io), and a NULL io behind a plan
    that is then never looked into (a block of zeroed host memory stands in for it)"""
    fn = getattr(lib, ENTRY)
    io = _lib.ChannelIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = A.BASE, 4000, 4000, 2
    io.d_rows, io.out_stride, io.nout_cap, io.d_nout = A.BASE + (1 << 24), 4000, 4000, A.BASE + (1 << 26)
    assert fn(None, None, None) == EINVAL
    assert fn(None, C.byref(io), None) == EINVAL
    assert fn(fake_ctx[0], None, None) == EINVAL


def test_the_entry_is_bound_with_three_arguments_and_an_int_return(lib):
    restype, argtypes = _lib.EXT_SIGNATURES[ENTRY]
    fn = getattr(lib, ENTRY)
    assert restype is C.c_int and len(argtypes) == 3
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert argtypes[1] is C.POINTER(_lib.ChannelIO)                 # the real entry's io: no new struct
    assert argtypes == _lib.SIGNATURES["mifsk_channelize_batch"][1]


def test_the_extension_header_declares_that_one_prototype_and_the_abi_tables_do_not():
    path = os.path.join(A.ROOT, "include", "mifsk", "channel_iq.h")
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert '#include "../mifsk.h"' in text
    code = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    found = re.findall(r"([\w\s*]+?)\b((?:mifsk|fsk)_\w+)\s*\(([^()]*)\)\s*;", code)
    assert [(" ".join(ret.split()), name, args.count(",") + 1) for ret, name, args in found] == [("int", ENTRY, 3)]
    assert not re.search(r"\bstruct\s+\w+\s*\{", code)              # no struct body
    assert not re.findall(r"^#define[ \t]+MIFSK_\w+[ \t]+\S", text, re.M)   # no macro with a value
    # the tables tests/test_abi.py pins stay the main headers': the entry is in neither
    assert ENTRY not in list(_lib.SIGNATURES) and ENTRY not in _lib.EXPORTS and ENTRY not in A.header_functions()
    assert list(_lib.EXT_SIGNATURES) == [ENTRY]
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)


@pytest.mark.parametrize("cnr_db", [None, 14.0], ids=["clean", "cnr14"])
def test_the_host_chains_audio_rows_decode_every_fm_channel(cnr_db):
    """The precondition of tests/test_gpu_channel_iq.py's end-to-end case, from the host transmitter's audio:
    fm_ref.c, float32 sum, impair_ref.c, channel_ref_iq, fm_ref.c, then the oracle gives each channel's 16
    bytes exactly."""
    words = Iq.fm_messages()
    cfg = M.rx_config("1200", sample_rate=Iq.FS)
    sigs = [M.synthesize(cfg, words[k], amplitude=1.0, leading_silence=Iq.LEAD[k]) for k in range(3)]
    n = (max(s.size for s in sigs) + 3) // 4 * 4
    audio = np.zeros((3, n), F32)
    for k, s in enumerate(sigs):
        audio[k, :s.size] = s
    host = Iq.fm_host_chain(M, audio, np.array([s.size for s in sigs], np.uint32), Iq.fm_sigma(M, cnr_db))
    assert host["nout"] == (n - Iq.NTAPS) // Iq.D_FM + 1 and n <= 40000
    ocfg = O.oracle_config("1200")
    for k in range(3):
        assert O.oracle_rx_stream(ocfg, host["audio"][k, :host["nout"]])["bytes"] == words[k].tobytes(), k
