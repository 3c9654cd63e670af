"""The host transmitter (csrc/mifsk_tx.cpp) against the reference program's transmitter at every
sample rate, bit length, start / stop shape, table length and sample format of
tests/golden/tx_shapes.json (recorded by tests/golden/make_tx_shapes.py from
oracle/_ref/minimodem_ref: sample count and SHA-256 per command line) -- it is what the device
transmitter is compared with (tests/test_gpu_txdev*.py) and what makes the input of the receive
tests.  Where oracle/_ref exists the same command lines run live on another payload."""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _txshapes as T
import minimodem_amd as M

CLI = os.path.join(O.REF_DIR, "minimodem_mifsk_batch")
FIX = T.load()
RECORDS = FIX["records"]
PAYLOAD = bytes.fromhex(FIX["payload"])
NGROUPS = 16


def synth(line, payload):
    cfg_kw, syn = T.parse(line)
    cfg = M.rx_config(**cfg_kw)
    return cfg, M.synthesize(cfg, payload, **syn)


def test_the_fixture_is_the_sweep():
    """the file holds the command lines of _txshapes.sweep_lines() that rx_config accepts, in
    order, on the payload of _txshapes: nothing was dropped from it by hand"""
    assert PAYLOAD == T.PAYLOAD and FIX["baudot_text"].encode() == T.BAUDOT_TEXT
    assert 0x00 in PAYLOAD and 0xFF in PAYLOAD
    assert all(any(b >> k & 1 for b in PAYLOAD) and any(not b >> k & 1 for b in PAYLOAD) for k in range(8))
    want = []
    for line in T.sweep_lines():
        try:
            M.rx_config(**T.parse(line)[0])
        except ValueError:
            continue
        want.append(line)
    assert [r["args"] for r in RECORDS] == want
    assert [r["args"] for r in FIX["baudot_records"]] == list(T.BAUDOT_LINES)


def test_the_fixture_covers_the_transmitter():
    rates, shapes, bits, tables = set(), set(), set(), set()
    for r in RECORDS:
        cfg_kw, syn = T.parse(r["args"])
        cfg = M.rx_config(**cfg_kw)
        rates.add(int(cfg.sample_rate))
        shapes.add((int(cfg.nstartbits), float(cfg.nstopbits)))
        bits.add(T.bit_nsamples(cfg))
        tables.add(syn.get("lut", 4096))
    assert rates == set(T.SAMPLE_RATES)
    assert shapes >= set(T.START_STOP)
    assert bits >= set(T.B_MUST_OCCUR), sorted(set(T.B_MUST_OCCUR) - bits)
    assert 0 in tables and any(n & (n - 1) for n in tables if n), tables


@pytest.mark.parametrize("group", range(NGROUPS))
def test_host_transmitter_equals_recorded_reference(group):
    bad = []
    for r in RECORDS[group::NGROUPS]:
        _cfg, x = synth(r["args"], PAYLOAD)
        if x.shape[0] != r["n"] or T.digest(x) != r["sha256"]:
            bad.append((r["args"], x.shape[0], r["n"]))
    if bad and O.have_ref():
        # where the reference is at hand: the first sample that differs
        for line, _n, _m in bad[:5]:
            wav = O.tmp_wav()
            try:
                O.ref_tx(PAYLOAD, line.split(), wav)
                _sr, ref = O.read_wav(wav)
            finally:
                os.unlink(wav)
            x = synth(line, PAYLOAD)[1]
            m = min(len(x), len(ref))
            d = np.flatnonzero(x[:m].view(np.uint32) != ref[:m].view(np.uint32))
            print("%s: %d samples, reference %d, first difference at %s" %
                  (line, len(x), len(ref), d[0] if d.size else "the end of the shorter one"))
    assert not bad, "%d of %d command lines differ from the recorded reference: %s" % (
        len(bad), len(RECORDS[group::NGROUPS]), bad[:5])


@pytest.mark.skipif(not O.have_ref(), reason="needs oracle/_ref")
def test_host_transmitter_equals_live_reference(tmp_path):
    """every command line again on a seeded payload that is not the recorded one"""
    payload = bytes(np.random.default_rng(20261019).integers(0, 256, size=48, dtype=np.uint8))
    assert payload != PAYLOAD
    wav = str(tmp_path / "ref.wav")
    bad = []
    for r in RECORDS:
        O.ref_tx(payload, r["args"].split(), wav)
        _sr, ref = O.read_wav(wav)
        x = synth(r["args"], payload)[1]
        if x.shape != ref.shape or x.tobytes() != ref.tobytes():
            m = min(len(x), len(ref))
            d = np.flatnonzero(x[:m].view(np.uint32) != ref[:m].view(np.uint32))
            bad.append((r["args"], len(x), len(ref), int(d[0]) if d.size else None))
    assert not bad, bad[:5]


@pytest.mark.skipif(not os.path.exists(CLI), reason="needs the batch command-line program (make -C oracle)")
@pytest.mark.parametrize("rec", FIX["baudot_records"], ids=[r["args"] for r in FIX["baudot_records"]])
def test_cli_baudot_framing_equals_recorded_reference(rec, tmp_path):
    """RTTY / TDD with --startbits / --stopbits / -R: characters -> 5-bit codes -> the host
    transmitter, through `minimodem_mifsk_batch --tx --file`, which accepts all three options"""
    wav = str(tmp_path / "mine.wav")
    r = subprocess.run([CLI, "--tx", "--file", wav] + rec["args"].split(), input=T.BAUDOT_TEXT,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    _sr, x = O.read_wav(wav)
    assert x.shape[0] == rec["n"]
    assert T.digest(x) == rec["sha256"]
