"""Live comparison of the restatement with the reference built from its own
sources (oracle/_ref) on the reference's OWN test inputs (its tests/testdata-*
payloads, stored as tests/golden/refdata.npz).  Runs where oracle/_ref was built;
the committed goldens (test_oracle_golden.py) cover the same ground elsewhere."""
import os

import numpy as np
import pytest

import _golden as G
import _oracle as O
import _shapes as S

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="needs oracle/_ref (the reference built from its sources)")
REFDATA = np.load(os.path.join(G.GOLDEN_DIR, "refdata.npz"))


def ref_payload(name):
    """the reference's test input file `name` (e.g. testdata-ascii.txt), as bytes"""
    return REFDATA[name.replace("-", "_").replace(".", "_")].tobytes()


P24 = "--samplerate 24000 -M 1200 -S 2400"
K24 = dict(sample_rate=24000, mark_f=1200, space_f=2400)
# (reference test, payload file, tx args, rx args, config kwargs, expect "perfect")
CASES = [
    ("01-self-test-1200", "testdata-ascii.txt", "1200", "1200", dict(baudmode="1200"), False),
    ("02-self-test-300", "testdata-ascii.txt", "300", "300", dict(baudmode="300"), False),
    ("05-self-test-12000", "testdata-ascii.txt", "12000", "12000", dict(baudmode="12000"), False),
    ("06-float-samples", "testdata-ascii.txt", "12000 --float-samples", "12000",
     dict(baudmode="12000"), False),
    ("07-no-lut", "testdata-ascii.txt", "1200 --lut=0", "1200", dict(baudmode="1200"), False),
    ("08-lut16", "testdata-ascii.txt", "1200 --lut=16", "1200", dict(baudmode="1200"), False),
    ("09-lut16-float", "testdata-ascii.txt", "1200 --lut=16 --float-samples", "1200",
     dict(baudmode="1200"), False),
    ("10-verify-perfect", "testdata-ascii.txt", "1200 " + P24, "1200 " + P24,
     dict(baudmode="1200", **K24), True),
    ("11-perfect-nolut", "testdata-ascii.txt", "1200 --lut=0 " + P24, "1200 " + P24,
     dict(baudmode="1200", **K24), True),
    ("12-perfect-lut16", "testdata-ascii.txt", "1200 --lut=16 " + P24, "1200 " + P24,
     dict(baudmode="1200", **K24), True),
    ("13-perfect-nolut-float", "testdata-ascii.txt", "1200 --lut=0 --float-samples " + P24,
     "1200 " + P24, dict(baudmode="1200", **K24), True),
    ("14-perfect-lut16-float", "testdata-ascii.txt", "1200 --lut=16 --float-samples " + P24,
     "1200 " + P24, dict(baudmode="1200", **K24), True),
    ("15-perfect-float", "testdata-ascii.txt", "1200 --float-samples " + P24, "1200 " + P24,
     dict(baudmode="1200", **K24), True),
    ("21-rate-slop-292", "testdata-ascii.txt", "292", "300", dict(baudmode="300"), False),
    ("21-rate-slop-308", "testdata-ascii.txt", "308", "300", dict(baudmode="300"), False),
    ("30-amplitude-0.01", "testdata-ascii.txt", "--volume 0.01 1200", "1200",
     dict(baudmode="1200"), False),
    ("30-amplitude-E", "testdata-ascii.txt", "--volume E 1200", "1200",
     dict(baudmode="1200"), False),
    ("60-multibyte", "testdata-multibyte.txt", "1200", "1200", dict(baudmode="1200"), False),
    ("80-SAME", "testdata-ascii.txt", "same", "same", dict(baudmode="same"), False),
    ("81-ascii7", "testdata-ascii.txt", "1200 -7", "1200 -7",
     dict(baudmode="1200", n_data_bits=7), False),
    ("03-rtty", "testdata-baudot.txt", "rtty", "rtty", dict(baudmode="rtty"), False),
    ("81-tdd", "testdata-baudot.txt", "tdd", "tdd", dict(baudmode="tdd"), False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_reference_program(case, tmp_path):
    name, payload_file, tx, rx, kw, perfect = case
    payload = ref_payload(payload_file)
    wav = str(tmp_path / "x.wav")
    O.ref_tx(payload, tx.split(), wav)
    out, err = O.ref_rx(wav, rx.split())
    ref_lines = [l for l in err.splitlines() if l.startswith("### NOCARRIER")]
    assert ref_lines
    if perfect:
        assert "confidence=inf" in ref_lines[-1] and "(rate perfect)" in ref_lines[-1]
    sr, x = O.read_wav(wav)
    cfg = O.oracle_config(**kw)
    assert sr == cfg.sample_rate
    for ring in (True, False):
        r = O.oracle_rx_stream(cfg, x, ring_mode=ring)
        if cfg.decoder == 0:
            assert r["bytes"] == out
            if "-7" not in tx and "E" not in tx:
                assert out == payload
        assert [O.format_nocarrier(cfg, e) for e in r["episodes"]] == ref_lines


# bit lengths the kernels treat differently (tests/test_gpu_bitlengths.py sweeps 3 .. 320 against
# the restatement): the shortest, an odd one, a tail of 5 samples, Bell-103 tones a bin apart, one
# past the tile threshold -- at a whole number of samples per bit and at two fractional ones
ODD_BIT_LENGTHS = [(B, d) for B in (3, 7, 37, 121, 257) for d in (0.0, -0.3, 0.4) if (B, d) != (3, -0.3)]


@pytest.mark.parametrize("B,delta", ODD_BIT_LENGTHS, ids=["B%d%+g" % c for c in ODD_BIT_LENGTHS])
def test_restatement_equals_reference_program_at_odd_bit_lengths(B, delta, tmp_path):
    """baud = 48000 / (B + delta): the reference program transmits and receives at that rate, the
    restatement must derive the same bit length and print what the reference prints."""
    mode = repr(48000.0 / (B + delta))
    payload = ref_payload("testdata-ascii.txt")[:80]
    wav = str(tmp_path / "b.wav")
    O.ref_tx(payload, [mode], wav)
    out, err = O.ref_rx(wav, [mode])
    ref_lines = [l for l in err.splitlines() if l.startswith("### NOCARRIER")]
    sr, x = O.read_wav(wav)
    cfg = O.oracle_config(mode)
    assert sr == cfg.sample_rate == 48000 and cfg.bit_nsamples == B
    for ring in (True, False):
        r = O.oracle_rx_stream(cfg, x, ring_mode=ring)
        assert r["bytes"] == out
        assert [O.format_nocarrier(cfg, e) for e in r["episodes"]] == ref_lines
    # (the reference itself garbles bits of 3 samples, and of 7 at a fractional rate; at B = 121
    # its two tones are hardly a bin apart: there only the equality above says anything)
    assert ref_lines
    if B >= 37 and B != 121:
        assert payload in out


def test_dc_offset_sweep_tests_40_41(tmp_path):
    """--Xrxnoise adds a DC offset of -factor to every sample (rand()/RAND_MAX is
    an integer division, src/simpleaudio-sndfile.c:64-70); tests 40/41 sweep it."""
    payload = ref_payload("testdata-ascii.txt")
    for flags, kw in (("1200", dict(baudmode="1200")),
                      ("1200 " + P24, dict(baudmode="1200", **K24))):
        wav = str(tmp_path / "n.wav")
        O.ref_tx(payload, (flags + " --volume 0.5").split(), wav)
        sr, x = O.read_wav(wav)
        for noise in (0.0, 0.05, 0.10, 0.50):
            out, err = O.ref_rx(wav, (flags + " --Xrxnoise %g --rx-one" % noise).split())
            ref_lines = [l for l in err.splitlines() if l.startswith("### NOCARRIER")]
            cfg = O.oracle_config(rx_one=1, **kw)
            xn = x + np.float32((0.0 - 0.5) * (noise * 2)) if noise else x
            r = O.oracle_rx_stream(cfg, xn.astype(np.float32), ring_mode=False)
            assert r["bytes"] == out == payload
            assert [O.format_nocarrier(cfg, e) for e in r["episodes"]] == ref_lines


def test_find_frame_against_reference_fsk_c():
    """Call level: reference src/fsk.c (+FFT shim) vs restatement on random windows of
    noisy FSK; integers exact, magnitudes to float tolerance."""
    rng = np.random.default_rng(7)
    for mode in ("1200", "300", "same", "12000"):
        cfg = O.oracle_config(mode)
        payload = bytes(rng.integers(32, 127, size=40, dtype=np.uint8))
        import tempfile
        wav = O.tmp_wav()
        O.ref_tx(payload, [mode, "--float-samples"], wav)
        sr, x = O.read_wav(wav)
        os.unlink(wav)
        x = (x + rng.normal(0, 0.2, x.shape)).astype(np.float32)
        xp = np.concatenate([x, np.zeros(4 * int(cfg.expect_nsamples), np.float32)])
        rl, ol = O.ref_lib(), O.oracle_lib()
        rp = rl.fsk_plan_new(float(sr), cfg.mark_f, cfg.space_f, cfg.band_width)
        op = ol.ofsk_plan_new(float(sr), cfg.mark_f, cfg.space_f, cfg.band_width)
        assert (rp.contents.fftsize, rp.contents.b_mark, rp.contents.b_space) == \
               (op.contents.fftsize, op.contents.b_mark, op.contents.b_space)
        for off in rng.integers(0, len(x) - 1, size=200):
            for ci, step, lim, exp in ((0, cfg.try_step[0], cfg.search_limit, cfg.expect_sync),
                                       (1, cfg.try_step_fine[1], float("inf"), cfg.expect_data)):
                args = (xp[int(off):], int(cfg.expect_nsamples), int(cfg.try_first[ci]),
                        int(cfg.try_max[ci]), int(step), lim, exp)
                rc, rb, ra, rs = O.ref_find_frame(rp, *args)
                oc, ob, oa, os_ = O.oracle_find_frame(op, *args)
                assert (rb, rs) == (ob, os_)
                assert oc == pytest.approx(rc, rel=1e-5, abs=1e-6)
                assert oa == pytest.approx(ra, rel=1e-5, abs=1e-6)
        rl.fsk_plan_destroy(rp)
        ol.ofsk_plan_destroy(op)


# frame shapes the named modes do not have (tests/test_gpu_frameshapes.py sweeps 187 of them against
# the restatement): (shape, further options, the reference's command line for them)
_RAW = lambda n: (dict(binary_raw_nbits=n), {}, ["--binary-raw", str(n)])                               # noqa: E731


def _framed(d, s, p, opts=None, args=()):
    kw = dict(n_data_bits=d, nstartbits=s, nstopbits=float(p))
    return kw, dict(opts or {}), ["-%d" % d, "--startbits", str(s), "--stopbits", "%g" % p] + list(args)


REF_SHAPES = [_RAW(1), _RAW(9), _RAW(33), _RAW(64),
              _framed(5, 0, 0, dict(baudot=1)),                 # (-5 selects the Baudot decoder)
              _framed(7, 2, 1.5), _framed(8, 20, 2), _framed(8, 1, 0.5),
              _framed(8, 13, 1, dict(invert_start_stop=1), ["--invert-start-stop"]),
              _framed(7, 1, 1, dict(msb_first=1), ["--msb-first"])]


@pytest.mark.parametrize("rate", ["1200", "b300.4"])
@pytest.mark.parametrize("shape", REF_SHAPES, ids=[S.option_label(kw, o) if o else S.shape_label(kw) for kw, o, _a in REF_SHAPES])
def test_restatement_equals_reference_program_at_other_frame_shapes(shape, rate, tmp_path):
    """1 .. 64 bit windows a frame at 40 and 300 samples per bit: the sigma = 0.03 stream of
    _shapes.py's keyer as a float WAV through the reference program with --startbits / --stopbits /
    -5 -7 -8 / --binary-raw N.  The restatement's episodes must print the reference's NOCARRIER
    lines, its bytes must be the reference's stdout where the decoder is ASCII, and for the other
    decoders (--binary-raw's lines of 0 and 1, -5's Baudot) the product's host post-pass over the
    restatement's frames must print that stdout.

    Twice: the stream as keyed, in ring mode -- it ends with its last bit, and a frame that
    reaches past the end reads the reference's stale buffer cells, which is what ring mode is
    (at raw 1 and 300 samples per bit the last frame's confidence is 4.04 there and 5.21 over
    flat mode's zeros) -- and behind a buffer's length of silence, as the reference's own
    transmissions end, in ring and flat mode.

    --binary-raw 64: NOCARRIER lines only.  The reference's bit_window() shifts 1ULL by 64 for
    its mask, which C leaves undefined; the build under oracle/_ref prints 64 zeros a frame.
    The restatement and the product do what its `// handle bits==64` comment says."""
    import minimodem_amd as M
    kw, opts, args = shape
    ri = S.RATE_IDS.index(rate)
    mode = S.RATES[ri][1]
    allkw = dict(kw, **opts)
    cfg, mcfg = O.oracle_config(mode, **allkw), M.rx_config(mode, **allkw)
    keyed = S.make_streams(mcfg, [S.SEED, ri, 2000 + REF_SHAPES.index(shape)])[1][1]
    wav = str(tmp_path / "s.wav")
    for x, rings in ((keyed, (True,)), (np.concatenate([keyed, np.zeros(int(cfg.samplebuf_size), np.float32)]), (True, False))):
        O.write_wav(wav, x, int(cfg.sample_rate), s16=False)
        out, err = O.ref_rx(wav, [mode] + args)
        ref_lines = [l for l in err.splitlines() if l.startswith("### NOCARRIER")]
        assert ref_lines
        for ring in rings:
            r = O.oracle_rx_stream(cfg, x, ring_mode=ring)
            assert len(r["frames"]) >= 3
            assert [O.format_nocarrier(cfg, e) for e in r["episodes"]] == ref_lines
            if cfg.decoder == 0:
                assert r["bytes"] == out
            if kw.get("binary_raw_nbits") != 64:
                text, _err = M.stream_text(mcfg, r["frames"]["bits"], r["episodes"], quiet=True)
                assert text == out


# --confidence / --limit as the reference's command line takes them: (threshold, limit), None = not given
CONFIDENCE_OPTIONS = [(None, None), (0, None), (0, 0), (0.5, None), (1.5, 1.5), (None, 8), (None, "inf"), (4, None),
                      (4, 20), (12, None), (30, None), (3, 1)]
# (mode, payload file, bytes of it, sigma)
CONFIDENCE_MODES = [("1200", "testdata-ascii.txt", 40, 0.25), ("300", "testdata-ascii.txt", 24, 0.3),
                    ("rtty", "testdata-baudot.txt", 6, 0.35), ("12000", "testdata-ascii.txt", 40, 0.15),
                    ("same", "testdata-ascii.txt", 40, 0.3)]


@pytest.mark.parametrize("mode,payload_file,nbytes,sigma", CONFIDENCE_MODES, ids=[m[0] for m in CONFIDENCE_MODES])
def test_restatement_equals_reference_program_under_confidence_options(mode, payload_file, nbytes, sigma, tmp_path):
    """-c and -l drive every decision of the receive loop (minimodem.c:1265-1321,1357: a search ends
    at the first candidate that reaches the limit, a frame counts only above the threshold, the
    limit is lifted to the threshold); the GPU sweeps of tests/test_gpu_thresholds.py take the
    restatement's word for them.  Here the reference program transmits, seeded noise is added in
    front of, over and behind the signal, and it receives with twelve settings -- not given, 0, 0 / 0,
    0.5, 1.5 / 1.5, -l 8, -l inf, 4, 4 / 20, 12, 30, 3 / 1: the restatement with the same two values
    must print the reference's NOCARRIER lines, and its bytes where the decoder is ASCII, in ring
    and flat mode.  (Behind the noise the file ends with a buffer's length of silence, as in
    test_restatement_equals_reference_program_at_other_frame_shapes: with -c 0 the noise itself is
    decoded, and a frame that reaches past the end of a file reads the reference's stale buffer
    cells, which ring mode alone replicates -- 0.873 against flat mode's 0.874 in the last line
    at 1200 baud.)"""
    wav = str(tmp_path / "c.wav")
    O.ref_tx(ref_payload(payload_file)[:nbytes], [mode], wav)
    sr, x = O.read_wav(wav)
    rng = np.random.default_rng([95, CONFIDENCE_MODES.index((mode, payload_file, nbytes, sigma))])
    x = np.concatenate([np.zeros(4000), x.astype(np.float64), np.zeros(4000)])
    x = np.concatenate([x + rng.normal(0, sigma, x.shape), np.zeros(int(O.oracle_config(mode).samplebuf_size))])
    O.write_wav(wav, np.clip(np.rint(x * 32768), -32768, 32767).astype("<i2"), sr, True)
    sr, x = O.read_wav(wav)
    outcomes = set()
    for thr, lim in CONFIDENCE_OPTIONS:
        args, kw = [], {}
        if thr is not None:
            args += ["-c", str(thr)]
            kw["confidence_threshold"] = float(thr)
        if lim is not None:
            args += ["-l", str(lim)]
            kw["search_limit"] = float(lim)
        out, err = O.ref_rx(wav, args + [mode])
        ref_lines = [l for l in err.splitlines() if l.startswith("### NOCARRIER")]
        cfg = O.oracle_config(mode, **kw)
        assert sr == cfg.sample_rate
        for ring in (True, False):
            r = O.oracle_rx_stream(cfg, x, ring_mode=ring)
            assert [O.format_nocarrier(cfg, e) for e in r["episodes"]] == ref_lines, (mode, thr, lim, ring)
            if cfg.decoder == 0:
                assert r["bytes"] == out, (mode, thr, lim, ring)
        outcomes.add((out, tuple(ref_lines)))
    # (the settings do something -- frames out of the noise at 0, the default's, fewer or none at 30: the
    # reference itself prints at least three different things)
    assert len(outcomes) >= 3, len(outcomes)
