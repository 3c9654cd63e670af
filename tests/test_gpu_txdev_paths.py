"""Every path of the device transmitter (tx_synth_kernel, csrc/mifsk_txdev.hip) against the host
transmitter (csrc/mifsk_tx.cpp, which tests/test_tx_shapes.py pins to the reference program at
the same bit lengths, frame shapes and tables), bit for bit and sample count included.

The kernel takes one path per axis; `paths()` below restates the rules, and
test_the_cases_reach_every_path (CPU) asserts that the cases reach all 22 combinations and
prints the table of tests/README.md.  The cases are the smallest that reach a path: B (samples
per bit) 1 and 2, 3 / 5 / 7 / 37 / 41 (no multiple of 4), 4 and 40 (vector stores), both sides
of the quotient table's 1024 samples, 1056, and 40 with start and stop tones of other lengths."""
import ctypes as C

import numpy as np
import pytest

import minimodem_amd as M
from minimodem_amd import _lib

gpu = pytest.mark.gpu

# csrc/mifsk_txdev.hip: TX_BLOCK (tones per chunk, two chunks in LDS) and TX_QUOT (longest bit
# with a quotient table), and the rules of tx_synth_kernel this restates:
#   uniform  = no start tone or as long as a bit, no stop tone or as long as a bit, B > 1
#   quot     = uniform and B <= TX_QUOT
#   vec4     = quot and a table and B % 4 == 0
#   pow2     = a table whose length is a power of two
# (tone and phase: `uniform`, `quot`, `vec4` above the chunk loop; sine: `pow2` / `table_len`
# in both sample loops; format: `as_s16`; tone lengths: mifsk_tx_synthesize_batch)
TX_BLOCK, TX_QUOT = 256, 1024


def tone_lengths(cfg):
    """(bit, start, stop) tone lengths in samples, in the transmitters' float arithmetic"""
    f32 = np.float32
    b = int(f32(f32(cfg.sample_rate) / f32(cfg.data_rate)) + f32(0.5))
    start = int(f32(b) * f32(cfg.nstartbits)) if cfg.nstartbits > 0 else 0
    stop = int(f32(b) * f32(cfg.nstopbits)) if cfg.nstopbits > 0 else 0
    return b, start, stop


def paths(cfg, lut, s16):
    """(tone, phase, sine, format) of tx_synth_kernel for a configuration and its options"""
    b, start, stop = tone_lengths(cfg)
    uniform = (not start or start == b) and (not stop or stop == b) and b > 1
    quot = uniform and b <= TX_QUOT
    vec4 = quot and lut and b % 4 == 0
    return ("magic" if uniform else "bsearch",
            "vec4" if vec4 else "quot" if quot else "div",
            "sinf" if not lut else "mod" if lut & (lut - 1) else "mask",
            "s16" if s16 else "f32")


ALL_PATHS = {(t, p, s, f)
             for t, p in (("magic", "vec4"), ("magic", "quot"), ("magic", "div"), ("bsearch", "div"))
             for s in ("mask", "mod", "sinf") if not (p == "vec4" and s == "sinf")
             for f in ("f32", "s16")}
assert len(ALL_PATHS) == 22

TONES_12K = dict(mark_f=12000.0, space_f=6000.0)     # tones that rx_config takes at B = 1 and 2
# name -> (baudmode, modem options, samples per bit)
CASES = {
    "B1": ("48000", TONES_12K, 1), "B2": ("24000", TONES_12K, 2), "B3": ("16000", {}, 3),
    "B4": ("12000", {}, 4), "B5": ("9600", {}, 5), "B7_8k": ("1171", dict(sample_rate=8000), 7),
    "B37_44k1": ("1200", dict(sample_rate=44100), 37), "B40": ("1200", {}, 40), "B41": ("1171", {}, 41),
    "B1020": ("47.06", {}, 1020), "B1023": ("46.92", {}, 1023), "B1024": ("46.875", {}, 1024),
    "B1025": ("46.83", {}, 1025), "B1056_uniform": ("45.45", dict(nstopbits=1.0), 1056),
}
# tones of three lengths in one chunk
for _a in (2, 3, 20):
    for _o in (0.5, 3.0):
        CASES["B40_start%d_stop%g" % (_a, _o)] = ("1200", dict(nstartbits=_a, nstopbits=_o), 40)
# the options, off the vector path: the quotient table and the division
for _m, _b in (("1171", 41), ("46.83", 1025)):
    CASES["B%d_msb" % _b] = (_m, dict(msb_first=1), _b)
    CASES["B%d_invss" % _b] = (_m, dict(invert_start_stop=1), _b)
    CASES["B%d_invfreq" % _b] = (_m, dict(inverted_freqs=1), _b)
    CASES["B%d_sync" % _b] = (_m, dict(sync_byte=0x16), _b)
    # (the sync frames go out LSB first whatever --msb-first says: minimodem.c:218-221)
    CASES["B%d_sync_msb" % _b] = (_m, dict(sync_byte=0x16, msb_first=1), _b)
# words drawn from 0 ... 255 (as in every case here) where only 5 / 7 bits of them are sent
CASES["B41_5bit"] = ("1171", dict(n_data_bits=5), 41)
CASES["B41_7bit"] = ("1171", dict(n_data_bits=7), 41)
CASES["B41_7bit_msb"] = ("1171", dict(n_data_bits=7, msb_first=1), 41)
LUTS = (4096, 1000, 17, 3, 0)
AMPS = (1.0, 0.37, 1.7)


def case_cfg(name):
    mode, kw, b = CASES[name]
    cfg = M.rx_config(mode, **kw)
    assert tone_lengths(cfg)[0] == b, (name, tone_lengths(cfg))
    return cfg


def test_the_cases_reach_every_path():
    """all 22 combinations of (tone, phase, sine, format), and which B reach each"""
    reached = {}
    for name in CASES:
        cfg = case_cfg(name)
        for lut in LUTS:
            for s16 in (False, True):
                reached.setdefault(paths(cfg, lut, s16), set()).add(name)
    print("| tone | phase | sine | format | cases |\n|---|---|---|---|---|")
    for p in sorted(ALL_PATHS):
        print("| %s | %s | %s | %s | %s |" % (p + (", ".join(sorted(reached.get(p, ()), key=list(CASES).index)),)))
    assert set(reached) == ALL_PATHS, ALL_PATHS ^ set(reached)
    # the edges that the rules turn on
    assert paths(case_cfg("B1"), 4096, False)[:2] == ("bsearch", "div")
    assert paths(case_cfg("B2"), 4096, False)[:2] == ("magic", "quot")
    assert paths(case_cfg("B1024"), 1000, False)[:2] == ("magic", "vec4")
    assert paths(case_cfg("B1023"), 1000, False)[:2] == ("magic", "quot")
    assert paths(case_cfg("B1025"), 1000, False)[:2] == ("magic", "div")
    assert paths(case_cfg("B1056_uniform"), 1000, False)[:2] == ("magic", "div")
    # tones of three lengths in one chunk (3 start and 3 stop bits: two, both other than a bit's)
    three = [name for name in CASES if len(set(tone_lengths(case_cfg(name)))) == 3]
    assert three == [name for name in CASES if "_start" in name and name != "B40_start3_stop3"], three


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU: the device transmitter has no CPU fallback")
    return torch, M.Context(0)


def check_batch(torch, ctx, cfg, words, nwords, lead, lut, amp, s16, d_words=None):
    """the device's rows == the host transmitter's streams, lengths included, zeros behind"""
    if d_words is None:
        d_words = torch.from_numpy(words).cuda()
    x, n = M.synthesize_batch(ctx, cfg, d_words, nwords=torch.from_numpy(nwords).cuda(), lut=lut,
                              amplitude=amp, leading_silence=torch.from_numpy(lead).cuda(), s16=s16)
    x, n = x.cpu().numpy(), n.cpu().numpy()
    for i in range(words.shape[0]):
        ref = M.synthesize(cfg, words[i, :nwords[i]], lut=lut, amplitude=amp,
                           leading_silence=int(lead[i]), s16=s16)
        assert int(n[i]) == ref.shape[0], (i, lut, amp)
        if x[i, :n[i]].tobytes() != ref.tobytes():
            d = np.flatnonzero(x[i, :n[i]].view(np.uint32) != ref.view(np.uint32))
            pytest.fail("stream %d lut %d amplitude %g: %d samples differ, the first at %d of %d" %
                        (i, lut, amp, d.size, d[0], n[i]))
        assert not x[i, n[i]:].any()
    return x, n


def ragged(b):
    """the 9-stream batch of test_gpu_txdev.py; from B = 1020 on at most 40 words a stream,
    which is still more than one chunk of tones (404)"""
    maxw = 300 if b < 1020 else 40
    words = np.random.default_rng(11).integers(0, 256, size=(9, maxw), dtype=np.uint8)
    nwords = np.minimum(np.array([maxw, 1, 0, 17, 255, 256, 257, 64, 299]), maxw).astype(np.int32)
    lead = np.array([0, 5, 100, 0, 3333, 1, 40, 41, 7], np.int32)
    return words, nwords, lead


@gpu
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("lut", LUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_tx_equals_host_generator_on_every_path(dev, name, lut, s16):
    torch, ctx = dev
    cfg = case_cfg(name)
    words, nwords, lead = ragged(CASES[name][2])
    d_words = torch.from_numpy(words).cuda()
    for amp in AMPS:
        check_batch(torch, ctx, cfg, words, nwords, lead, lut, amp, s16, d_words)


# streams that end exactly at, one before and one behind a chunk of TX_BLOCK tones, and at the
# second chunk's end (where the double buffer wraps): name -> (mode, options, tones of a
# stream of n words, words per stream)
EDGE_CASES = {
    "B3_1bit": ("16000", dict(n_data_bits=1, nstartbits=0, nstopbits=0.0), lambda n: n + 2,
                (253, 254, 255, 256, 510, 511, 3000)),
    "B40_1bit": ("1200", dict(n_data_bits=1, nstartbits=0, nstopbits=0.0), lambda n: n + 2,
                 (253, 254, 255, 256, 510, 511, 3000)),
    "B40_8N0": ("1200", dict(nstartbits=1, nstopbits=0.0), lambda n: 4 + 9 * n, (28, 56, 29, 57)),
}


def test_the_chunk_edge_cases_end_on_chunk_edges():
    tones = {name: {f(n) for n in ns} for name, (_m, _kw, f, ns) in EDGE_CASES.items()}
    for name in ("B3_1bit", "B40_1bit"):
        assert tones[name] >= {TX_BLOCK - 1, TX_BLOCK, TX_BLOCK + 1, 2 * TX_BLOCK, 2 * TX_BLOCK + 1}
    assert TX_BLOCK in tones["B40_8N0"]
    for name, (mode, kw, _f, _ns) in EDGE_CASES.items():
        M.rx_config(mode, **kw)


@gpu
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_device_tx_streams_that_end_on_chunk_edges(dev, name, s16):
    torch, ctx = dev
    mode, kw, ntones, ns = EDGE_CASES[name]
    cfg = M.rx_config(mode, **kw)
    nwords = np.array(ns, np.int32)
    words = np.random.default_rng(12).integers(0, 256, size=(len(ns), int(nwords.max())), dtype=np.uint8)
    lead = (np.arange(len(ns)) * 3).astype(np.int32)
    for lut in (4096, 1000, 0):
        _x, n = check_batch(torch, ctx, cfg, words, nwords, lead, lut, 1.0, s16)
        b = tone_lengths(cfg)[0]
        assert [int(v) for v in n] == [int(lead[i]) + b * ntones(int(nwords[i])) for i in range(len(ns))]


@gpu
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("name", ["B3", "B40", "B41", "B40_start2_stop0.5"])
def test_device_tx_reads_a_row_strided_words_view(dev, name, s16):
    """words = big[:, :k]: rows 512 bytes apart, and what lies between them is not read"""
    torch, ctx = dev
    cfg = case_cfg(name)
    words, nwords, lead = ragged(CASES[name][2])
    big = np.random.default_rng(13).integers(0, 256, size=(9, 512), dtype=np.uint8)
    big[:, :words.shape[1]] = words
    view = torch.from_numpy(big).cuda()[:, :words.shape[1]]
    assert view.stride(0) == 512 and not view.is_contiguous()
    for lut in (4096, 17):
        a, na = check_batch(torch, ctx, cfg, words, nwords, lead, lut, 1.0, s16, view)
        b, nb = check_batch(torch, ctx, cfg, words, nwords, lead, lut, 1.0, s16, view.contiguous())
        assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes()


# ---- rows that are cut: mifsk_tx_synthesize_batch through ctypes, as the other GPU tests call
# the ABI, into a buffer of nstreams * stride + 64 floats filled with a NaN pattern
PATTERN = 0x7FC0BEEF     # a quiet NaN, as int32
NCUT, CUT_WORDS, GUARD = 4, 30, 64      # 4 rows: with an odd stride they start at all four alignments
CUT_CASES = {"vec4_B40": "B40", "quot_B41": "B41", "div_B1056": "B1056_uniform",
             "bsearch_stop2": ("1200", dict(nstopbits=2.0))}


def chunk_end(cfg, nwords):
    """samples of the first TX_BLOCK tones of a stream of nwords words (no sync frames)"""
    b, start, stop = tone_lengths(cfg)
    tones = [b] * (2 if cfg.nstartbits else 0)
    for _ in range(nwords):
        tones += ([start] if start else []) + [b] * int(cfg.n_data_bits) + ([stop] if stop else [])
    tones += [b, b]
    assert len(tones) > TX_BLOCK
    return sum(tones[:TX_BLOCK])


@gpu
@pytest.mark.parametrize("lead", [0, 3])
@pytest.mark.parametrize("name", list(CUT_CASES))
def test_device_tx_cut_rows_are_prefixes_and_nothing_is_written_behind(dev, name, lead):
    torch, ctx = dev
    lib = _lib.load()
    c = CUT_CASES[name]
    cfg = case_cfg(c) if isinstance(c, str) else M.rx_config(c[0], **c[1])
    if name == "bsearch_stop2":
        assert paths(cfg, 4096, False)[:2] == ("bsearch", "div")
    else:
        assert paths(cfg, 4096, False)[1] == name.split("_")[0]
    words = np.random.default_rng(14).integers(0, 256, size=(NCUT, CUT_WORDS), dtype=np.uint8)
    d_words = torch.from_numpy(words).cuda()
    d_n = torch.zeros(NCUT, dtype=torch.int32, device="cuda")
    b = tone_lengths(cfg)[0]
    end0 = lead + chunk_end(cfg, CUT_WORDS)
    mid = lead + 4 * (128 * b // 4)                 # lead + 4k, in the middle of the first chunk
    for lut, s16 in ((4096, False), (1000, True)):
        refs = [M.synthesize(cfg, words[i], lut=lut, leading_silence=lead, s16=s16) for i in range(NCUT)]
        full = refs[0].shape[0]
        assert all(r.shape[0] == full for r in refs) and mid + 3 < end0 < full - 1
        strides = [mid, mid + 1, mid + 2, mid + 3, end0, end0 + 1, full - 1, full, full + 5]
        if lead:
            strides = [lead - 1] + strides
        assert any(s % 2 for s in strides)
        for stride in strides:
            out = torch.full((NCUT * stride + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
            d_n.zero_()
            rc = lib.mifsk_tx_synthesize_batch(
                ctx.handle, C.byref(cfg), C.c_void_p(d_words.data_ptr()), CUT_WORDS, None, CUT_WORDS, NCUT,
                lut, C.c_float(1.0), None, lead, 1 if s16 else 0, C.c_void_p(out.data_ptr()), stride,
                C.c_void_p(d_n.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            got = out.cpu().numpy()
            assert d_n.cpu().numpy().tolist() == [full] * NCUT, stride      # the stream's length, cut or not
            assert (got[NCUT * stride:] == PATTERN).all(), stride       # nothing behind the last row
            for i in range(NCUT):
                want = np.zeros(stride, np.float32)
                m = min(stride, full)
                want[:m] = refs[i][:m]
                row = got[i * stride:(i + 1) * stride]
                if row.tobytes() != want.tobytes():
                    d = np.flatnonzero(row.view(np.uint32) != want.view(np.uint32))
                    pytest.fail("row %d of stride %d (lut %d): %d samples differ, the first at %d" %
                                (i, stride, lut, d.size, d[0]))
