"""The frame shapes of tests/test_gpu_frameshapes.py: the list of shapes and rates, a numpy keyer
for frames the host transmitter cannot fill (it takes 8-bit words), and the five streams of a
configuration.  Plain helpers: the CPU and the GPU tests, tests/test_oracle_vs_reference.py and
tests/test_launch_plans.py share them."""
import numpy as np

# (id, baudmode, bit length at 48 kHz): each the smallest rate that reaches a kernel family
RATES = [
    ("1200", "1200", 40),                           # resident linear lattice
    ("b40.4", repr(48000.0 / 40.4), 40),            # 40 samples, nothing linear: direct lattice on both engines
    ("12000", "12000", 4),                          # generic linear, staging width 4 / 10
    ("240", "240", 200),                            # direct, then no lattice, then no SCAN slab
    ("b300.4", repr(48000.0 / 300.4), 300),         # the tile and the shared segments
    ("45.45", "45.45", 1056),                       # RTTY's windows
]
RATE_IDS = [r[0] for r in RATES]
NSTREAMS = 5
SEED = 3


def shape_label(kw):
    """'raw43' / '7-13-1.5' (data bits - start bits - stop bits)"""
    if "binary_raw_nbits" in kw:
        return "raw%d" % kw["binary_raw_nbits"]
    return "%d-%d-%g" % (kw["n_data_bits"], kw["nstartbits"], kw["nstopbits"])


def shape_n_bits(kw):
    """expect_n_bits of a shape: the data bits, the start bits and -- with stop bits of any length --
    the previous frame's stop bit and this one's"""
    if "binary_raw_nbits" in kw:
        return kw["binary_raw_nbits"]
    return kw["n_data_bits"] + kw["nstartbits"] + (2 if kw["nstopbits"] else 0)


RAW = [dict(binary_raw_nbits=n) for n in range(1, 65)]
# (without start bits the oracle itself locks on fewer than three frames of 3 stop bits at four of the rates)
FRAMED = [dict(n_data_bits=d, nstartbits=s, nstopbits=float(p))
          for d in (5, 7, 8) for s in (0, 1, 2, 3, 7, 13, 20) for p in (0, 0.5, 1, 1.5, 2, 3)
          if not (s == 0 and p == 3)]
SHAPES = RAW + FRAMED
assert len(RAW) == 64 and len(FRAMED) == 123 and len(SHAPES) == 187
GROUP = 16
GROUPS = [("raw%d-%d" % (lo + 1, lo + GROUP), RAW[lo: lo + GROUP]) for lo in range(0, 64, GROUP)] + \
         [("framed%d" % (lo // GROUP), FRAMED[lo: lo + GROUP]) for lo in range(0, len(FRAMED), GROUP)]
GROUP_IDS = [g[0] for g in GROUPS]


def key_fsk(cfg, segments, amplitude=0.8, leading_silence=0):
    """Phase-continuous FSK on cfg.mark_f (bit 1) / cfg.space_f (bit 0) from [(bit, samples as a
    float)], computed in float64: sample n carries the bit whose span holds n."""
    edges = np.cumsum(np.array([d for _b, d in segments], np.float64))
    tone = np.where(np.array([b for b, _d in segments], bool), float(cfg.mark_f), float(cfg.space_f))
    n = int(edges[-1])
    which = np.minimum(np.searchsorted(edges, np.arange(n, dtype=np.float64), side="right"), len(tone) - 1)
    phase = 2.0 * np.pi * np.cumsum(tone[which]) / float(cfg.sample_rate)
    return np.concatenate([np.zeros(leading_silence), amplitude * np.sin(phase)]).astype(np.float32)


def frame_segments(cfg, words, lead_bits=12, tail_bits=4):
    """idle, then one frame per word -- start bits, the word's n_data_bits low bits in the order
    they are sent (bit 0 first), one stop element of nstopbits bit times where the shape has
    any -- then idle.  Idle and stop are mark and start is space, or the other way round with
    --invert-start-stop."""
    spb = float(cfg.sample_rate) / float(cfg.data_rate)
    stop, start = (0, 1) if cfg.invert_start_stop else (1, 0)
    segs = [(stop, spb)] * lead_bits
    for w in words:
        segs += [(start, spb)] * int(cfg.nstartbits)
        segs += [((int(w) >> i) & 1, spb) for i in range(int(cfg.n_data_bits))]
        if cfg.nstopbits:
            segs.append((stop, spb * float(cfg.nstopbits)))
    return segs + [(stop, spb)] * tail_bits


def random_words(rng, cfg, n):
    nd = int(cfg.n_data_bits)
    return [int.from_bytes(rng.bytes(8), "little") & ((1 << nd) - 1) for _ in range(n)]


def make_streams(cfg, seed, sync_frames=0):
    """-> (words sent, the five streams of one configuration): clean, sigma 0.03, sigma 0.2
    (refinements and rescans), clean and cut B // 3 samples short, noise only.  Each keyed stream
    is max(4, 160 // expect_n_bits) frames of random data bits behind 12 idle bits (and behind
    `sync_frames` frames of the sync byte), 0 .. 200 samples of silence in front."""
    rng = np.random.default_rng(seed)
    nframes = max(4, 160 // int(cfg.expect_n_bits))
    words = [int(cfg.sync_byte)] * sync_frames + random_words(rng, cfg, nframes)
    segs = frame_segments(cfg, words)
    streams = []
    for sigma in (0.0, 0.03, 0.2, 0.0):
        x = key_fsk(cfg, segs, leading_silence=int(rng.integers(0, 201)))
        if sigma:
            x = (x + rng.normal(0, sigma, x.shape)).astype(np.float32)
        streams.append(x)
    streams[3] = streams[3][: len(streams[3]) - int(cfg.bit_nsamples) // 3]
    streams.append(rng.normal(0, 0.3, 6 * int(cfg.expect_nsamples)).astype(np.float32))
    return words, streams


def configs(rate, shapes=None):
    """[(label, baudmode, shape kwargs, seed)] of a rate's configurations"""
    ri = RATE_IDS.index(rate)
    mode = RATES[ri][1]
    return [("%s/%s" % (rate, shape_label(kw)), mode, kw, [SEED, ri, SHAPES.index(kw)])
            for kw in (SHAPES if shapes is None else shapes)]


# The options leg, at every rate of at least 40 samples per bit: (shape, options, sync frames sent first)
OPTION_RATES = [r for r, _mode, B in RATES if B >= 40]
_R = lambda n: dict(binary_raw_nbits=n)                                             # noqa: E731
_F = lambda d, s, p: dict(n_data_bits=d, nstartbits=s, nstopbits=float(p))          # noqa: E731
OPTIONS = [(_R(n), dict(msb_first=1), 0) for n in (1, 8, 31, 32, 33, 40, 64)] + [
    (_F(7, 1, 1), dict(msb_first=1), 0),
    (_F(8, 1, 1), dict(invert_start_stop=1), 0),
    (_F(5, 2, 1.5), dict(invert_start_stop=1), 0),
    (_F(8, 20, 2), dict(invert_start_stop=1), 0),
    (_R(8), dict(sync_byte=0xAB), 16),              # SAME's shape
    (_F(8, 1, 1), dict(sync_byte=0x16), 16),
    (_R(40), dict(sync_byte=0xAB54A98CEB), 16),     # above 2^32
    (_F(8, 1, 1), dict(inverted_freqs=1), 0),
]


def option_label(kw, opts):
    return shape_label(kw) + "+" + ",".join("%s=%s" % (k, hex(v) if k == "sync_byte" else v) for k, v in opts.items())


OPTION_IDS = [option_label(kw, o) for kw, o, _s in OPTIONS]
# (added to the option's index in the seed.  Nothing marks where a raw frame begins, and after a lock on the
# sync pattern the reference's fine search may settle a whole bit off: with most seeds the oracle then finds
# no sync frame in one or two of the raw streams.  Taken for the oracle's counts of sync frames alone.)
OPTION_SEED = 1000
