"""The transmitter's command lines of tests/golden/tx_shapes.json: what the sweep is
(tests/golden/make_tx_shapes.py records it from the reference program), and how a command line
of `minimodem --tx` turns into rx_config() / synthesize() arguments (tests/test_tx_shapes.py
replays it through the host transmitter)."""
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx_shapes.json")

SAMPLE_RATES = (48000, 44100, 11025, 8000)
RATES = ("110", "300", "1171", "1200", "45.45", "47", "3000", "9600", "12000", "16000", "24000")
START_STOP = ((1, 1.0), (0, 0.0), (2, 1.0), (1, 0.5), (1, 1.5), (3, 3.0), (1, 0.0), (0, 2.0), (20, 1.0))
# (table, sample format, volume)
TONES = (("--lut=4096", ""), ("--lut=1000", "--float-samples"), ("--lut=17 --volume 0.3", ""),
         ("--lut=0", "--float-samples"))
# (the last: the sync frames go out LSB first whatever --msb-first says, minimodem.c:218-221)
OPTIONS = ("--msb-first", "--invert-start-stop", "--inverted", "--sync-byte 0x16", "-7",
           "--msb-first --sync-byte 0x16")
# B = 1025, 1024, 1023, 1020 (both sides of the device's quotient table), 2 and 1
EDGES = ("46.83", "46.875", "46.92", "47.06", "-M 12000 -S 6000 24000", "-M 12000 -S 6000 48000")
B_MUST_OCCUR = (1, 2, 3, 5, 7, 37, 40, 41, 1020, 1023, 1024, 1025, 1056)

# 64 bytes: 0x00, 0xFF, every bit position alone and alone missing, runs, text
PAYLOAD = bytes([0x00, 0xFF] + [1 << k for k in range(8)] + [0xFF ^ (1 << k) for k in range(8)]
                + [0x55, 0xAA, 0x00, 0x00, 0xFF, 0xFF, 0x0F, 0xF0, 0x33, 0xCC, 0x7F, 0x80, 0x16, 0x7E]) \
    + b"The quick brown fox, 0123456789\n"
assert len(PAYLOAD) == 64
# Baudot lines go through the command-line program (characters -> 5-bit codes): letters,
# figures, both shifts several times
BAUDOT_TEXT = b"RYRYRY THE QUICK BROWN FOX 0123456789 JUMPS -$!&#'()\"/:;?,. OVER 73 DE MI355X\r\n"
BAUDOT_LINES = ("rtty --stopbits 1", "rtty --startbits 2 --stopbits 2", "rtty -R 44100 --float-samples",
                "tdd --stopbits 1.5 -R 8000", "tdd --startbits 3 --stopbits 3 --lut=1000")


def _fmt(v):
    return ("%g" % v)


def sweep_lines():
    """Every ASCII command line of the fixture, as strings (before the refused ones are dropped)."""
    lines = []
    for sr in SAMPLE_RATES:
        for rate in RATES:
            for nstart, nstop in START_STOP:
                for tone, fmt in TONES:
                    lines.append(" ".join(w for w in ("-R %d" % sr, "--startbits %d" % nstart,
                                                      "--stopbits %s" % _fmt(nstop), tone, fmt, rate) if w))
    for sr in (48000, 44100):
        for rate in ("1200", "1171"):
            for opt in OPTIONS:
                for tone, fmt in TONES:
                    lines.append(" ".join(w for w in ("-R %d" % sr, opt, tone, fmt, rate) if w))
    for edge in EDGES:
        lines.append("-R 48000 --lut=1000 --float-samples " + edge)
    return lines


def parse(line):
    """A transmit command line -> (rx_config keyword arguments, synthesize() keyword arguments)."""
    cfg, syn = {}, {"s16": True}
    words = line.split()
    i = 0
    mode = None

    def value():
        nonlocal i
        i += 1
        return words[i]
    while i < len(words):
        w = words[i]
        if w == "-R":
            cfg["sample_rate"] = int(value())
        elif w == "--startbits":
            cfg["nstartbits"] = int(value())
        elif w == "--stopbits":
            cfg["nstopbits"] = float(value())
        elif w == "-M":
            cfg["mark_f"] = float(value())
        elif w == "-S":
            cfg["space_f"] = float(value())
        elif w == "--volume":
            syn["amplitude"] = float(value())
        elif w.startswith("--lut="):
            syn["lut"] = int(w[6:])
        elif w == "--float-samples":
            syn["s16"] = False
        elif w == "--msb-first":
            cfg["msb_first"] = 1
        elif w == "--invert-start-stop":
            cfg["invert_start_stop"] = 1
        elif w == "--inverted":
            cfg["inverted_freqs"] = 1
        elif w == "--sync-byte":
            cfg["sync_byte"] = int(value(), 0)
        elif w == "-7":
            cfg["n_data_bits"] = 7
        elif mode is None and not w.startswith("-"):
            mode = w
        else:
            raise ValueError("unknown transmit option %r" % w)
        i += 1
    cfg["baudmode"] = mode
    return cfg, syn


def bit_nsamples(cfg):
    """minimodem.c:131-132, in float as the C does it"""
    return int(np.float32(np.float32(cfg.sample_rate) / np.float32(cfg.data_rate)) + np.float32(0.5))


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, "<f4").tobytes()).hexdigest()


def load():
    with open(FIXTURE) as f:
        return json.load(f)
