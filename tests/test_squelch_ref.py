"""The power squelch on the host (include/mifsk/squelch.h): the definition proved on the restatement
tools/squelch_ref.c alone -- the sample energy against exact integer and rational arithmetic, the saturation
rule, the gate against a ten-line machine in Python, pieces against the whole for every cut of a row, and what
the spans promise across calls."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _squelch as Sq
from _squelch import F32, FULL, STATE, same_bits


def model_energy(a, b):
    """the header's rule in exact arithmetic: every rounding a correctly rounded float() of a Fraction"""
    a, b = float(F32(a)), float(F32(b))
    if math.isnan(a) or math.isnan(b) or math.isinf(a) or math.isinf(b):
        return FULL
    bb = float(Fraction(b) ** 2)
    p = float(Fraction(a) ** 2 + Fraction(bb))
    if not p < 256.0:
        return FULL
    e = Fraction(p) * 2 ** 40
    lo = math.floor(e)
    return lo + (1 if e - lo > Fraction(1, 2) or (e - lo == Fraction(1, 2) and lo % 2) else 0)


def test_pcm16_energies_are_exact_integers():
    rng = np.random.default_rng(1)
    v = rng.integers(-32768, 32768, size=(4000, 2)).astype(np.int16)
    v[:6] = [(-32768, -32768), (32767, 32767), (0, 0), (-32768, 0), (1, 0), (0, -1)]
    want = [(int(i) ** 2 + int(q) ** 2) << 10 for i, q in v]
    assert Sq.ref_energies(v.astype(F32) / F32(32768.0)).tolist() == want
    assert max(want) == 1 << 41 and want[4] == 1 << 10
    # ... and through the rows' reader, one window per sample
    r = Sq.ref_squelch(v[None], None, 1, 1)
    assert r["nwindows"][0] == 4000 and r["energy"][0, :4000].tolist() == want and r["energy"][0, 4000] == Sq.FILL64


def test_float_energies_against_exact_arithmetic():
    rng = np.random.default_rng(2)
    iq = (rng.standard_normal((3000, 2)) * 10.0 ** rng.uniform(-8, 1.3, (3000, 1))).astype(F32)
    iq[:8] = [(1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (-0.0, 0.0), (2.0 ** -22, 0.0), (3 * 2.0 ** -22, 0.0), (1e-30, 1e-30),
              (np.uint32(5).view(F32), 1e-20)]
    got = Sq.ref_energies(iq).tolist()
    assert got == [model_energy(a, b) for a, b in iq]
    assert got[0] == got[1] == 1 << 40 and got[3] == 0 and got[6] == 0 and got[7] == 0
    assert got[4] == 0 and got[5] == 1               # 2^-44 2^40 = 0.0625 -> 0; 9 2^-44 2^40 = 0.5625 -> 1
    assert FULL in got and min(got) == 0


def test_the_saturation_rule():
    """On the power itself: p = 256 - ulp is the last one that is scaled, and rint((256 - 2^-45) 2^40) = rint(2^48 -
    2^-5) is 2^48 as well, so no energy is above full scale; p = 256, +Inf and NaN are full scale.  (Two float32
    scalars do not reach p = 256 - ulp: b^2 steps by more than an ulp of 256 wherever a^2 + b^2 gets there.)  A
    pair whose exact sum is below 256 and rounds up to it is found by search with exact arithmetic."""
    scale = Sq.ref_lib().squelch_ref_scale
    below = math.nextafter(256.0, 0.0)
    assert below == 256.0 - 2.0 ** -45 and scale(below) == FULL and scale(256.0) == FULL
    assert scale(255.5) == 511 << 39 and scale(256.0 - 2.0 ** -39) == FULL - 2 and scale(256.0 - 2.0 ** -41) == FULL
    assert scale(256.0 - 3 * 2.0 ** -41) == FULL - 2          # 2^48 - 1.5: the tie goes to the even one
    assert scale(float("inf")) == FULL and scale(float("nan")) == FULL and scale(1e300) == FULL
    assert scale(0.0) == 0 and scale(2.0 ** -41) == 0 and scale(3 * 2.0 ** -41) == 2 and scale(2.0 ** -40) == 1
    sides = {}
    for k in range(1, 200):
        a = float(F32(16.0 - k * 2.0 ** -20))
        b0 = F32(math.sqrt(256.0 - a * a))
        for b in (np.nextafter(b0, F32(0)), b0, np.nextafter(b0, F32(1))):
            p = float(Fraction(a) ** 2 + Fraction(float(Fraction(float(b)) ** 2)))
            sides.setdefault(p < 256.0, []).append((a, float(b), p))
    assert len(sides[True]) > 100 and len(sides[False]) > 100 and any(p == 256.0 for _a, _b, p in sides[False])
    for a, b, p in sides[True] + sides[False]:                  # within 4e-9 of 256 on either side
        assert abs(p - 256.0) < 4e-9
        assert Sq.ref_energies([[a, b]])[0] == model_energy(a, b) == (FULL if p >= 256.0 else round(p * 2.0 ** 40)), (a, b)
    edge = float(F32(16.0 - 2.0 ** -20))
    assert Sq.ref_energies([[edge, 0.0]])[0] == (1 << 48) - (1 << 25) + 1 == model_energy(edge, 0.0)
    full = [(16.0, 0.0), (0.0, -16.0), (16.0, 1e-30), (1e30, 0.0), (3e38, 3e38), (np.inf, 0.0), (0.0, -np.inf),
            (np.nan, 0.0), (1.0, np.nan), (np.inf, np.nan), (-np.inf, np.inf)]
    assert Sq.ref_energies(full).tolist() == [FULL] * len(full)
    # a window of 32768 such samples is 2^63: the sum does not wrap
    r = Sq.ref_squelch(np.full((1, 32768, 2), np.nan, F32), None, 32768, 1)
    assert r["nwindows"][0] == 1 and r["energy"][0, 0] == 1 << 63 and r["gate"][0, 0] == 1


# ---------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------
def machine(energies, open_level, close_level, hang, w0=0, gate=0, low=0, span_first=0):
    gates = []
    for w, e in enumerate(energies, w0):
        if e >= open_level:
            span_first = span_first if gate else w
            gate, low = 1, 0
        elif gate:
            low = 0 if e >= close_level else low + 1
            if low > hang:
                gate, low = 0, 0
        gates.append(gate)
    return gates, gate, low, span_first


def runs_of(gates, w0, open_in, span_first_in):
    """the maximal runs of open windows as the header reports them"""
    spans, at = [], None
    for j, g in enumerate(list(gates) + [0]):
        if g and at is None:
            at = j
        elif not g and at is not None:
            spans.append((span_first_in if at == 0 and open_in else w0 + at, w0 + j))
            at = None
    return spans


HIGH, MID, LOW = F32(1.0), F32(0.5), F32(0.0)        # energies 2^40, 2^38, 0 with one sample to the window
GATE_CASES = [(hang, same) for hang in (0, 1, 3, 100) for same in (False, True)]


@pytest.mark.parametrize("hang,same", GATE_CASES, ids=["hang%d%s" % (h, "-close==open" if s else "") for h, s in GATE_CASES])
def test_the_gate_against_the_machine(hang, same):
    rng = np.random.default_rng(100 + hang + same)
    open_level, close_level = 1 << 40, (1 << 40) if same else (1 << 38)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        weights = rng.dirichlet((1.0, 1.0, 4.0 if hang > 3 else 2.0))
        amp = rng.choice([HIGH, MID, LOW], n, p=weights).astype(F32)
        if hang > 3 and trial % 2:
            amp[int(rng.integers(0, n)):] = LOW         # a tail long enough for the hang time to run out
        iq = np.zeros((1, n + (-n) % 2, 2), F32)
        iq[0, :n, trial % 2] = amp
        state = np.zeros(1, STATE)
        if trial % 3:
            state[0] = (int(rng.integers(0, 1 << 40)), 0, int(rng.integers(0, 1000)), trial % 3 - 1, int(rng.integers(0, hang + 1)))
        w0 = int(state["seen"][0])
        r = Sq.ref_squelch(iq, [n], 1, open_level, close_level, hang, state=state, span_cap=n)
        energies = [int(round(float(a) ** 2 * 2 ** 40)) for a in amp]
        gate_in = int(state["open"][0])
        gates, gate, low, first = machine(energies, open_level, close_level, hang, w0, gate_in,
                                          int(state["low"][0]) if gate_in else 0, int(state["span_first"][0]))
        assert r["nwindows"][0] == n and r["energy"][0, :n].tolist() == energies
        assert r["gate"][0, :n].tolist() == gates, (trial, hang)
        out = r["state"][0]
        assert (out["seen"], out["acc"], out["open"], out["low"], out["span_first"]) == (w0 + n, 0, gate, low, first)
        want = runs_of(gates, w0, gate_in, int(state["span_first"][0]))
        assert r["nspans"][0] == len(want) and [tuple(x) for x in r["spans"][0, :len(want)].tolist()] == want


def test_the_hang_time_counts_consecutive_low_windows():
    """hang = 2: two low windows in a row leave the gate open, a window at or above close_level starts the count
    again, the third low one in a row closes it"""
    seq = [HIGH, LOW, LOW, MID, LOW, LOW, LOW, LOW, HIGH, LOW, LOW, HIGH, LOW, LOW, LOW, MID]
    iq = np.zeros((1, len(seq), 2), F32)
    iq[0, :, 0] = seq
    r = Sq.ref_squelch(iq, None, 1, 1 << 40, 1 << 38, 2)
    assert r["gate"][0, :16].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    assert r["spans"][0, :3].tolist() == [[0, 6], [8, 14], [Sq.FILL64, Sq.FILL64]] and r["nspans"][0] == 2
    assert r["state"][0]["open"] == 0 and r["state"][0]["low"] == 0


# ---------------------------------------------------------------------------
# pieces == the whole
# ---------------------------------------------------------------------------
N, B = 700, 96


def bursty_row(rng, n, s16):
    """noise at -50 dBFS with bursts of a carrier at -6 dBFS, the second one ragged"""
    amp = np.full(n, 10.0 ** (-50 / 20))
    amp[100:290] = 0.5
    amp[400:480:3] = 0.5
    amp[430:470] = 0.5
    ph = rng.uniform(0, 2 * np.pi, n)
    iq = (np.stack([np.cos(ph), np.sin(ph)], axis=1) * amp[:, None] + rng.standard_normal((n, 2)) * 1e-3).astype(F32)
    return np.round(iq * 32767).astype(np.int16) if s16 else iq


@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_pieces_equal_the_whole_for_every_cut(s16):
    rng = np.random.default_rng(7 + s16)
    iq = bursty_row(rng, N, s16)
    audio = rng.standard_normal(N).astype(F32)
    audio[[3, 250, 699]] = np.uint32(0x7FC12345).view(F32)          # a NaN with a payload
    levels = (Sq.ref_level(-12.0, B), Sq.ref_level(-20.0, B), 1)
    whole = Sq.ref_pieces(iq, [N], B, *levels, audio=audio)
    energy, gate, spans, state, muted = whole
    assert len(energy) == N // B == 7 and gate.tolist() == [0, 1, 1, 1, 1, 1, 0] and spans == [(1, 6)]
    assert (state["seen"][0], state["open"][0]) == (N, 0) and state["acc"][0] == int(Sq.ref_energies(
        iq.astype(F32) / (32768 if s16 else 1))[7 * B:].sum())
    # causal: the gate opens one window late and the hang time keeps one window of tail
    assert not muted[:2 * B].any() and same_bits(muted[2 * B:7 * B], audio[2 * B:7 * B]) and not muted[7 * B:].any()
    assert muted.view(np.uint32)[250] == 0x7FC12345 and not muted.view(np.uint32)[[3, 699]].any()

    def check(cuts):
        assert sum(cuts) == N
        e, g, sp, st, mu = Sq.ref_pieces(iq, cuts, B, *levels, audio=audio)
        assert np.array_equal(e, energy) and np.array_equal(g, gate) and sp == spans, cuts
        assert st.tobytes() == state.tobytes() and same_bits(mu, muted), cuts

    for c in range(N + 1):
        check([c, N - c])
    for trial in range(20):                                         # pieces shorter than a window, empty ones among them
        cuts = []
        while sum(cuts) < N:
            cuts.append(min(int(rng.integers(0, B)), N - sum(cuts)))
        assert max(cuts) < B and 0 in cuts + [0]
        check(cuts)
    check([1] * N)


def test_muting_keeps_open_samples_bit_for_bit():
    rng = np.random.default_rng(9)
    iq = bursty_row(rng, N, False)
    audio = np.full(N, np.uint32(0xFFC00001).view(F32))             # every sample a NaN with a payload
    _e, gate, _sp, _st, muted = Sq.ref_pieces(iq, [N], B, Sq.ref_level(-12.0, B), Sq.ref_level(-20.0, B), 0, audio=audio)
    assert gate.tolist() == [0, 1, 1, 0, 1, 0, 0]
    bits = muted.view(np.uint32)
    keyed = np.zeros(N, bool)
    keyed[2 * B:4 * B] = keyed[5 * B:6 * B] = True              # the windows behind an open one
    assert (bits[keyed] == 0xFFC00001).all() and not bits[~keyed].any()                                   # +0.0f


# ---------------------------------------------------------------------------
# spans across calls
# ---------------------------------------------------------------------------
def test_a_span_that_crosses_three_calls_keeps_its_first_window():
    iq = np.zeros((1, 40, 2), F32)
    iq[0, 5:31, 0] = 1.0
    state, seen = None, []
    for a, b in ((0, 12), (12, 22), (22, 40)):
        r = Sq.ref_squelch(np.ascontiguousarray(iq[:, a:b]), None, 2, 1 << 41, 1 << 41, 0, state=state)
        state = r["state"]
        seen.append((r["spans"][0, :r["nspans"][0]].tolist(), int(r["nwindows"][0])))
    # windows 3 .. 14 are open (window 2 holds one sample of the burst: 2^40 < 2^41)
    assert seen == [([[3, 6]], 6), ([[3, 11]], 5), ([[3, 15]], 9)]
    assert Sq.merge_spans([(np.array(s), len(s)) for s, _n in seen]) == [(3, 15)]
    assert state[0]["open"] == 0 and state[0]["span_first"] == 3
    # a call that completes no window reports no span, and the gate stays as it was
    state = Sq.ref_squelch(np.ascontiguousarray(iq[:, 6:14]), None, 2, 1 << 41, state=None)["state"]
    assert state[0]["open"] == 1
    r = Sq.ref_squelch(np.ascontiguousarray(iq[:, 14:16]), [1], 2, 1 << 41, state=state)
    assert r["nwindows"][0] == 0 and r["nspans"][0] == 0 and r["state"][0]["open"] == 1 and r["state"][0]["acc"] == 1 << 40
    # a gate that the call's first window closes reports nothing of the run before
    r = Sq.ref_squelch(np.zeros((1, 4, 2), F32), None, 2, 1 << 41, state=state)
    assert r["nspans"][0] == 0 and r["gate"][0, :2].tolist() == [0, 0]


def test_span_cap_overflow_keeps_the_true_count():
    iq = np.zeros((1, 24, 2), F32)
    iq[0, [2, 3, 8, 14, 15, 16, 21], 0] = 1.0
    for cap in (0, 1, 2, 5):
        r = Sq.ref_squelch(iq, None, 1, 1 << 40, span_cap=max(cap, 1), want=("energy", "gate", "state") + (("spans",) if cap else ()))
        want = [[2, 4], [8, 9], [14, 17], [21, 22]]
        if cap:
            assert r["nspans"][0] == 4
            assert r["spans"][0].tolist() == (want + [[Sq.FILL64] * 2] * 4)[:cap]
        assert r["gate"][0, :24].sum() == 7
