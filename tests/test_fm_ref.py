"""The FM stage on the host (include/mifsk.h: mifsk_fm_demod_batch, mifsk_fm_modulate_batch): the angle
header the device compiles (minimodem_amd/csrc/mifsk_angle.h, through tools/angle_check.c) against the
restatement tools/fm_ref.c bit for bit and against atan2; the restated modulator's integer phase; and the
round trip modulator -> discriminator within the bound the number formats give.  No device."""
import numpy as np

import _fm as Fm
from _fm import F32, same_bits


def assert_same_turns(got, want, y, x):
    if not same_bits(got, want):
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
        i = int(bad[0])
        raise AssertionError("%d angles differ, first for (y, x) = (%s, %s): %s != %s" % (
            len(bad), float(y[i]).hex(), float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()))


def test_the_header_equals_the_restatement_at_the_corners():
    y, x = Fm.corner_pairs()
    assert y.size > 500
    got, want = Fm.header_turns(y, x), Fm.ref_turns(y, x)
    assert_same_turns(got, want, y, x)
    # the corners are what they claim to be: NaN and Inf / Inf give NaN (y NaN beside x = +-0.0 gives 0.0: the
    # comparisons make the largest magnitude 0.0), everything else lies in [-0.5, 0.5]
    nan_in = np.isnan(y) | np.isnan(x)
    both_inf = np.isinf(y) & np.isinf(x)
    excepted = np.isnan(y) & (x == 0.0)
    assert np.isnan(want[(nan_in | both_inf) & ~excepted]).all() and (want[excepted] == 0.0).all()
    rest = want[~(nan_in | both_inf)]
    assert np.isfinite(rest).all() and rest.min() == -0.5 and rest.max() == 0.5
    # 1e308 either side: mn + mx overflows, the quotient is -0.0 and the answer an eighth of a turn
    assert Fm.ref_lib().fm_ref_turn(1e308, 1e308) == 0.125 and Fm.ref_lib().fm_ref_turn(-1e308, -1e308) == -0.375
    # the largest subnormal quotient survives the division
    assert Fm.ref_lib().fm_ref_turn(2.0 ** -1074, 2.0 ** -1074) == 0.125


def test_the_header_equals_the_restatement_on_random_pairs():
    rng = np.random.default_rng(1717)
    n = 1 << 16
    y = rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n)
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n)
    y[: n // 2] = rng.standard_normal(n // 2)
    x[: n // 2] = rng.standard_normal(n // 2)
    assert_same_turns(Fm.header_turns(y, x), Fm.ref_turns(y, x), y, x)


def test_the_angle_is_atan2_within_the_truncation_bound():
    """|turn - atan2 / (2 pi)| <= 4e-12 on 10^6 random finite pairs: the series' u^25 / 25 / (2 pi) = 1.7e-12 at
    u = tan(pi/8), and the rounding"""
    rng = np.random.default_rng(1718)
    n = 1000000
    y, x = rng.standard_normal(n), rng.standard_normal(n)
    y[:1000] *= 1e-5                    # near the axes
    x[1000:2000] *= 1e-5
    got = Fm.header_turns(y, x)
    want = np.arctan2(y, x) / (2.0 * np.pi)
    worst = float(np.abs(got - want).max())
    print("max |turn - atan2 / (2 pi)| = %.3g turns" % worst)
    assert worst <= 4e-12
    assert Fm.header_lib().angle_check_sweep(200000) <= 4e-12          # the tool's own sweep, long double atan2l


def test_fixed_values():
    turn = Fm.ref_lib().fm_ref_turn
    assert turn(0.0, 1.0) == 0.0 and turn(1.0, 0.0) == 0.25 and turn(0.0, -1.0) == 0.5
    assert turn(-1.0, 0.0) == -0.25
    for y in (0.0, -0.0):
        for x in (0.0, -0.0):
            assert turn(y, x) == 0.0
    assert turn(1.0, 1.0) == 0.125 and turn(1.0, -1.0) == 0.375 and turn(-1.0, -1.0) == -0.375
    assert turn(-1.0, 1.0) == -0.125
    y, x = np.array([0.0, 1.0, 0.0, -1.0, 0.0]), np.array([1.0, 0.0, -1.0, 0.0, 0.0])
    assert same_bits(Fm.header_turns(y, x), np.array([0.0, 0.25, 0.5, -0.25, 0.0]))


# ---------------------------------------------------------------------------
# the modulator's restatement
# ---------------------------------------------------------------------------
DEV = 3000.0 / 48000.0                  # turns per sample: exact


def test_the_phase_wraps_mod_2_64():
    x = np.full((2, 8), 0.5, F32)
    top = np.array([(1 << 64) - 1, 0], np.uint64)
    out, phase = Fm.ref_modulate(x, None, False, 8, DEV, phase0=top)
    step = int(0.5 * DEV * 2 ** 48)
    assert step == 1 << 43
    assert int(phase[0]) == ((1 << 64) - 1 + 8 * step) % (1 << 64) == 8 * step - 1
    assert int(phase[1]) == 8 * step
    # one unit of 2^-48 turns below: the word is one less at every sample
    w0 = ((np.arange(1, 9, dtype=np.uint64) * np.uint64(step) - np.uint64(1)) >> np.uint64(16)).astype(np.uint32)
    w1 = ((np.arange(1, 9, dtype=np.uint64) * np.uint64(step)) >> np.uint64(16)).astype(np.uint32)
    assert np.array_equal(w0 + np.uint32(1), w1)
    assert not same_bits(out[0], out[1]) and np.abs(out[0] - out[1]).max() < 1e-6
    # a negative step from 0 wraps below zero
    out, phase = Fm.ref_modulate(-x[:1], None, False, 8, DEV)
    assert int(phase[0]) == (1 << 64) - 8 * step
    # and the sample one turn on equals the sample here: 2^48 to the turn
    a, _p = Fm.ref_modulate(x[:1], None, False, 8, DEV, phase0=np.array([5 << 48], np.uint64))
    b, _p = Fm.ref_modulate(x[:1], None, False, 8, DEV)
    assert same_bits(a, b)


def test_steps_outside_the_range_are_zero():
    step = Fm.ref_lib().fm_ref_step
    assert step(1.0, DEV, 0.0) == 1 << 44 and step(-1.0, DEV, 0.0) == (1 << 64) - (1 << 44)
    assert step(0.0, DEV, 0.25) == 1 << 46
    # |d| >= 16384, NaN and Inf give 0; just below the limit does not
    assert step(16384.0, 1.0, 0.0) == 0 and step(-16384.0, 1.0, 0.0) == 0 and step(1.0, 1e9, 0.0) == 0
    assert step(float("nan"), DEV, 0.0) == 0 and step(float("inf"), DEV, 0.0) == 0
    assert step(float("-inf"), DEV, 0.0) == 0 and step(1.0, float("nan"), 0.0) == 0
    assert step(1.0, 0.0, float("inf")) == 0
    below = float(np.nextafter(F32(16384.0), F32(0.0)))
    assert step(below, 1.0, 0.0) == int(below * 2 ** 48) and step(-below, 1.0, 0.0) == (1 << 64) - int(below * 2 ** 48)
    # rint: to nearest even
    assert step(1.0, 2.5 * 2.0 ** -48, 0.0) == 2 and step(1.0, 3.5 * 2.0 ** -48, 0.0) == 4
    # in a row such a sample holds the phase where it was
    x = np.array([[0.5, np.nan, np.inf, 3e38, 0.5, -np.inf, 0.25, 0.0]], F32)
    out, phase = Fm.ref_modulate(x, None, False, 8, DEV)
    assert int(phase[0]) == (1 << 43) * 2 + (1 << 42)
    assert same_bits(out[0, 1], out[0, 0]) and same_bits(out[0, 3], out[0, 0]) and same_bits(out[0, 5], out[0, 4])
    assert np.isfinite(out).all()


def test_pieces_through_phase_out_equal_the_whole():
    rng = np.random.default_rng(1719)
    x = rng.uniform(-1.0, 1.0, (3, 4100)).astype(F32)
    phase0 = np.array([0, (1 << 64) - 1, 0x0123456789ABCDEF], np.uint64)
    for s16 in (False, True):
        whole, end = Fm.ref_modulate(x, None, s16, 4100, DEV, centre=-0.01, amplitude=0.7, phase0=phase0)
        phase, parts = phase0, []
        for a, b in ((0, 4), (4, 1028), (1028, 1029), (1029, 4100)):
            part, phase = Fm.ref_modulate(x[:, a:b], None, s16, b - a, DEV, centre=-0.01, amplitude=0.7, phase0=phase)
            parts.append(part)
        assert same_bits(np.concatenate(parts, axis=1), whole) and np.array_equal(phase, end)
    # and the discriminator's pieces through last -> prev
    iq, _end = Fm.ref_modulate(x, None, False, 4100, DEV)
    audio, last = Fm.ref_demod(iq, None, 4100, gain=16.0)
    prev, parts = None, []
    for a, b in ((0, 4), (4, 1028), (1028, 1029), (1029, 4100)):
        part, prev = Fm.ref_demod(iq[:, a:b], None, b - a, gain=16.0, prev=prev)
        parts.append(part)
    assert same_bits(np.concatenate(parts, axis=1), audio) and same_bits(prev, last)
    assert same_bits(last, iq[:, -1])


def test_round_trip_modulator_to_discriminator():
    """48 kHz, deviation 3 kHz, |x| <= 1: |out - x| <= gain (2 sqrt 2 2^-24 / (2 pi) + 2^-31) + 2^-23 for n >= 1 --
    the float rounding of I and Q (half an ulp of 1 on either part of either sample, as an angle), the 2^-32
    turn phase step taken twice, and the output's float rounding near 1."""
    rng = np.random.default_rng(1720)
    n = 20000
    x = np.stack([rng.uniform(-1.0, 1.0, n), np.sin(np.arange(n) * 0.05), np.sign(np.sin(np.arange(n) * 0.02)),
                  np.zeros(n)]).astype(F32)
    gain = 48000.0 / 3000.0
    iq, _phase = Fm.ref_modulate(x, None, False, n, DEV)
    out, _last = Fm.ref_demod(iq, None, n, gain=gain)
    bound = gain * (2.0 * np.sqrt(2.0) * 2.0 ** -24 / (2.0 * np.pi) + 2.0 ** -31) + 2.0 ** -23
    worst = float(np.abs(out[:, 1:].astype(np.float64) - x[:, 1:]).max())
    print("round trip: max |out - x| = %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound
    assert np.all(out[:, 0] == 0.0)                                     # no sample before the first: (0, 0)
