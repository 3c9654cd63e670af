"""The channel model's noise field on the host: the restatement (tools/impair_ref.c) against the
definition's known answers, the device's header (minimodem_amd/csrc/mifsk_gauss.h, compiled for the
host by tools/gauss_check.c) against the restatement bit for bit and against the C library, and the
field's moments."""
import numpy as np
import pytest

import _impair as Im
from _impair import same_bits


def _hex(values):
    return np.array([float.fromhex(v) for v in values], np.float64)


def test_philox_known_answers():
    cases = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for counter, key, words in cases:
        assert " ".join("%08x" % w for w in Im.ref_philox(counter, key)) == words
    # the header's Philox makes the same words: the block behind the second set of z below
    words = np.empty(4, np.uint32)
    Im.header_lib().gauss_check_field(0x01234567DEADBEEF, 5, 0x500000000 >> 2, 0, words.ctypes.data, None)
    assert " ".join("%08x" % w for w in words) == "02081902 623895ca 13b61ad3 32611d7f"
    assert same_bits(Im.ref_philox((0x40000000, 1, 5, 0), (0xDEADBEEF, 0x01234567)), words)


def test_z_known_answers_as_bit_patterns():
    want0 = _hex(("0x1.fb7665db1b649p-1", "-0x1.d96d5ff0aec98p-1", "-0x1.3c373dd6d9558p-1", "-0x1.eda3633cd971p-2"))
    want5 = _hex(("-0x1.2869a07130971p+1", "0x1.09bcef4090687p+1", "0x1.7c6ae00e54393p-1", "0x1.11cf48b0be383p+1"))
    seed5, n5 = 0x01234567DEADBEEF, 0x500000000
    lib = Im.ref_lib()
    assert same_bits(np.array([lib.impair_ref_z(0, 0, n) for n in range(4)]), want0)
    assert same_bits(np.array([lib.impair_ref_z(seed5, 5, n5 + n) for n in range(4)]), want5)
    assert same_bits(Im.ref_field(0, 0, 0, 4), want0) and same_bits(Im.ref_field(seed5, 5, n5, 4), want5)
    assert same_bits(Im.header_field(0, 0, 0, 4), want0) and same_bits(Im.header_field(seed5, 5, n5, 4), want5)
    # a count that is no multiple of 4, and w = 0xFFFFFFFF: R = -0.0
    assert same_bits(Im.ref_field(0, 0, 0, 3), want0[:3])
    rcs, _z = Im.ref_words([[0xFFFFFFFF, 0]])
    assert rcs[0, 0] == 0.0 and np.signbit(rcs[0, 0]) and rcs[0, 1] == 1.0 and rcs[0, 2] == 0.0


def test_the_transform_against_the_c_library_on_a_strided_sweep():
    """tools/gauss_check.c at stride 997: every |R - libm| and |C, S - libm| is at most 2^-40 (measured:
    below 1e-15; the bound is about 1000 times that and still 2^-16 of a float's last place at 1.0)."""
    mx = np.empty(2, np.float64)
    Im.header_lib().gauss_check_sweep(997, mx.ctypes.data)
    print("max |R - libm| = %.3g, max |C, S - libm| = %.3g" % (mx[0], mx[1]))
    assert mx[0] <= 2.0 ** -40 and mx[1] <= 2.0 ** -40


def test_the_header_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(16)
    words = rng.integers(0, 1 << 32, size=(1 << 20, 2), dtype=np.uint64).astype(np.uint32)
    corners = np.array(Im.corner_words(), np.uint32)
    edge = np.stack([np.repeat(corners, corners.size), np.tile(corners, corners.size)], axis=1)
    words = np.concatenate([edge, words])
    rcs_r, z_r = Im.ref_words(words)
    rcs_h, z_h = Im.header_words(words)
    assert same_bits(rcs_h, rcs_r)
    assert same_bits(z_h, z_r)
    assert same_bits(Im.header_field(77, 3, 1 << 34, 4096), Im.ref_field(77, 3, 1 << 34, 4096))
    assert not np.isnan(z_r).any() and np.isfinite(z_r).all()


@pytest.fixture(scope="module")
def normals():
    return Im.ref_field(0x0000000200000001, 0, 0, 1 << 22)


def test_moments_of_the_field_lie_within_five_standard_errors(normals):
    z = normals
    n = z.size
    mean, var = z.mean(), z.var()
    c = z - mean
    skew, kurt = (c ** 3).mean() / var ** 1.5, (c ** 4).mean() / var ** 2
    print("n = %d: mean %.5f, var %.5f, skew %.5f, kurt %.5f" % (n, mean, var, skew, kurt))
    # five standard errors of n = 2^22 normals: 5 / sqrt n, 5 sqrt(2 / n), 5 sqrt(6 / n), 5 sqrt(24 / n)
    assert abs(mean) <= 0.00244
    assert abs(var - 1.0) <= 0.00345
    assert abs(skew) <= 0.00946
    assert abs(kurt - 3.0) <= 0.0239


def test_the_largest_normal_is_bounded(normals):
    """R's maximum is sqrt(64 ln 2) = 6.66 (w = 0); C and S lie in [-1, 1]"""
    assert np.abs(normals).max() <= 6.67
    rcs, z = Im.ref_words([[0, 0], [0, 1 << 30], [0, 1 << 29]])
    assert abs(rcs[0, 0] - np.sqrt(64.0 * np.log(2.0))) < 1e-14 and np.abs(z).max() <= 6.67
    corners = np.array(Im.corner_words(), np.uint32)
    rcs, _z = Im.ref_words(np.stack([corners, corners], axis=1))
    assert np.abs(rcs[:, 1:]).max() <= 1.0 and rcs[:, 0].max() <= 6.67
