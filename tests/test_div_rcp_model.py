"""The claim behind `div_by_rcp` (minimodem_amd/csrc/mifsk_devlib.h): for floats x, c with a
normal quotient, (float)((double)x * rc) is the IEEE float quotient x / c whenever rc is 1 / c in
double to within a few units in the last place -- the exact quotient of two 24-bit significands
stays at least 2^-48 (relative) away from every float rounding boundary, the product is within
2^-51 of it.  A numpy model of that arithmetic (float64 multiply, float32 rounding) over random
and adversarial operands, with the reciprocal perturbed by up to +-2 ulp (what v_rcp_f64 plus two
Newton steps can be off by).  That the device's reciprocal does stay within those 2 ulp, and that
its quotients are the IEEE ones on these same operands, is measured on the device by
tests/test_gpu_devmath.py (mifsk_selftest_rcp); the operand generators are shared (tests/_divops.py)."""
import numpy as np

import _divops


def _check(x, c):
    x = x.astype(np.float32)
    c = c.astype(np.float32)
    want = x / c                                            # IEEE float division
    normal = np.isfinite(want) & ((np.abs(want) >= np.finfo(np.float32).tiny) | (want == 0))
    rc = np.float64(1.0) / c.astype(np.float64)
    for k in (-2, -1, 0, 1, 2):
        r = rc
        for _ in range(abs(k)):
            r = np.nextafter(r, np.inf if k > 0 else -np.inf)
        got = (x.astype(np.float64) * r).astype(np.float32)
        bad = normal & (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        assert not bad.any(), (k, x[bad][:4], c[bad][:4], got[bad][:4], want[bad][:4])


def test_random_operands():
    rng = np.random.default_rng(1)
    n = 2_000_000
    with np.errstate(all="ignore"):
        # magnitudes as the confidence pass sees them, and the whole float range
        for x, c in _divops.random_pairs(rng, n):
            _check(x, c)


def test_quotients_next_to_rounding_boundaries():
    """x = q * c for q one step either side of a float midpoint: the hardest quotients there are."""
    rng = np.random.default_rng(2)
    n = 500_000
    with np.errstate(all="ignore"):
        for x, c in _divops.midpoint_pairs(rng, n):
            _check(x, c)
        # small integers over small integers (the frame length, the class counts)
        for x, c in _divops.small_integer_pairs(rng, n):
            _check(x, c)
