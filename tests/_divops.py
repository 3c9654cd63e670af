"""Operand pairs (x, c) for the float division x / c made through a double reciprocal
(`div_by_rcp`, minimodem_amd/csrc/mifsk_devlib.h): what tests/test_div_rcp_model.py feeds its numpy
model of that arithmetic and tests/test_gpu_devmath.py the device code itself.  Each generator
yields pairs of arrays (converted to float32 by the caller) and draws from `rng` in a fixed
order."""
import numpy as np


def random_pairs(rng, n):
    """magnitudes as the confidence pass sees them, then the whole float range"""
    x = rng.uniform(0, 2, n)
    c = rng.uniform(1e-3, 2, n)
    yield x, c
    bits = rng.integers(0, 0x7F7FFFFF, size=n, dtype=np.uint32)
    bits2 = rng.integers(0x00800000, 0x7F7FFFFF, size=n, dtype=np.uint32)
    yield bits.view(np.float32), bits2.view(np.float32)


def midpoint_operands(rng, n):
    """c in [1, 2) and, for each, the midpoint between a float q in [1, 2) and its upper
    neighbour (as a double)"""
    c = rng.integers(0x3F800000, 0x40000000, size=n, dtype=np.uint32).view(np.float32)     # [1, 2)
    q = rng.integers(0x3F800000, 0x40000000, size=n, dtype=np.uint32).view(np.float32)
    return c, q.astype(np.float64) + 2.0 ** -24                                            # a midpoint


def midpoint_pairs(rng, n):
    """x = q * c for q one step either side of a float midpoint: the hardest quotients there are"""
    c, mid = midpoint_operands(rng, n)
    for eps in (-2.0 ** -47, 2.0 ** -47, -2.0 ** -40, 2.0 ** -40):
        yield (mid * (1 + eps) * c.astype(np.float64)).astype(np.float32), c               # rounded: lands near


def small_integer_pairs(rng, n):
    """small integers over small integers (the frame length, the class counts)"""
    a = rng.integers(1, 1 << 24, size=n).astype(np.float32)
    b = rng.integers(1, 64, size=n).astype(np.float32)
    yield a, b
    yield a * np.float32(1e-7), np.full(n, 11, np.float32)
