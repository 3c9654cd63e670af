"""The device arithmetic the receive kernels rest on, per value, against references made on the
host (numpy in float64 / IEEE float32, and the oracle's ofsk_frame_confidence) -- never against
other device code.  The kernels of minimodem_amd/csrc/mifsk_selftest.hip call the very routines
of mifsk_devlib.h / mifsk_devmath.h:

  * rcp_of_float / div_by_rcp: the reciprocal lies within the 2 ulp that tests/test_div_rcp_model.py
    proves sufficient, on every mantissa and every exponent; the quotients are IEEE's on that
    file's own operands;
  * sqrt_sumsq == the correctly rounded sqrt as a DOUBLE; sqrt_newton1's g stays inside the
    margin its guard (kSqrtGuard) assumes and gives the same float wherever the guard lets it
    through; band_mag == the hypotf identity, conversions and special values included;
  * frame_confidence and its fixed / staged layouts at twelve frame lengths on magnitudes no
    recording produces (ties, FLT_EPSILON noise, one-class frames, 0 / 0, inf, NaN, subnormals,
    overflow, quotients next to float midpoints, required bits), and the same plain frames
    through the reciprocal arm and -- with one odd lane planted per wave -- the division arm.

NaN equals NaN whatever its sign or payload; everything else is compared as bit patterns.
What is pinned is the routines' arithmetic as inlined into the self-test kernels, not how the
compiler schedules them inside a receive loop (tests/test_gpu_parity.py compares that)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _divops
import _oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FLT_EPSILON = F32(2.0 ** -23)
FLT_MAX = np.finfo(F32).max
N_BITS = [1, 4, 5, 6, 8, 10, 11, 12, 32, 33, 47, 64]
SPECIALISED = (8, 10, 11)
EINVAL = -22


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import minimodem_amd as M
    c = M.Context(0)
    yield c
    c.close()


def _same(got, want):
    """elementwise: the same bit pattern, or both NaN"""
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert got.dtype == want.dtype and got.shape == want.shape
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def _ulps(a, b):
    """distance of two finite doubles of one sign in units of the last place"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _first_bad(ok, *cols):
    i = np.flatnonzero(~ok)[:4]
    return [(int(k),) + tuple(c[k] for c in cols) for k in i]


# ---------------------------------------------------------------------------
# reciprocal and division
# ---------------------------------------------------------------------------

def test_reciprocal_is_within_the_two_ulp_the_division_proof_allows(ctx):
    """rcp_of_float(c) against 1.0 / float64(c) (correctly rounded on the host): at most 2 units in
    the last place apart -- exactly what test_div_rcp_model.py perturbs its model by.  Every
    mantissa of one exponent, 4096 mantissas at each of the 254 normal exponents, subnormal
    floats, both signs.  MEASURED on an MI355X: 0 ulp -- all 11 649 052 reciprocals are the
    correctly rounded ones (tests/README.md)."""
    rng = np.random.default_rng(11)
    one_exp = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(F32)         # [1, 2)
    exps = np.repeat(np.arange(1, 255, dtype=np.uint32), 4096) << np.uint32(23)
    all_exp = (exps | rng.integers(0, 1 << 23, size=exps.size, dtype=np.uint32)).view(F32)
    sub = np.concatenate([rng.integers(1, 1 << 23, size=1 << 16, dtype=np.uint32),
                          np.array([1, 2, 3, 0x7FFFFF, 0x400000], np.uint32)]).view(F32)
    edge = np.array([1.0, 2.0, 0.5, 3.0, 11.0, 10.0, 8.0, FLT_MAX, np.finfo(F32).tiny], F32)
    c = np.concatenate([one_exp, all_exp, sub, edge])
    c = np.concatenate([c, -one_exp[::8], -all_exp, -sub, -edge])
    x = rng.uniform(0, 2, c.size).astype(F32)
    rc, q = ctx.selftest_rcp(c, x)
    want = F64(1.0) / c.astype(F64)
    assert np.isfinite(rc).all() and (np.signbit(rc) == np.signbit(want)).all()
    d = _ulps(rc, want)
    worst = int(d.max())
    print("rcp_of_float: largest distance from 1.0 / c over %d values: %d ulp (%d values at it, %d exact)"
          % (c.size, worst, int((d == worst).sum()), int((d == 0).sum())))
    assert worst <= 2, "largest distance %d ulp, e.g. %r" % (worst, _first_bad(d <= 2, c, rc, want))
    # and the quotients made with it, where IEEE's is not subnormal
    with np.errstate(all="ignore"):
        wq = x / c
    plain = ~((wq != 0) & (np.abs(wq) < np.finfo(F32).tiny))
    ok = _same(q, wq) | ~plain
    assert ok.all(), _first_bad(ok, x, c, q, wq)


def _division_pairs():
    rng = np.random.default_rng(1)
    yield from _divops.random_pairs(rng, 1_000_000)
    rng = np.random.default_rng(2)
    yield from _divops.midpoint_pairs(rng, 500_000)
    yield from _divops.small_integer_pairs(rng, 500_000)
    # zeros, infinities and NaN over plain divisors (the divisor itself must be finite and not
    # zero: callers test that, float_is_plain)
    sx = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, np.finfo(F32).tiny, 2.0 ** -149], F32)
    sc = np.array([1.0, -3.0, 11.0, 2.0 ** -126, 2.0 ** -149, FLT_MAX, 0.1, 1.9999999], F32)
    yield np.repeat(sx, sc.size), np.tile(sc, sx.size)


def test_quotients_through_the_reciprocal_are_the_ieee_quotients(ctx):
    """div_by_rcp(x, rcp_of_float(c)) == float32 x / c on the operands of test_div_rcp_model.py
    (random, next to float midpoints, small integers), wherever the IEEE quotient is normal, zero,
    infinite or NaN (a subnormal quotient sends the wave through the division proper)."""
    tiny = np.finfo(F32).tiny
    total = pairs = 0
    for x, c in _division_pairs():
        x, c = x.astype(F32), c.astype(F32)
        with np.errstate(all="ignore"):
            want = x / c
        checked = ~((want != 0) & (np.abs(want) < tiny))
        _, got = ctx.selftest_rcp(c, x)
        ok = _same(got, want) | ~checked
        assert ok.all(), _first_bad(ok, x, c, got, want)
        total += int(checked.sum())
        pairs += x.size
    # (what is left out is the subnormal quotients of the pairs drawn from the whole float range)
    assert pairs > 5_000_000 and total > 0.98 * pairs


# ---------------------------------------------------------------------------
# square roots and band_mag
# ---------------------------------------------------------------------------

def _sumsq(fr, fi):
    """s as band_mag builds it: the squares of two floats are exact in double, their sum is
    rounded once"""
    fr, fi = fr.astype(F64), fi.astype(F64)
    return fr * fr + fi * fi


@functools.lru_cache(maxsize=None)
def _sqrt_inputs():
    """pairs of floats (fr, fi) and the index range of each group"""
    rng = np.random.default_rng(7)
    groups = []

    def add(name, a, b):
        groups.append((name, np.asarray(a, F32), np.asarray(b, F32)))

    # sums of squares of floats over all exponents (now and then infinite or NaN, as they come)
    n = 1 << 21
    add("random", rng.integers(0, 1 << 31, size=n, dtype=np.uint32).view(F32),
        rng.integers(0, 1 << 31, size=n, dtype=np.uint32).view(F32))
    add("zero and infinity", [0.0, -0.0, 0.0, np.inf, -np.inf, np.inf, 1.0], [0.0, 0.0, -0.0, 1.0, 0.0, np.inf, np.inf])
    # 2^-298 = (2^-149)^2 is the smallest sum that is not zero: it and its neighbours
    i, j = np.meshgrid(np.arange(16, dtype=np.uint32), np.arange(16, dtype=np.uint32))
    add("smallest", i.ravel().view(F32), j.ravel().view(F32))
    # around 2^-250, where sqrt_newton1's range test cuts (floats around 2^-125)
    lo = rng.integers(0x00800000, 0x02000000, size=1 << 14, dtype=np.uint32).view(F32)
    add("range cut", lo, np.where(rng.random(lo.size) < 0.5, 0, lo[::-1]))
    add("range cut exact", [2.0 ** -125, np.nextafter(F32(2.0 ** -125), F32(0)), np.nextafter(F32(2.0 ** -125), F32(1))],
        [0.0, 0.0, 0.0])
    top = (np.uint32(0x7F7FFFFF) - rng.integers(0, 4096, size=1 << 14, dtype=np.uint32)).view(F32)
    add("near 2 FLT_MAX^2", top, top[::-1].copy())
    f = rng.integers(0x00000001, 0x7F800000, size=1 << 19, dtype=np.uint32).view(F32)
    add("exact squares", f, np.zeros_like(f))
    # Next to float rounding boundaries, as selftest_sqrt_kernel places its values: m = a point
    # within +-600 double-ulps of the midpoint between float f and its upper neighbour, and the
    # sum of squares of two FLOATS nearest to m^2: fr = f, fi = (float)sqrt(m^2 - f^2) ~ f 2^-11.5.
    # Rounding fi to float moves the sum's root by up to 2^6 double-ulps, so the roots land
    # within +-664 of the midpoints: all inside the guard's 2^12, where the two paths can part.
    n = (1 << 20) + (1 << 19) - (1 << 15) - 512
    fb = rng.integers(30 << 23, 254 << 23, size=n, dtype=np.uint32)
    f = fb.view(F32)
    mid = 0.5 * (f.astype(F64) + (fb + np.uint32(1)).view(F32).astype(F64))
    m = (mid.view(np.int64) + rng.integers(-600, 601, size=n)).view(F64)
    add("float midpoints", f, np.sqrt((m - f.astype(F64)) * (m + f.astype(F64))).astype(F32))
    fr = np.concatenate([g[1] for g in groups])
    fi = np.concatenate([g[2] for g in groups])
    ends = np.cumsum([g[1].size for g in groups])
    where = {g[0]: slice(int(e - g[1].size), int(e)) for g, e in zip(groups, ends)}
    return fr, fi, where


@pytest.fixture(scope="module")
def sqrt_run(ctx):
    fr, fi, where = _sqrt_inputs()
    with np.errstate(all="ignore"):
        s = _sumsq(fr, fi)
        root = np.sqrt(s)                       # correctly rounded (IEEE 754)
        got_root, g, unsafe, mag = ctx.selftest_mag(fr.astype(F64), fi.astype(F64), 1.0)
    return dict(fr=fr, fi=fi, where=where, s=s, root=root, got_root=got_root, g=g, unsafe=unsafe, mag=mag)


def test_sqrt_inputs_are_where_they_should_be():
    """(the placement of the boundary cases, checked on the host)"""
    fr, fi, where = _sqrt_inputs()
    assert 0.98 * (1 << 22) < fr.size <= (1 << 22) + 4096
    sl = where["float midpoints"]
    root = np.sqrt(_sumsq(fr[sl], fi[sl]))
    off = np.abs((root.view(np.int64) & 0x1FFFFFFF) - (1 << 28))       # from the float midpoint
    assert off.max() <= 600 + 64 + 2 and np.median(off) > 100
    s = _sumsq(fr[where["smallest"]], fi[where["smallest"]])
    assert np.sort(np.unique(s))[:3].tolist() == [0.0, 2.0 ** -298, 2.0 ** -297]


def test_sqrt_sumsq_is_the_correctly_rounded_double(sqrt_run):
    r = sqrt_run
    ok = _same(r["got_root"], r["root"])
    assert ok.all(), _first_bad(ok, r["s"], r["got_root"], r["root"])
    # (s = 0 and s = inf come back as they went in: the sequence itself would make NaN of them)
    z = (r["s"] == 0) | np.isinf(r["s"])
    assert z.sum() >= 6 and _same(r["got_root"][z], r["s"][z]).all()


def test_short_sqrt_stays_inside_its_guard_margin(sqrt_run):
    """Wherever sqrt_newton1 calls a value safe, (float)g is (float)sqrt(s) and g lies within
    kSqrtGuard = 2^12 units of its last place of sqrt(s) -- the margin the guard's argument
    needs (mifsk_devmath.h claims 2^8).  It calls unsafe every s below 2^-250, zero, infinite
    or NaN.  MEASURED on an MI355X: at most 35 units over 4 170 195 sums in range, 2 630 609 of
    them called safe (tests/README.md)."""
    r = sqrt_run
    s, g, root, unsafe = r["s"], r["g"], r["root"], r["unsafe"]
    assert set(np.unique(unsafe).tolist()) <= {0, 1}
    out_of_range = ~(s >= 2.0 ** -250) | ~np.isfinite(s)              # (NaN: not >=)
    assert out_of_range.sum() > 1000
    assert (unsafe[out_of_range] == 1).all(), _first_bad(unsafe == 1, s, unsafe)
    safe = unsafe == 0
    assert np.isfinite(g[safe]).all() and (g[safe] > 0).all()
    with np.errstate(over="ignore"):
        ok = _same(g[safe].astype(F32), root[safe].astype(F32))
    assert ok.all(), _first_bad(ok, s[safe], g[safe], root[safe])
    d = _ulps(g[safe], root[safe])
    worst = int(d.max())
    # the same distance over the values the guard caught but whose s is in range: the bound is a
    # property of the sequence, not of the guard's verdict
    caught = ~safe & ~out_of_range
    worst_all = max(worst, int(_ulps(g[caught], root[caught]).max()))
    print("sqrt_newton1: largest |g - sqrt s| over %d safe values: %d units of g's last place "
          "(%d over all %d in range; claimed 2^8 = 256, guard 2^12 = 4096)"
          % (int(safe.sum()), worst, worst_all, int(safe.sum() + caught.sum())))
    assert worst < 1 << 12, "largest distance %d, e.g. %r" % (worst, _first_bad(d < 4096, s[safe], g[safe], root[safe]))
    assert worst_all < 1 << 12
    # the guard is neither idle nor a blanket: it catches the boundary cases (all within 666 of a
    # midpoint) and next to nothing of the random sums (2^13 / 2^29, the non-finite, the tiny)
    w = r["where"]
    assert (unsafe[w["float midpoints"]] == 1).all()
    assert unsafe[w["random"]].mean() < 0.02
    assert (unsafe[w["exact squares"]][s[w["exact squares"]] >= 2.0 ** -250] == 0).all()


def _band_mag_inputs():
    rng = np.random.default_rng(9)
    n = 1 << 17

    def doubles_between_floats(bits):
        # a float's value with random bits below its last place: the conversion has to round
        return (bits.view(F32).astype(F64).view(np.int64)
                | rng.integers(0, 1 << 29, size=bits.size)).view(F64) * rng.choice([-1.0, 1.0], bits.size)

    re = [doubles_between_floats(rng.integers(0, 0x7F800000, size=n, dtype=np.uint32))]
    im = [doubles_between_floats(rng.integers(0, 0x7F800000, size=n, dtype=np.uint32))]
    # subnormal floats and below: the conversion rounds at a fixed place, to 0 under 2^-150
    sub = rng.uniform(0, 2.0 ** -125, n // 4) * rng.choice([1.0, 2.0 ** -10, 2.0 ** -24], n // 4)
    re.append(sub)
    im.append(np.where(rng.random(sub.size) < 0.5, 0.0, sub[::-1]))
    # conversions that overflow to infinity, ties of the conversion, zeros, NaN, infinities
    top = float(FLT_MAX)
    sp = np.array([0.0, -0.0, 1.0, -1.0, 3.0, 4.0, top, top * (1 + 2.0 ** -26), top * (1 + 2.0 ** -25),
                   top * (1 + 2.0 ** -24), 1e39, -1e39, 1e300, -1e300, np.inf, -np.inf, np.nan,
                   2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52), 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149,
                   2.0 ** -126, 2.0 ** -126 * (1 - 2.0 ** -25), 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 5e-324])
    a, b = np.meshgrid(sp, sp)
    re.append(a.ravel())
    im.append(b.ravel())
    return np.concatenate(re), np.concatenate(im)


@pytest.mark.parametrize("scalar", [1.0, 2.0 / 40, 2.0 / 1056, 1.0 / (92 / 2.0)])
def test_band_mag_is_the_hypotf_identity(ctx, scalar):
    """band_mag(re, im, scalar) == float32(sqrt(float64(fr)^2 + float64(fi)^2)) * scalar with
    fr = float32(re), fi = float32(im): the reference's hypotf (tests/test_host_math.py pins that
    identity to the C library) on the FFT's float output, times its magscalar."""
    re, im = _band_mag_inputs()
    scalar = F32(scalar)
    with np.errstate(all="ignore"):
        fr, fi = re.astype(F32), im.astype(F32)
        want = np.sqrt(_sumsq(fr, fi)).astype(F32) * scalar
    assert np.isinf(fr[np.abs(re) > 3.5e38]).all()        # (the overflowing conversions are in)
    *_, got = ctx.selftest_mag(re, im, float(scalar))
    ok = _same(got, want)
    assert ok.all(), _first_bad(ok, re, im, got, want)
    # (+-inf, NaN): C's hypot() returns +inf for an infinite argument even when the other one is
    # NaN; band_mag returns NaN, and mifsk_devmath.h says why that changes nothing -- the pair
    # arises in both bands of a window alike, and the reference's confidence is then inf / inf,
    # NaN as well.  Pinned here so that a change of that behaviour is a decision.
    pair = (np.isinf(re) & np.isnan(im)) | (np.isnan(re) & np.isinf(im))
    assert pair.sum() == 4 and np.isnan(got[pair]).all()


# ---------------------------------------------------------------------------
# confidence
# ---------------------------------------------------------------------------

_BITS0, _AMPL0 = 0xDEADBEEFCAFEF00D, -123.5         # what "untouched" out-params still hold


def _expect(nb, req_mask, req_val):
    return "".join("d" if not (req_mask >> k) & 1 else str((req_val >> k) & 1) for k in range(nb)).encode()


def _oracle_conf(mags, req_mask=0, req_val=0):
    """ofsk_frame_confidence per case -> what the device must give: (conf, ampl, bits), and
    which cases a required bit rejected (the oracle returns 0.0 and leaves its out-params
    untouched there; the device returns 0, 0, 0)."""
    fn = O.oracle_lib().ofsk_frame_confidence
    nc, nb, _ = mags.shape
    expect = _expect(nb, req_mask, req_val)
    mark = np.ascontiguousarray(mags[:, :, 0], F32)
    space = np.ascontiguousarray(mags[:, :, 1], F32)
    conf, ampl, bits = np.zeros(nc, F32), np.zeros(nc, F32), np.zeros(nc, np.uint64)
    rejected = np.zeros(nc, bool)
    b, a = C.c_ulonglong(), C.c_float()
    pm, ps = mark.ctypes.data, space.ctypes.data
    for i in range(nc):
        b.value, a.value = _BITS0, _AMPL0
        c = fn(pm + 4 * nb * i, ps + 4 * nb * i, nb, expect, C.byref(b), C.byref(a))
        if b.value == _BITS0 and a.value == _AMPL0:
            assert c == 0.0
            rejected[i] = True
        else:
            conf[i], ampl[i], bits[i] = c, a.value, b.value
    return conf, ampl, bits, rejected


def _check_conf(got, want, where=None):
    gc, ga, gb, _ = got
    wc, wa, wb = want[:3]
    ok = _same(gc, wc) & _same(ga, wa) & (gb == wb)
    if where is not None:
        ok = ok | ~where
    assert ok.all(), _first_bad(ok, gc, wc, ga, wa, gb, wb)


@functools.lru_cache(maxsize=None)
def _plain(nb):
    """4096 frames (64 waves) as a demodulated signal's are: both magnitudes in [2^-10, 2],
    distinct"""
    rng = np.random.default_rng(1000 + nb)
    m = (2.0 ** -10 + rng.random((4096, nb, 2)) * (2.0 - 2.0 ** -10)).astype(F32)
    tie = m[:, :, 0] == m[:, :, 1]
    m[:, :, 1][tie] = np.nextafter(m[:, :, 1][tie], F32(0))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _planted(nb):
    """the plain frames with lane 0 of every wave replaced by a frame of magnitudes 2^-140: its
    avg_sig is subnormal, which sends its whole wave through the division arm"""
    m = _plain(nb).copy()
    m[0::64] = F32(2.0 ** -140)
    m.setflags(write=False)
    return m


def _midpoint_frames(nb, count, rng):
    """Frames whose divergence terms |sig - cls| / cls are quotients NEXT TO A FLOAT MIDPOINT,
    as near as two floats' quotient gets.  The divisor comes from the midpoint generator of
    tests/_divops.py, cut to 20 bits (C, odd); the dividend X is SOLVED for: X 2^k - N C = +-1
    with N odd puts X / C at 1 / (C 2^k) from the midpoint N / 2^k of two adjacent floats.  The
    mark class is pairs of (C + X) u and (C - X) u: every partial sum is an integer below 2^24
    (exact), so the class mean is C u exactly and each term is X / C; the other bits are space
    bits of one magnitude (terms 0).  The confidence is snr * (1 - divergence): a quotient
    rounded the wrong way shows in it."""
    pairs = min(nb, 8) // 2
    if pairs == 0:
        return np.zeros((0, nb, 2), F32)
    u = 2.0 ** -20
    frames = []
    while len(frames) < count:
        c, _ = _divops.midpoint_operands(rng, 256)
        for cv in c.tolist():
            Cq = (int(cv * 2 ** 23) >> 4) | 1                                   # [2^19, 2^20), odd
            j, delta = int(rng.integers(1, 3)), int(rng.choice([-1, 1]))
            k = j + 24                                                          # quotients in [2^-j, 2^(1-j))
            X = (delta * pow(1 << k, -1, Cq)) % Cq
            N = (X * (1 << k) - delta) // Cq
            if not (N & 1 and (1 << 24) <= N < (1 << 25) and 2 <= X <= Cq - 2):
                continue
            assert X * (1 << k) - N * Cq == delta
            m = np.empty((nb, 2), F32)
            m[:, 0], m[:, 1] = 2.0 ** -22, 1.0                                  # space bits
            m[:2 * pairs:2, 0] = (Cq + X) * u                                   # mark bits
            m[1:2 * pairs:2, 0] = (Cq - X) * u
            m[:2 * pairs, 1] = 2.0 ** -22
            frames.append(m)
            if len(frames) == count:
                break
    return np.stack(frames)


@functools.lru_cache(maxsize=None)
def _edges(nb):
    """1024 frames: edge cases at scattered lanes of waves of otherwise plain frames.  Every
    magnitude is +0, positive, +inf or NaN."""
    rng = np.random.default_rng(2000 + nb)
    base = _plain(nb)[:1024].copy()
    special = []

    def frame():
        return base[int(rng.integers(0, 1024))].copy()

    ks = sorted({0, nb // 2, nb - 1})
    for k in ks:                                    # mark == space in one bit (the strict >)
        f = frame()
        f[k, 1] = f[k, 0]
        special.append(f)
    f = frame()                                     # ... and in every bit
    f[:, 1] = f[:, 0]
    special.append(f)
    eps3 = [np.nextafter(FLT_EPSILON, F32(0)), FLT_EPSILON, np.nextafter(FLT_EPSILON, F32(1))]
    for e in eps3:                                  # noise exactly FLT_EPSILON and its neighbours
        for k in ks:
            for side in (0, 1):
                f = frame()
                f[k, side] = e
                special.append(f)
        for side in (0, 1):
            f = frame()
            f[:, side] = e
            special.append(f)
    for side in (0, 1):                             # all-mark and all-space frames
        f = frame()
        f.sort(axis=1)
        special.append(f if side else f[:, ::-1].copy())
    f = frame()                                     # a class whose magnitudes are all +0 (0 / 0)
    f[f[:, 0] < f[:, 1]] = 0.0
    special.append(f)
    f = frame()
    f[::2, 1] = 0.0
    f[::2, 0] = 0.0
    special.append(f)
    special.append(np.zeros((nb, 2), F32))
    for v in (np.inf, np.nan):                      # +inf and NaN magnitudes in one bit
        for k in ks:
            for side in (0, 1, 2):
                f = frame()
                if side == 2:
                    f[k, :] = v
                else:
                    f[k, side] = v
                special.append(f)
    f = frame()
    f[ks[0], 0], f[ks[-1], 1] = np.inf, np.nan
    special.append(f)
    for scale in (2.0 ** -126, 2.0 ** -135, 2.0 ** -147):       # subnormal magnitudes
        special.append((frame() * F32(scale)).astype(F32))
        for k in ks:
            f = frame()
            f[k] *= F32(scale)
            special.append(f)
    for scale in (0.45, 0.5, 0.26):                 # near FLT_MAX: the sums overflow
        special.append((frame() * F32(scale) * FLT_MAX).astype(F32))
    f = frame()
    f[ks[-1], 0] = FLT_MAX
    special.append(f)
    special.extend(_midpoint_frames(nb, 96, rng))
    special = np.stack(special).astype(F32)
    assert len(special) <= 320 and not np.signbit(special).any()
    # three per wave and at varying lanes; the rest of each wave stays plain
    at = (np.arange(len(special)) * 3 + np.arange(len(special)) % 3) % 1024
    at = np.unique(at)[:len(special)]
    assert len(at) == len(special)
    base[at] = special
    base.setflags(write=False)
    return base


def _required(nb):
    """the first, the last and a middle bit, and a bit above 32 where there is one"""
    ks = sorted({0, nb // 2, nb - 1} | ({40} if nb > 40 else set()))
    mask = sum(1 << k for k in ks)
    val = sum(1 << k for i, k in enumerate(ks) if i % 2 == 0)
    return ks, mask, val


@functools.lru_cache(maxsize=None)
def _required_cases(nb):
    """the plain frames with their required bits made right (even cases) or right but for one
    (odd cases): lanes of one wave leave at the rejection while their neighbours go on"""
    rng = np.random.default_rng(3000 + nb)
    ks, mask, val = _required(nb)
    m = _plain(nb).copy()
    for k in ks:
        hi, lo = m[:, k].max(axis=1), m[:, k].min(axis=1)
        one = bool((val >> k) & 1)
        m[:, k, 0], m[:, k, 1] = (hi, lo) if one else (lo, hi)
    wrong = rng.choice(ks, size=m.shape[0])
    for i in range(1, m.shape[0], 2):
        m[i, wrong[i]] = m[i, wrong[i], ::-1].copy()
    m.setflags(write=False)
    return m


_SETS = {"plain": _plain, "planted": _planted, "edges": _edges, "required": _required_cases}


@functools.lru_cache(maxsize=None)
def _want(name, nb):
    if name == "required":
        _, mask, val = _required(nb)
        return _oracle_conf(_SETS[name](nb), mask, val)
    return _oracle_conf(_SETS[name](nb))


_got_cache = {}


def _got(ctx, name, nb, variant):
    key = (name, nb, variant)
    if key not in _got_cache:
        mask, val = _required(nb)[1:] if name == "required" else (0, 0)
        _got_cache[key] = ctx.selftest_confidence(variant, _SETS[name](nb), mask, val)
    return _got_cache[key]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("nb", N_BITS)
def test_confidence_of_plain_frames(ctx, nb, variant):
    got = _got(ctx, "plain", nb, variant)
    _check_conf(got, _want("plain", nb))
    # nothing in [2^-10, 2] can be zero, non-finite or give a subnormal quotient
    assert (got[3] == 0).all()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("nb", N_BITS)
def test_confidence_reciprocal_arm_and_division_arm_agree(ctx, nb, variant):
    """One odd lane per wave sends the other 63 -- plain frames -- through the divisions proper:
    they must give what they gave through the reciprocals, and what the oracle gives."""
    got = _got(ctx, "planted", nb, variant)
    _check_conf(got, _want("planted", nb))
    specialised = nb in SPECIALISED and variant in (1, 2)
    assert (got[3] == (1 if specialised else 0)).all()
    others = np.arange(4096) % 64 != 0
    plain = _got(ctx, "plain", nb, variant)
    _check_conf(got, plain, where=others)
    assert (plain[3] == 0).all()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("nb", N_BITS)
def test_confidence_of_edge_cases(ctx, nb, variant):
    """ties, FLT_EPSILON noise, one-class frames, 0 / 0, inf, NaN, subnormals, overflow and
    quotients next to float midpoints, in waves of otherwise plain frames"""
    _check_conf(_got(ctx, "edges", nb, variant), _want("edges", nb))


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("nb", N_BITS)
def test_confidence_with_required_bits(ctx, nb, variant):
    _, mask, val = _required(nb)
    m = _required_cases(nb)
    want = _want("required", nb)
    rejected = want[3]
    # (the cases are what they were built to be: every other one violates)
    assert (rejected == (np.arange(len(m)) % 2 == 1)).all()
    got = _got(ctx, "required", nb, variant)
    _check_conf(got, want)                          # (rejected: 0, 0, 0 on both sides)
    gc, ga, gb, fb = got
    assert (gc[rejected].view(np.uint32) == 0).all() and (ga[rejected].view(np.uint32) == 0).all()
    assert (gb[rejected] == 0).all()
    assert ((gb[~rejected] & np.uint64(mask)) == np.uint64(val)).all()
    assert (fb == 0).all()


@pytest.mark.parametrize("nb", N_BITS)
def test_confidence_variants_agree(ctx, nb):
    """the three layouts on the same frames, against one another"""
    for name in ("plain", "planted", "edges", "required"):
        ref = _got(ctx, name, nb, 0)
        for variant in (1, 2):
            _check_conf(_got(ctx, name, nb, variant), ref)


def test_selftest_entries_refuse_bad_arguments(ctx):
    from minimodem_amd import _lib
    lib = _lib.load()
    h = ctx.handle
    m = np.ones((4, 8, 2), F32)
    conf, ampl = np.zeros(4, F32), np.zeros(4, F32)
    bits, fb = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    good = [h, 1, 8, 0, 0, m.ctypes.data, 4, conf.ctypes.data, ampl.ctypes.data, bits.ctypes.data, fb.ctypes.data]
    assert lib.mifsk_selftest_confidence(*good) == 0
    for pos, bad in ((0, None), (1, -1), (1, 3), (2, 0), (2, 65), (5, None), (7, None), (8, None), (9, None), (10, None)):
        args = list(good)
        args[pos] = bad
        assert lib.mifsk_selftest_confidence(*args) == EINVAL, (pos, bad)
    c, x = np.ones(4, F32), np.ones(4, F32)
    rc, q = np.zeros(4, F64), np.zeros(4, F32)
    good = [h, c.ctypes.data, x.ctypes.data, 4, rc.ctypes.data, q.ctypes.data]
    assert lib.mifsk_selftest_rcp(*good) == 0 and rc.tolist() == [1.0] * 4
    for pos in (0, 1, 2, 4, 5):
        args = list(good)
        args[pos] = None
        assert lib.mifsk_selftest_rcp(*args) == EINVAL, pos
    re, im = np.ones(4, F64), np.zeros(4, F64)
    root, g, un, mag = np.zeros(4, F64), np.zeros(4, F64), np.zeros(4, np.uint8), np.zeros(4, F32)
    good = [h, re.ctypes.data, im.ctypes.data, 1.0, 4, root.ctypes.data, g.ctypes.data, un.ctypes.data, mag.ctypes.data]
    assert lib.mifsk_selftest_mag(*good) == 0 and root.tolist() == [1.0] * 4
    for pos in (0, 1, 2, 5, 6, 7, 8):
        args = list(good)
        args[pos] = None
        assert lib.mifsk_selftest_mag(*args) == EINVAL, pos
