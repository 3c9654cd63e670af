"""Every correlator of csrc/mifsk_devlib.h, the four double accumulators compared as doubles.

The receive kernels claim "the oracle's sums in the oracle's order".  The parity tests look at
those sums after they are rounded to float and pushed through a magnitude: a correlator that
summed in another order, or multiplied and added unfused, would almost never change a frame.
Here mifsk_selftest_corr runs bit windows through ONE routine -- whole waves, every lane in the
routine, tables and derived configuration the product's own -- and returns the accumulators
unrounded; the reference is the oracle's ofsk_bit_dft_f64 on the same samples, compared with ==
(by value: corr_lds_fixed<1> documents that the sign of a zero may differ; NaN for NaN).

On N(0, 0.5) samples an unfused in-order sum differs from the fused one in 84 % of windows of 4
samples and in practically all longer ones (asserted below: at least half, for every length from
4 on), so plain random audio makes the comparison sharp.  Every routine at every bit length it
admits up to 130 (the tile also at 256 .. 320 and 1056), window starts at all four alignments
and different in every lane, 1 / 31 / 32 / 33 / 64 windows in a wave, the last legal position of
every bound -- and, in windows of their own, zeros, subnormals, 1e30, one infinity, one NaN."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

F32, F64 = np.float32, np.float64
NSPECIAL, NPLAIN = 35, 60            # 95 cases a call: a full wave and one of 31
B_MAX = 130


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, ctx
    ctx.close()


class Plans:
    """configuration + oracle plan per bit length: the Bell-202 bands (and FFT size) with the bit
    length set by hand, so that every length from 1 on has a table; 1056 is RTTY as it is"""

    def __init__(self):
        self.lib = O.oracle_lib()
        self.plans = {}

    def get(self, B):
        import minimodem_amd as M
        mode = "rtty" if B == 1056 else "1200"
        cfg, ocfg = M.rx_config(mode), O.oracle_config(mode)
        if mode not in self.plans:
            self.plans[mode] = self.lib.ofsk_plan_new(float(ocfg.sample_rate), ocfg.mark_f, ocfg.space_f,
                                                      ocfg.band_width)
        plan = self.plans[mode]
        assert (plan.contents.fftsize, plan.contents.b_mark, plan.contents.b_space) == \
               (cfg.fftsize, cfg.b_mark, cfg.b_space)
        if mode == "rtty":
            assert cfg.bit_nsamples == 1056
        cfg.bit_nsamples = B
        return cfg, plan

    def dft(self, plan, x, a, n):
        """ofsk_bit_dft_f64 of x[a : a + n]"""
        assert 0 <= a and a + n <= len(x)
        out = np.empty(4, F64)
        self.lib.ofsk_bit_dft_f64(plan, x.ctypes.data + 4 * int(a), int(n), out.ctypes.data)
        return out

    def table(self, plan, B):
        """[B, 4] twiddles as the oracle makes them"""
        tw = np.empty((B, 4), F64)
        w = np.empty(2, F64)
        for n in range(B):
            for j, b in enumerate((plan.contents.b_mark, plan.contents.b_space)):
                self.lib.ofsk_twiddle(int(b), n, int(plan.contents.fftsize), w.ctypes.data)
                tw[n, 2 * j: 2 * j + 2] = w
        return tw


@pytest.fixture(scope="module")
def plans():
    return Plans()


ALIGNED = {"lds_fixed", "lds_fixed_halves", "lds_stream", "lds_stream_lean"}


def reach(routine, B):
    """samples a routine loads from a window's start on (what must lie inside the array)"""
    if routine in ("lds_stream", "lds_stream_lean", "global_stream"):
        return 16 * ((B + 15) // 16)
    if routine == "global_tiled":
        return 32 * ((B + 31) // 32)
    return B


def admits(routine, B):
    if routine == "lds_fixed":
        return B % 4 == 0 and 4 <= B <= 48
    if routine == "lds_fixed_halves":
        return B % 4 == 0 and 8 <= B <= 48
    if routine in ("lds_stream", "lds_stream_lean"):
        return B % 4 == 0 and B >= 4
    return B >= 1


def make_input(routine, B, seed=0):
    """-> (samples, starts): 35 windows of special values, none overlapping another, then 60
    windows of N(0, 0.5) samples at starts of every alignment the routine takes, the last of
    them at the last legal position of the routine's bound"""
    rng = np.random.default_rng([seed, B, len(routine)])
    R = reach(routine, B)
    step = 1 if routine not in ALIGNED else 4
    pitch = ((R + 3) & ~3) + 4
    room = 256
    n = NSPECIAL * pitch + R + room
    x = rng.normal(0, 0.5, n).astype(F32)
    starts = []
    for k in range(NSPECIAL):
        a = k * pitch + (k % 4 if step == 1 else 0)
        w = x[a: a + B]
        kind = k % 5
        if kind == 0:                      # zeros: with a sample or two among them, all +0, all -0
            w[:] = 0.0 if k < 10 else -0.0
            if k < 5:
                w[rng.integers(0, B, size=min(B, 2))] = rng.normal(0, 0.5, min(B, 2))
        elif kind == 1:                    # subnormals
            w[:] = (w.astype(F64) * 1e-40).astype(F32)
        elif kind == 2:                    # 1e30
            w[:] = (w.astype(F64) * 2e30).astype(F32)
        elif kind == 3:                    # one infinity
            w[rng.integers(0, B)] = np.inf if k % 2 else -np.inf
        else:                              # one NaN
            w[rng.integers(0, B)] = np.nan
        starts.append(a)
    s0 = NSPECIAL * pitch
    last = n - R                           # a + reach == n: the last legal position
    assert s0 % 4 == 0 and (last % 4 == 0 or step == 1)
    plain = [s0, s0 + step, s0 + 2 * step, s0 + 3 * step, last]
    plain += (s0 + step * rng.integers(0, (last - s0) // step + 1, size=NPLAIN - len(plain))).tolist()
    starts += plain
    assert len(starts) == NSPECIAL + NPLAIN and len({a % 4 for a in plain}) == (4 if step == 1 else 1)
    assert np.any((np.abs(x) > 0) & (np.abs(x) < np.finfo(F32).tiny)) and np.isinf(x).sum() >= 7
    return x, np.array(starts, np.uint32)


def assert_sums_equal(got, exp, what):
    """== by value, NaN positions equal"""
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:6].tolist())
    bad = ~((got == exp) | nan)
    assert not bad.any(), (what, "%d of %d sums differ" % (bad.sum(), bad.size),
                           np.argwhere(bad)[:6].tolist(), got[bad][:4], exp[bad][:4])


def check(ctx, plans, routine, B, param=0, ncases=None, only_plain=False, seed=0):
    cfg, plan = plans.get(B)
    x, starts = make_input(routine, B, seed)
    if only_plain:
        starts = starts[starts > starts[NSPECIAL]]      # (the lowest start is no multiple of 4 then)
        assert int(starts.min()) % 4 == 1
    if ncases is not None:
        starts = starts[len(starts) - ncases:]
    got, _ = ctx.selftest_corr(cfg, routine, x, starts, param=param)
    exp = np.stack([plans.dft(plan, x, a, B) for a in starts])
    assert_sums_equal(got, exp, (routine, B, param, ncases))
    return len(starts)


SWEEP = [("lds_fixed", 0), ("lds_fixed_halves", 0), ("lds_stream", 0), ("lds_stream_lean", 0),
         ("global_stream", 0), ("global_tiled", 0), ("slab_plain", 0), ("skewed_stream", 0), ("skewed_stream", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("routine,param", SWEEP, ids=["%s-%d" % s if s[0] == "skewed_stream" else s[0] for s in SWEEP])
def test_correlator_sums_equal_the_oracles_at_every_bit_length(gpu, plans, routine, param):
    M, ctx = gpu
    lengths = [B for B in range(1, B_MAX + 1) if admits(routine, B)]
    assert lengths[0] == {"lds_fixed": 4, "lds_fixed_halves": 8, "lds_stream": 4, "lds_stream_lean": 4}.get(routine, 1)
    windows = 0
    for B in lengths:
        windows += check(ctx, plans, routine, B, param)
        if routine == "skewed_stream" and B % 3 == 0:
            check(ctx, plans, routine, B, param, only_plain=True)       # row 0 of the slab inside a float4
    assert windows == 95 * len(lengths)


@pytest.mark.gpu
@pytest.mark.parametrize("routine,param", SWEEP, ids=["%s-%d" % s if s[0] == "skewed_stream" else s[0] for s in SWEEP])
@pytest.mark.parametrize("ncases", [1, 31, 32, 33, 64])
def test_correlator_sums_with_partly_filled_waves(gpu, plans, routine, param, ncases):
    """lanes beyond the last case shadow a window; the tile's instantiation changes at 32"""
    M, ctx = gpu
    for B in (4, 8, 21, 40, 48, 92, 130):
        if admits(routine, B):
            assert check(ctx, plans, routine, B, param, ncases=ncases, seed=ncases) == ncases


@pytest.mark.gpu
@pytest.mark.parametrize("span", [(256, 288), (289, 320), (1056, 1056)], ids=["B256-288", "B289-320", "B1056"])
def test_tile_sums_equal_the_oracles_at_long_bit_lengths(gpu, plans, span):
    """every (short last step, tail of the last group) of the 32-sample tile step"""
    M, ctx = gpu
    for B in range(span[0], span[1] + 1):
        check(ctx, plans, "global_tiled", B)
        check(ctx, plans, "global_tiled", B, ncases=32, seed=1)        # the instantiation for <= 32 windows


def seg_input(B, shortest=1, seed=0):
    x, starts = make_input("slab_plain", B, seed)
    rng = np.random.default_rng([seed, B, 77])
    lens = rng.integers(shortest, B + 1, size=len(starts)).astype(np.uint32)
    lens[[3, 40, 70]] = B
    lens[[4, 41, 71]] = shortest
    # the last legal position of a + len <= n, for a long and for a short segment
    starts = starts.copy()
    starts[NSPECIAL + 4] = len(x) - int(lens[NSPECIAL + 4])
    starts[NSPECIAL + 5] = len(x) - int(lens[NSPECIAL + 5])
    return x, starts, lens


@pytest.mark.gpu
@pytest.mark.parametrize("never_whole", [0, 1], ids=["whole-below-shortest", "masked-throughout"])
def test_segment_sums_and_their_energy(gpu, plans, never_whole):
    """seg_group in lock step over the wave's longest segment, every lane a length of its own:
    the sums are the oracle's over that lane's segment alone; the float sum of squares (an error
    bound's input, not an output) lies within n * 2^-24 relative of the float64 one, n = the
    float operations of its chain: 8 fmas per group and the final addition of the two halves"""
    M, ctx = gpu
    unmasked_groups = 0
    for B in range(1, B_MAX + 1):
        cfg, plan = plans.get(B)
        # (at every fourth length no segment is shorter than 20: the waves' first group goes unmasked)
        x, starts, lens = seg_input(B, shortest=20 if B % 4 == 0 and B >= 20 else 1)
        got, esum = ctx.selftest_corr(cfg, "seg_group", x, starts, lens=lens, param=never_whole)
        exp = np.stack([plans.dft(plan, x, a, n) for a, n in zip(starts, lens)])
        assert_sums_equal(got, exp, ("seg_group", B, never_whole))
        for i in range(NSPECIAL, len(starts)):
            w0 = 64 * (i // 64)
            lmax = int(lens[w0: w0 + 64].max())
            nops = 8 * ((lmax + 15) // 16) + 1
            ref = float(np.sum(x[starts[i]: starts[i] + lens[i]].astype(F64) ** 2))
            assert abs(float(esum[i]) - ref) <= nops * 2.0 ** -24 * ref, (B, i, esum[i], ref, nops)
        unmasked_groups += int(lens[:64].min()) // 16 + int(lens[64:].min()) // 16
    assert never_whole or unmasked_groups > 0


def test_random_audio_tells_a_fused_in_order_sum_from_an_unfused_one(plans):
    """the inputs' own check, on the host: for every bit length from 4 on, a numpy sum of the
    same products in the same order, but rounded after the multiplication, differs from
    ofsk_bit_dft_f64 in at least half of the sweep's windows of random samples"""
    for B in range(4, B_MAX + 1):
        cfg, plan = plans.get(B)
        x, starts = make_input("global_stream", B)
        tw = plans.table(plan, B)
        differ = 0
        for a in starts[NSPECIAL:]:
            exp = plans.dft(plan, x, a, B)
            unfused = np.cumsum(x[a: a + B].astype(F64)[:, None] * tw, axis=0)[-1]
            assert np.allclose(unfused, exp, rtol=0, atol=1e-12 * B)
            differ += not np.array_equal(unfused, exp)
        assert differ >= NPLAIN // 2, (B, differ)


@pytest.mark.gpu
def test_corr_entry_refuses_what_would_break_a_precondition(gpu, plans):
    """-EINVAL and no launch: one past the last legal position of every bound, a misaligned LDS
    window, a bit length the routine does not take, bad segments, too many samples for LDS"""
    M, ctx = gpu
    for routine, B in (("lds_fixed", 40), ("lds_fixed_halves", 40), ("lds_stream", 52), ("lds_stream_lean", 52),
                       ("global_stream", 37), ("global_tiled", 37), ("global_tiled", 300), ("slab_plain", 37),
                       ("skewed_stream", 37)):
        cfg, plan = plans.get(B)
        x, starts = make_input(routine, B)
        step = 4 if routine in ALIGNED else 1
        last = len(x) - reach(routine, B)
        assert int(starts.max()) == last
        ctx.selftest_corr(cfg, routine, x, [last])                              # legal
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, routine, x, [0, last + step])
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, routine, x, [0xFFFFFFFF])
        if step == 4:
            for off in (1, 2, 3):
                with pytest.raises(ValueError):
                    ctx.selftest_corr(cfg, routine, x, [0, 4 + off])
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, routine, x, [0], param=2)
        if routine != "skewed_stream":
            with pytest.raises(ValueError):
                ctx.selftest_corr(cfg, routine, x, [0], param=1)
    for routine, B in (("lds_fixed", 52), ("lds_fixed", 6), ("lds_fixed_halves", 4), ("lds_fixed_halves", 52),
                       ("lds_stream", 6), ("lds_stream_lean", 3)):
        cfg, plan = plans.get(B)
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, routine, np.zeros(256, F32), [0])
    cfg, plan = plans.get(40)
    big = np.zeros(12292, F32)
    for routine in ("lds_fixed", "lds_stream", "slab_plain", "skewed_stream"):
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, routine, big, [0])
    ctx.selftest_corr(cfg, "global_stream", big, [0])
    x = np.ones(200, F32)
    ctx.selftest_corr(cfg, "seg_group", x, [160, 199], lens=[40, 1])            # legal, both at the end
    for starts, lens in (([161], [40]), ([0], [0]), ([0], [41]), ([200], [1])):
        with pytest.raises(ValueError):
            ctx.selftest_corr(cfg, "seg_group", x, starts, lens=lens)
    lib = M._lib.load()
    st = np.zeros(1, np.uint32)
    acc = np.zeros(4, F64)
    assert lib.mifsk_selftest_corr(ctx.handle, C.byref(cfg), 9, 0, x.ctypes.data, 200, st.ctypes.data, None, 1,
                                   acc.ctypes.data, None) == -22
    assert lib.mifsk_selftest_corr(ctx.handle, C.byref(cfg), 8, 0, x.ctypes.data, 200, st.ctypes.data, None, 1,
                                   acc.ctypes.data, None) == -22
    assert lib.mifsk_selftest_corr(ctx.handle, C.byref(cfg), 4, 0, None, 200, st.ctypes.data, None, 1,
                                   acc.ctypes.data, None) == -22
    assert lib.mifsk_selftest_corr(ctx.handle, C.byref(cfg), 4, 0, x.ctypes.data, 0, st.ctypes.data, None, 1,
                                   acc.ctypes.data, None) == -22
    # ... and the context still works
    got, _ = ctx.selftest_corr(cfg, "global_stream", x, [0])
    assert_sums_equal(got, plans.dft(plan, x, 0, 40)[None, :], "after the refusals")
