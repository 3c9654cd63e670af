"""The lane scans of the bulk replay and the wave maximum, per lane, against serial references.

replay_scan_asm / _soft / _track (csrc/mifsk_devlib.h) replay the receive loop's float state --
amplitude tracker, running peak of the confidence, the two episode totals -- over up to 64 frames
as a DPP lane scan: hand-counted wait states, two register sets used in turn, a lane 0 that no
DPP instruction may write.  The parity tests see them only through whole frames.  Here
mifsk_selftest_scan seeds them as the receive loops do and returns every lane's state after (x)
and before (b) its frame; the reference is the recurrence of the routines' comments as a serial
float32 loop:
    t <- (t + a) * 0.5;  pk <- max(pk, c)  [soft: c < 0.75 pk ? c : max(pk, c)];  sc += c;  sa += a
compared as raw bits (where a total is NaN: NaN in both, x86 and gfx950 generate different NaNs).
wave_max_f32 is compared with the maximum numpy takes over the lanes that are not NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
T, PK, SC, SA = 0, 1, 2, 3
ROUTINES = ["asm", "soft", "track"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    c = M.Context()
    yield c
    c.close()


def serial_scan(routine, state, cv, av, K, totals):
    """-> (x[K, 4], b[K, 4]): the state after and before each of K frames, float32 throughout.
    What a routine leaves alone comes back as the receive loop seeded it: in x the first frame's
    update of the state before frame 0, in b that state."""
    t, pk, sc, sa = (F32(v) for v in state)
    t0, pk0, sc0, sa0 = t, pk, sc, sa
    x, b = np.zeros((K, 4), F32), np.zeros((K, 4), F32)
    half, k075 = F32(0.5), F32(0.75)
    with np.errstate(all="ignore"):
        for l in range(K):
            c, a = F32(cv[l]), F32(av[l])
            b[l] = (t, pk, sc, sa)
            t = F32(F32(t + a) * half)
            if routine == "asm":
                pk = c if pk < c else pk
            elif routine == "soft":
                pk = c if c < F32(pk * k075) else (c if pk < c else pk)
            if totals:
                sc, sa = F32(sc + c), F32(sa + a)
            x[l] = (t, pk, sc, sa)
            if routine == "track":          # the peak: untouched, i.e. every lane's own seed
                seed = c if pk0 < c else pk0
                x[l, PK] = c if c < F32(pk0 * k075) else seed
                b[l, PK] = pk0
            if not totals:
                x[l, SC], x[l, SA] = F32(sc0 + c), F32(sa0 + a)
                b[l, SC], b[l, SA] = sc0, sa0
    return x, b


def assert_same_bits(got, exp, what):
    got, exp = np.asarray(got, F32), np.asarray(exp, F32)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), what
    bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~nan
    assert not bad.any(), (what, np.argwhere(bad)[:8].tolist(), got[bad][:8], exp[bad][:8])


def _k_all():
    return np.arange(1, 65, dtype=np.uint32)             # wave w replays w + 1 frames


def case_plain(rng):
    """values in the ranges the loop produces: confidences of a few units, amplitudes below 1,
    totals of an episode some hundred frames old"""
    n = 64
    cv = rng.uniform(1.5, 9.0, (n, 64))
    av = rng.uniform(0.05, 1.0, (n, 64))
    state = np.stack([rng.uniform(0.05, 1.0, n), rng.uniform(1.5, 9.0, n),
                      rng.uniform(0, 3000.0, n), rng.uniform(0, 300.0, n)], axis=1)
    state[::7, 1:] = 0.0                                    # a fresh episode: no peak, no totals yet
    return state, cv, av


def case_falling(rng):
    """confidences that sag and recover, so that the soft rule (c < 0.75 pk: the peak restarts at
    c) fires in mid wave, several times"""
    n = 64
    base = 6.0 * np.exp(-np.arange(64) / rng.uniform(4, 30, (n, 1))) + 1.2
    cv = base * rng.uniform(0.8, 1.25, (n, 64))
    cv[:, 20::17] *= 3.0
    av = rng.uniform(0.05, 1.0, (n, 64))
    state = np.stack([rng.uniform(0.05, 1.0, n), rng.uniform(1.5, 12.0, n),
                      rng.uniform(0, 100.0, n), rng.uniform(0, 10.0, n)], axis=1)
    return state, cv, av


def case_ties(rng):
    """few distinct values: ties between the peak and the confidence, and confidences exactly AT
    0.75 x the peak (not below it: no restart) and one float below that (restart)"""
    n = 64
    below3 = np.nextafter(F32(3.0), F32(0.0))
    vals = np.array([4.0, 3.0, below3, 2.25, 4.0, 8.0, 6.0, np.nextafter(F32(6.0), F32(0.0)), 2.0], F32)
    cv = vals[rng.integers(0, len(vals), (n, 64))]
    av = np.array([0.5, 0.25, 1.0, 0.5], F32)[rng.integers(0, 4, (n, 64))]
    state = np.stack([np.full(n, 0.5), vals[rng.integers(0, len(vals), n)],
                      rng.integers(0, 64, n) * 4.0, rng.integers(0, 64, n) * 0.5], axis=1)
    return state, cv, av


def case_nan_and_inf(rng):
    """one NaN confidence per wave (the peak is left alone by it; the confidence total becomes
    NaN), an infinite one in every third wave"""
    state, cv, av = case_plain(rng)
    for w in range(64):
        cv[w, rng.integers(0, w + 1)] = np.nan
        if w % 3 == 0:
            cv[w, rng.integers(0, w + 1)] = np.inf
    return state, cv, av


def case_denormal(rng):
    """amplitudes, the tracker and the amplitude total in and around the float subnormals"""
    n = 64
    cv = rng.uniform(1.5, 9.0, (n, 64))
    av = (rng.uniform(0.0, 1.0, (n, 64)) * 10.0 ** rng.uniform(-45, -37, (n, 64)))
    av[:, ::9] = 0.0
    av[:, 5::11] = 1.4e-45
    state = np.stack([rng.uniform(0, 1, n) * 10.0 ** rng.uniform(-45, -37, n), rng.uniform(1.5, 9.0, n),
                      rng.uniform(0, 50.0, n), rng.uniform(0, 1, n) * 1e-38], axis=1)
    return state, cv, av


CASES = {"plain": case_plain, "falling": case_falling, "ties": case_ties,
         "nan-inf": case_nan_and_inf, "denormal": case_denormal}


@pytest.mark.parametrize("totals", [True, False], ids=["totals", "lean"])
@pytest.mark.parametrize("routine", ROUTINES)
@pytest.mark.parametrize("case", list(CASES))
def test_lane_scan_equals_the_serial_recurrence(ctx, case, routine, totals):
    """64 waves in one launch, wave w replaying K = w + 1 frames: every K from 1 to 64"""
    rng = np.random.default_rng([5, list(CASES).index(case)])
    state, cv, av = (np.asarray(v, F32) for v in CASES[case](rng))
    if case == "denormal":
        tiny = np.finfo(F32).tiny
        assert np.any((av > 0) & (av < tiny)) and np.any((state[:, T] > 0) & (state[:, T] < tiny))
    K = _k_all()
    x, b = ctx.selftest_scan(routine, state, cv, av, K, totals=totals)
    restarts = 0
    for w in range(64):
        k = int(K[w])
        ex, eb = serial_scan(routine, state[w], cv[w], av[w], k, totals)
        assert_same_bits(x[w, :k], ex, (case, routine, totals, "after", w))
        assert_same_bits(b[w, :k], eb, (case, routine, totals, "before", w))
        # what the routine must leave alone, said once more without the reference
        if not totals:
            assert_same_bits(b[w, :k, SC:], np.broadcast_to(state[w, SC:], (k, 2)), "totals untouched")
        if routine == "track":
            assert_same_bits(b[w, :k, PK], np.full(k, state[w, PK]), "peak untouched")
        restarts += int(np.sum(ex[1:, PK] < eb[1:, PK]))
    if routine == "soft" and case in ("falling", "ties"):
        assert restarts >= 32, restarts                    # (the soft rule did fire in mid wave)


def test_scans_agree_where_their_rules_coincide(ctx):
    """rising confidences never trip the soft rule: asm and soft give the same peaks, and all
    three the same tracker and totals"""
    rng = np.random.default_rng(11)
    state, cv, av = (np.asarray(v, F32) for v in case_plain(rng))
    cv = np.sort(cv, axis=1)
    state[:, PK] = 0.0
    K = _k_all()
    xa, ba = ctx.selftest_scan("asm", state, cv, av, K)
    xs, bs = ctx.selftest_scan("soft", state, cv, av, K)
    xt, bt = ctx.selftest_scan("track", state, cv, av, K)
    for w in range(64):
        k = int(K[w])
        assert_same_bits(xs[w, :k], xa[w, :k], ("soft == asm", w))
        assert_same_bits(bs[w, :k], ba[w, :k], ("soft == asm", w))
        for col in (T, SC, SA):
            assert_same_bits(xt[w, :k, col], xa[w, :k, col], ("track == asm", w, col))
            assert_same_bits(bt[w, :k, col], ba[w, :k, col], ("track == asm", w, col))


def test_scan_entry_refuses_bad_arguments(ctx):
    import minimodem_amd as M
    lib = M._lib.load()
    state, cv, av = np.zeros((1, 4), F32), np.ones((1, 64), F32), np.ones((1, 64), F32)
    x, b = np.zeros((1, 64, 4), F32), np.zeros((1, 64, 4), F32)
    for k, routine, totals in ((0, 0, 1), (65, 0, 1), (4, 3, 1), (4, -1, 1), (4, 0, 2)):
        kk = np.array([k], np.uint32)
        assert lib.mifsk_selftest_scan(ctx.handle, routine, totals, state.ctypes.data, cv.ctypes.data,
                                       av.ctypes.data, kk.ctypes.data, 1, x.ctypes.data, b.ctypes.data) == -22
    kk = np.array([4], np.uint32)
    assert lib.mifsk_selftest_scan(ctx.handle, 0, 1, None, cv.ctypes.data, av.ctypes.data, kk.ctypes.data, 1,
                                   x.ctypes.data, b.ctypes.data) == -22
    assert lib.mifsk_selftest_wave_max(ctx.handle, None, 1, x.ctypes.data) == -22


def test_wave_max_equals_numpy(ctx):
    rng = np.random.default_rng(3)
    waves = []
    # the maximum in each of the 64 lanes in turn, over values of both signs
    v = rng.normal(0, 100.0, (64, 64)).astype(F32)
    v[np.arange(64), np.arange(64)] = 1000.0 + np.arange(64)
    waves.append(v)
    # ... among confidences as the search hands them over: -inf for lanes without a candidate
    v = np.full((64, 64), -np.inf, F32)
    for w in range(64):
        lanes = rng.choice(64, size=1 + w % 9, replace=False)
        v[w, lanes] = rng.uniform(0.0, 9.0, len(lanes))
        v[w, w] = 10.0 + w
    waves.append(v)
    waves.append(np.full((1, 64), -np.inf, F32))                       # -inf everywhere
    v = rng.uniform(0.0, 9.0, (64, 64)).astype(F32)                     # one NaN lane: it never wins
    v[np.arange(64), np.arange(64)] = np.nan
    waves.append(v)
    v = np.full((64, 64), -np.inf, F32)                                 # NaN next to nothing but -inf
    v[np.arange(64), 63 - np.arange(64)] = np.nan
    waves.append(v)
    waves.append(rng.integers(0, 3, (16, 64)).astype(F32))              # ties
    waves.append(np.where(rng.random((8, 64)) < 0.5, np.inf, 1.0).astype(F32))
    v = np.concatenate(waves)
    got = ctx.selftest_wave_max(v)
    exp = np.fmax.reduce(v, axis=1)                                     # (np.max but for the NaN lanes)
    plain = ~np.isnan(v).any(axis=1)
    assert np.array_equal(exp[plain], np.max(v[plain], axis=1))
    assert not np.isnan(exp).any()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), np.argwhere(got != exp)[:8].tolist()
