"""mifsk_detect_carrier_batch (include/mifsk.h, minimodem_amd/csrc/mifsk_carrier.hip): fsk_detect_carrier
on windows of every stream of a batch, against the oracle's ofsk_detect_carrier window by window --
every evaluated window of every case, bands exactly, magnitudes as f32 bit patterns, no tolerance.

Audio comes from the project's own synthesiser and a seeded generator; every case is a batch of a few
short streams.  All three output arrays are made with guard cells around them, which every call
must leave alone."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE, NO_WINDOW = -1, -2
GUARD = 64
BAND_GUARD, MAG_GUARD = -77, F32(7.25)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


# ---------------------------------------------------------------------------
# the oracle's side
# ---------------------------------------------------------------------------
_PLANS = {}


def _plan(cfg):
    key = (int(cfg.sample_rate), float(cfg.mark_f), float(cfg.space_f), float(cfg.band_width))
    if key not in _PLANS:
        p = O.oracle_lib().ofsk_plan_new(float(cfg.sample_rate), cfg.mark_f, cfg.space_f, cfg.band_width)
        assert p.contents.fftsize == cfg.fftsize and p.contents.nbands == cfg.nbands
        _PLANS[key] = p
    return _PLANS[key]


def oracle_band(cfg, win, threshold):
    win = np.ascontiguousarray(win, F32)
    return int(O.oracle_lib().ofsk_detect_carrier(_plan(cfg), win.ctypes.data, win.shape[0], C.c_float(threshold)))


def same_f32(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def evaluated(n, stride, first, window, hop, w):
    """window w lies wholly inside a row of n samples (clamped to the row's stride)"""
    return first + w * hop + window <= min(n, stride)


# ---------------------------------------------------------------------------
# one call, with guard cells around its outputs
# ---------------------------------------------------------------------------
def survey(gpu, cfg, x, lens=None, window=None, hop=None, first=0, nwindows=None, threshold=0.001,
           spectrum=True, rxnoise=0.0, stream=None):
    """-> dict of numpy arrays: band, mag, spectrum (guard pattern where nothing was written), window,
    hop, nwindows.  Asserts that the guard cells around the three arrays are intact."""
    M, torch, ctx = gpu
    d = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ns, width = d.shape
    dl = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    window = M.carrier_window_default(cfg) if window is None else window
    hop = hop or window
    if nwindows is None:
        nwindows = max(1, M.carrier_windows(width, window, hop, first))
    nb = int(cfg.nbands)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        fb = torch.full((ns * nwindows + 2 * GUARD,), BAND_GUARD, dtype=torch.int32, device=d.device)
        fm = torch.full((ns * nwindows + 2 * GUARD,), float(MAG_GUARD), dtype=torch.float32, device=d.device)
        fs = torch.full((ns * nwindows * nb + 2 * GUARD,), float(MAG_GUARD), dtype=torch.float32, device=d.device)
    out = {"band": fb[GUARD:GUARD + ns * nwindows].view(ns, nwindows),
           "mag": fm[GUARD:GUARD + ns * nwindows].view(ns, nwindows)}
    if spectrum:
        out["spectrum"] = fs[GUARD:GUARD + ns * nwindows * nb].view(ns, nwindows, nb)
    res = M.carrier_survey(ctx, cfg, d, nsamples=dl, window=window, hop=hop, first=first, nwindows=nwindows,
                           threshold=threshold, spectrum=spectrum, rxnoise=rxnoise, stream=stream, out=out)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    assert res["window"] == window and res["hop"] == hop
    hb, hm, hs = fb.cpu().numpy(), fm.cpu().numpy(), fs.cpu().numpy()
    for flat, guard in ((hb, BAND_GUARD), (hm, MAG_GUARD), (hs, MAG_GUARD)):
        assert (flat[:GUARD] == guard).all() and (flat[-GUARD:] == guard).all(), "a guard cell was written"
    if not spectrum:
        assert (hs == MAG_GUARD).all()
    return {"band": hb[GUARD:-GUARD].reshape(ns, nwindows), "mag": hm[GUARD:-GUARD].reshape(ns, nwindows),
            "spectrum": hs[GUARD:-GUARD].reshape(ns, nwindows, nb), "window": window, "hop": hop,
            "nwindows": nwindows, "first": first, "threshold": threshold}


def check_bands(cfg, x, lens, r, check_mag=True):
    """every window of `r`: the oracle's band where it is evaluated, NO_WINDOW / 0 / an untouched
    spectrum row where not; the winner's magnitude by the oracle alone; the spectrum's own
    consistency.  Returns (evaluated, with a band)."""
    ns, stride = x.shape
    window, hop, first, thr = r["window"], r["hop"], r["first"], r["threshold"]
    n_eval = n_band = 0
    for s in range(ns):
        n = stride if lens is None else int(lens[s])
        for w in range(r["nwindows"]):
            band, mag, spec = int(r["band"][s, w]), r["mag"][s, w], r["spectrum"][s, w]
            if not evaluated(n, stride, first, window, hop, w):
                assert band == NO_WINDOW and same_f32(mag, 0.0), (s, w, band, mag)
                assert (spec == MAG_GUARD).all(), (s, w)
                continue
            n_eval += 1
            a = first + w * hop
            win = x[s, a:a + window]
            assert band == oracle_band(cfg, win, thr), (s, w, band, oracle_band(cfg, win, thr))
            if band < 0:
                assert band == NONE and same_f32(mag, 0.0), (s, w, band, mag)
            else:
                n_band += 1
                assert 1 <= band < cfg.nbands
                if check_mag:
                    # bit for bit the oracle's: it is the largest threshold the band still passes
                    assert oracle_band(cfg, win, mag) == band, (s, w, band, mag)
                    if np.isfinite(mag):
                        assert oracle_band(cfg, win, np.nextafter(mag, F32(np.inf))) == NONE, (s, w, band, mag)
            if not (spec == MAG_GUARD).all():           # (a call with the spectrum)
                assert not (spec == MAG_GUARD).any(), (s, w)
                if band >= 1:
                    assert same_f32(spec[band], mag), (s, w)
                best, best_band = F32(0.0), NONE        # fsk.c:554-580 on the spectrum
                for b in range(1, cfg.nbands):
                    if spec[b] < F32(thr):
                        continue
                    if best < spec[b]:
                        best, best_band = spec[b], b
                assert best_band == band, (s, w, best_band, band)
    return n_eval, n_band


# ---------------------------------------------------------------------------
# audio
# ---------------------------------------------------------------------------
def rows_for(M, cfg, width, seed, nrows=6, noise=0.02):
    """rows of `width` samples: frames behind silences, AWGN on some, one all-zero row, one with a NaN
    and an Inf, noise alone"""
    rng = np.random.default_rng(seed)
    x = np.zeros((nrows, width), F32)
    B = max(4, int(cfg.nsamples_per_bit))
    for s in range(nrows):
        kind = s % 6
        if kind == 2:
            continue                                                     # all zero
        if kind == 5:
            x[s] = rng.normal(0, 0.003, width).astype(F32)               # noise about the threshold
            continue
        words = rng.integers(32, 127, size=max(2, width // (10 * B) + 1), dtype=np.uint8)
        sig = M.synthesize(cfg, words, amplitude=float(rng.uniform(0.3, 1.0)))
        lead = (0, 3 * B + 1, 0, B // 2, 7 * B)[kind]
        lead = min(lead, width // 3)
        k = min(len(sig), width - lead)
        x[s, lead:lead + k] = sig[:k]
        if kind in (0, 4):
            x[s] += rng.normal(0, noise, width).astype(F32)
        if kind == 3:
            x[s, width // 2] = np.nan
            x[s, width // 4 + 1] = np.inf
    return x


MODES = {
    # name: (baudmode, options, row width, rows)
    "1200": ("1200", {}, 1000, 6),
    "1200-24k": ("1200", {"sample_rate": 24000}, 500, 6),
    "12000": ("12000", {}, 260, 6),
    "same": ("same", {}, 92 * 5 + 12, 6),
    "rtty": ("rtty", {}, 1056 * 3 + 8, 4),
    "300-bw2": ("300", {"band_width": 2.0}, 160 * 3 + 4, 3),
}
SHAPES = {"1200": (240, 121, 40), "1200-24k": (120, 61, 20), "12000": (240, 121, 4), "same": (92, 47, 92),
          "rtty": (4800, 2401, 1056), "300-bw2": (24000, 12001, 160)}


@pytest.mark.parametrize("name", list(MODES))
def test_band_and_magnitude_equal_the_oracles_window_by_window(gpu, name):
    M, torch, ctx = gpu
    mode, opts, width, nrows = MODES[name]
    cfg = M.rx_config(mode, **opts)
    assert (cfg.fftsize, cfg.nbands, M.carrier_window_default(cfg)) == SHAPES[name]
    x = rows_for(M, cfg, width, seed=11 + len(name), nrows=nrows)
    lens = np.full(nrows, width, np.int32)
    lens[-1] = width - 1                                    # (the last row loses its last window, if it ended there)
    r = survey(gpu, cfg, x, lens)
    n_eval, n_band = check_bands(cfg, x, lens, r)
    assert n_eval >= 2 * nrows and n_band >= nrows, (n_eval, n_band)


@pytest.fixture(scope="module")
def bell(gpu):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    return cfg, rows_for(M, cfg, 1000, seed=5, nrows=6)


@pytest.mark.parametrize("window", [1, 3, 40, 239, 240])
def test_window_lengths(gpu, bell, window):
    cfg, x = bell
    r = survey(gpu, cfg, x, None, window=window, hop=max(window, 97) if window < 40 else window)
    n_eval, _ = check_bands(cfg, x, None, r)
    assert n_eval == 6 * r["nwindows"]


@pytest.mark.parametrize("hop", [1, 7, 40, 100])
def test_hops_overlap_and_gaps(gpu, bell, hop):
    cfg, x = bell
    x = x[:3, :400] if hop == 1 else x
    r = survey(gpu, cfg, np.ascontiguousarray(x), None, window=40, hop=hop)
    n_eval, n_band = check_bands(cfg, np.ascontiguousarray(x), None, r, check_mag=hop != 1)
    assert n_eval == x.shape[0] * r["nwindows"] and n_band > 0


@pytest.mark.parametrize("first", [0, 1, 3, 39])
def test_first(gpu, bell, first):
    cfg, x = bell
    r = survey(gpu, cfg, x, None, first=first)
    assert r["nwindows"] == (1000 - first - 40) // 40 + 1
    check_bands(cfg, x, None, r)


@pytest.mark.parametrize("nstreams", [1, 3, 70])
def test_batch_sizes(gpu, nstreams):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    x = rows_for(M, cfg, 360, seed=nstreams, nrows=nstreams)
    r = survey(gpu, cfg, x, None)
    n_eval, n_band = check_bands(cfg, x, None, r, check_mag=nstreams < 70)
    assert n_eval == nstreams * 9 and n_band > 0


def test_row_lengths_nwindows_and_windows_that_do_not_fit(gpu, bell):
    M, torch, ctx = gpu
    cfg, x = bell
    first, window, hop = 3, 40, 47
    # 0, one short of a window, exactly one, the last window ending on the row's last sample (k = 5, 20), one
    # short of that, a length beyond the stride (clamped)
    lens = np.array([0, first + window - 1, first + window, first + 5 * hop + window, first + 5 * hop + window - 1,
                     5000], np.int32)
    fits = M.carrier_windows(1000, window, hop, first)
    assert fits == 21 and first + 20 * hop + window < 1000
    for nwindows in (fits + 6, fits, 4, 1):                 # room for more than fit, for all, for fewer
        r = survey(gpu, cfg, x, lens, window=window, hop=hop, first=first, nwindows=nwindows)
        n_eval, _ = check_bands(cfg, x, lens, r, check_mag=nwindows == fits)
        assert n_eval == sum(min(nwindows, M.carrier_windows(min(int(n), 1000), window, hop, first)) for n in lens)
    # first beyond every row; a window that does not fit the rows at all
    r = survey(gpu, cfg, x, lens, first=10 ** 12, nwindows=3)
    assert (r["band"] == NO_WINDOW).all() and (r["mag"] == 0).all() and (r["spectrum"] == MAG_GUARD).all()
    r = survey(gpu, cfg, x[:, :200].copy(), None, window=240, nwindows=2)
    assert (r["band"] == NO_WINDOW).all() and (r["mag"] == 0).all()


@pytest.mark.parametrize("threshold", [0.0, 0.001, 0.5, 1e9])
def test_thresholds(gpu, bell, threshold):
    cfg, x = bell
    r = survey(gpu, cfg, x, None, threshold=threshold)
    n_eval, n_band = check_bands(cfg, x, None, r)
    if threshold == 1e9:
        # (the row with an Inf sample has windows whose magnitudes are infinite: those pass any threshold)
        finite = np.isfinite(r["spectrum"]).all(axis=2)
        assert (r["band"][finite] == NONE).all() and (r["mag"][finite] == 0).all() and finite.sum() >= 5 * 25 - 2


def test_without_the_spectrum_band_and_magnitude_are_unchanged(gpu, bell):
    cfg, x = bell
    a = survey(gpu, cfg, x, None, spectrum=True)
    b = survey(gpu, cfg, x, None, spectrum=False)
    assert np.array_equal(a["band"], b["band"]) and same_f32(a["mag"], b["mag"])


# ---------------------------------------------------------------------------
# the spectrum, against a restatement made with the C library
# ---------------------------------------------------------------------------
def libm_spectrum(cfg, win):
    """every band's magnitude of one window: sincos() per table entry (one call gives both, as the
    oracle's table is compiled), fma() chains in index order, hypotf() times the float scalar"""
    libm = C.CDLL("libm.so.6")
    libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    libm.sincos.restype = None
    libm.fma.argtypes = [C.c_double] * 3
    libm.fma.restype = C.c_double
    libm.hypotf.argtypes = [C.c_float] * 2
    libm.hypotf.restype = C.c_float
    N = int(cfg.fftsize)
    key = ("cs", N)
    if key not in _PLANS:
        tab = []
        sn, cs = C.c_double(0), C.c_double(0)
        for k in range(N):
            libm.sincos(2.0 * np.pi * float(k) / float(N), C.byref(sn), C.byref(cs))
            tab.append((cs.value, -sn.value))
        _PLANS[key] = tab
    tab = _PLANS[key]
    scalar = F32(1.0) / (F32(len(win)) / F32(2.0))
    out = np.zeros(int(cfg.nbands), F32)
    xs = [float(v) for v in win]                            # (double)x[n]
    for b in range(int(cfg.nbands)):
        re = im = 0.0
        for n, xv in enumerate(xs):
            c, s = tab[(b * n) % N]
            re = libm.fma(xv, c, re)
            im = libm.fma(xv, s, im)
        out[b] = F32(libm.hypotf(F32(re), F32(im))) * scalar
    return out


@pytest.mark.parametrize("mode,nwin", [("1200", 30), ("12000", 48)])
def test_every_band_of_the_spectrum_equals_a_restatement_with_the_c_library(gpu, mode, nwin):
    M, torch, ctx = gpu
    cfg = M.rx_config(mode)
    window = M.carrier_window_default(cfg)
    x = rows_for(M, cfg, window * (nwin // 6), seed=3, nrows=6)
    x[3] = np.where(np.isfinite(x[3]), x[3], F32(0.25))     # (finite values: hypotf(inf, nan) is C's own rule)
    r = survey(gpu, cfg, x, None)
    assert r["nwindows"] == nwin // 6
    for s in range(6):
        for w in range(r["nwindows"]):
            ref = libm_spectrum(cfg, x[s, w * window:(w + 1) * window])
            assert same_f32(r["spectrum"][s, w], ref), (s, w, np.flatnonzero(r["spectrum"][s, w] != ref)[:8])


# ---------------------------------------------------------------------------
# PCM16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rxnoise", [0.0, 0.25])
def test_pcm16_rows_give_what_ingest_and_the_float_call_give(gpu, rxnoise):
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    xf = rows_for(M, cfg, 1000, seed=8, nrows=5)
    xf[3] = np.where(np.isfinite(xf[3]), xf[3], F32(0.5))
    pcm = np.zeros((5, 1008), np.int16)                     # a stride that is a multiple of 8
    pcm[:, :1000] = np.clip(np.round(xf * 32767.0), -32768, 32767).astype(np.int16)
    pcm[4, :1000] = np.random.default_rng(2).integers(-32768, 32768, 1000, dtype=np.int16)
    lens = np.array([1000, 333, 1008, 41, 999], np.int32)
    d = torch.from_numpy(pcm).cuda()
    dl = torch.from_numpy(lens).cuda()
    f = M.ingest_s16(ctx, d, nsamples=dl, rxnoise=rxnoise, stride=1008)
    torch.cuda.synchronize()
    for first, hop in ((1, 40), (7, 13)):                   # odd starts
        a = survey(gpu, cfg, d, lens, first=first, hop=hop, rxnoise=rxnoise)
        b = survey(gpu, cfg, f, lens, first=first, hop=hop)
        assert np.array_equal(a["band"], b["band"]) and same_f32(a["mag"], b["mag"])
        assert same_f32(a["spectrum"], b["spectrum"])
        assert (a["band"] >= 0).sum() > 20 and (a["band"] == NO_WINDOW).sum() > 20
    check_bands(cfg, f.cpu().numpy(), lens, b, check_mag=False)


# ---------------------------------------------------------------------------
# it is the detection the receive loop makes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mark,space", [(1600, 2600), (2000, 2800), (1000, 1800)])
def test_the_survey_finds_the_band_the_receive_loop_tunes_to(gpu, mark, space):
    """Bell 202 moved to other bands, behind 0, 40, 400 and 1960 samples of silence (whole 40-sample
    windows, inside the loop's first refill: its scan windows are the survey's).  The loop drops a
    detection whose space band falls outside the plan and scans on (minimodem.c:1207-1213), which is
    what carrier_tones reports as IndexError.  The reference's shift for "1200" is +4 bands (800 Hz):
    the pair it tunes to is the pair the stream was made with where that pair is 800 Hz apart; a
    1600 / 2600 pair is tuned to 1600 / 2400, the oracle's receive loop says the same, and the stream
    decodes with it all the same."""
    M, torch, ctx = gpu
    cfg = M.rx_config("1200")
    auto = M.rx_config("1200", auto_carrier_threshold=0.001)
    oauto = O.oracle_config("1200", auto_carrier_threshold=0.001)
    txcfg = M.rx_config("1200", mark_f=float(mark), space_f=float(space))
    payload = b"carrier survey"
    sig = M.synthesize(txcfg, payload, amplitude=0.7)
    silences = (0, 40, 400, 1960)
    width = (1960 + len(sig) + 4000 + 7) & ~7
    x = np.zeros((len(silences), width), F32)
    for i, lead in enumerate(silences):
        x[i, lead:lead + len(sig)] = sig
    d = torch.from_numpy(x).cuda()
    out = M.demod_batch(ctx, auto, d, want=("bytes", "carrier_band"), force_engine=True)
    torch.cuda.synchronize()
    loop = M.results_to_host(out)
    r = survey(gpu, cfg, d, None, window=40, hop=40, threshold=0.001, spectrum=False)
    for i, lead in enumerate(silences):
        found = None
        for w in range(r["nwindows"]):
            band = int(r["band"][i, w])
            if band < 0:
                continue
            try:
                found = (w, band, M.carrier_tones(cfg, band))
                break
            except IndexError:
                continue
        assert found is not None, i
        w, band, tones = found
        assert band == int(loop["carrier_band"][i]), (i, band, loop["carrier_band"][i])
        assert w * 40 >= lead - 39 and band == mark // 200
        ref = O.oracle_rx_stream(oauto, x[i])
        assert (tones["b_mark"], tones["b_space"]) == (ref["carrier_band"], ref["carrier_b_space"])
        assert tones["mark_f"] == float(mark)
        if space - mark == 800:
            assert tones["space_f"] == float(space)
        tuned = M.rx_config("1200", mark_f=tones["mark_f"], space_f=tones["space_f"])
        dec = M.demod_batch(ctx, tuned, d[i:i + 1], want=("bytes",))
        torch.cuda.synchronize()
        dec = M.results_to_host(dec)
        assert dec["bytes"][0, :int(dec["nbytes"][0])].tobytes() == payload, (i, tones)


# ---------------------------------------------------------------------------
# the caller's stream
# ---------------------------------------------------------------------------
def test_a_stream_of_the_callers_and_two_configurations_back_to_back(gpu, bell):
    M, torch, ctx = gpu
    cfg, x = bell
    cfg2 = M.rx_config("12000")
    alone1 = survey(gpu, cfg, x, None)
    alone2 = survey(gpu, cfg2, x, None, window=4, hop=52)
    st = torch.cuda.Stream()
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    on_stream = survey(gpu, cfg, d, None, stream=st)
    assert np.array_equal(on_stream["band"], alone1["band"]) and same_f32(on_stream["mag"], alone1["mag"])
    assert same_f32(on_stream["spectrum"], alone1["spectrum"])
    # two calls with different configurations back to back on one context and one stream, read after one
    # synchronise
    with torch.cuda.stream(st):
        o1 = M.carrier_survey(ctx, cfg, d, spectrum=True, stream=st)
        o2 = M.carrier_survey(ctx, cfg2, d, window=4, hop=52, spectrum=True, stream=st)
    st.synchronize()
    assert np.array_equal(o1["band"].cpu().numpy(), alone1["band"]) and same_f32(o1["mag"].cpu().numpy(), alone1["mag"])
    assert np.array_equal(o2["band"].cpu().numpy(), alone2["band"]) and same_f32(o2["mag"].cpu().numpy(), alone2["mag"])
    assert same_f32(o1["spectrum"].cpu().numpy(), alone1["spectrum"])
    assert same_f32(o2["spectrum"].cpu().numpy(), alone2["spectrum"])
