"""mifsk_fm_squelch_batch (include/mifsk/squelch.h, minimodem_amd/csrc/mifsk_squelch.hip) against the host
restatement tools/squelch_ref.c: every energy, gate, span, count, state record and audio sample of every case
bit for bit.  Rows are a few thousand samples (one case of 65 537 rows of 4, one row of 65 rounds of windows);
every array a call reads or writes lies inside a larger pool whose cells around it the call must leave alone,
and every output is filled beforehand with what the restatement's arrays hold where nothing is written."""
import ctypes as C

import numpy as np
import pytest

import _fm as Fm
import _impair as Im
import _oracle as O
import _squelch as Sq
from _squelch import F32, STATE, TILE, same_bits

pytestmark = pytest.mark.gpu

GUARD = 512                         # cells either side: the rows stay 16-byte aligned
GUARDS = {np.dtype(np.float32): F32(7.25), np.dtype(np.int16): np.int16(12345), np.dtype(np.int64): np.int64(-77),
          np.dtype(np.int32): np.int32(-99), np.dtype(np.uint8): np.uint8(0xA5)}
KINDS = pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
NAN = np.uint32(0x7FC12345).view(F32)           # a NaN with a payload


@pytest.fixture(scope="module")
def gpu():
    import torch
    import minimodem_amd as M
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    ctx = M.Context()
    yield M, torch, ctx
    ctx.close()


def _pool(torch, shape, dtype, fill):
    """an array of `shape` inside a pool of guard cells -> (pool, the array's view); fill: an array or one value"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    pool = torch.full((n + 2 * GUARD,), GUARDS[dtype].item(), dtype=getattr(torch, dtype.name), device="cuda")
    view = pool[GUARD:GUARD + n].view(*shape)
    if np.ndim(fill) == 0:
        view.fill_(fill)
    else:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype)).cuda())
    return pool, view


def _inside(pool, shape):
    """the array inside the pool as numpy, the guard cells checked"""
    host = pool.cpu().numpy()
    guard = GUARDS[host.dtype]
    assert np.all(host[:GUARD] == guard) and np.all(host[-GUARD:] == guard), "the guard cells were written"
    return host[GUARD:-GUARD].reshape(shape)


def squelch(gpu, iq, window, open_level, close_level=None, hang=0, lens=None, nsamples=None, state=None, audio=None,
            span_cap=8, win_stride=None, want=("energy", "gate", "spans", "state"), in_place=False):
    """One call of the entry between guard cells, through the io struct -> what _squelch.ref_squelch returns"""
    M, torch, ctx = gpu
    rows, stride = iq.shape[:2]
    nsamples = stride if nsamples is None else nsamples
    kmax = stride if lens is not None else min(nsamples, stride)
    win_stride = Sq.win_stride_of(kmax, window) if win_stride is None else win_stride
    i64 = lambda a: np.asarray(a).view(np.int64)                    # noqa: E731
    pin, d_iq = _pool(torch, iq.shape, iq.dtype, iq)
    pools = {"energy": _pool(torch, (rows, win_stride), np.int64, Sq.FILL64), "gate": _pool(torch, (rows, win_stride), np.uint8, Sq.FILL8),
             "nwindows": _pool(torch, (rows,), np.int32, Sq.FILL32), "spans": _pool(torch, (rows, span_cap, 2), np.int64, Sq.FILL64),
             "nspans": _pool(torch, (rows,), np.int32, Sq.FILL32), "state": _pool(torch, (rows, 4), np.int64, 0)}
    if state is not None:
        state = np.ascontiguousarray(state, STATE)
        pools["state_in"] = _pool(torch, (rows, 4), np.int64, i64(state).reshape(rows, 4))
    if in_place:
        pools["state"] = pools["state_in"]
    if audio is not None:
        pools["audio"] = _pool(torch, audio.shape, np.float32, audio)
    d_lens = None if lens is None else torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    ptr = lambda name: pools[name][1].data_ptr() if name in want or name in ("nwindows", "audio", "state_in") else None   # noqa: E731
    io = M.FmSquelchIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = d_iq.data_ptr(), stride, nsamples, rows
    io.d_nsamples = None if d_lens is None else d_lens.data_ptr()
    io.kind, io.window, io.hang = int(iq.dtype == np.int16), window, hang
    io.open_level, io.close_level = open_level, open_level if close_level is None else close_level
    io.d_state, io.d_state_out = (None if state is None else ptr("state_in")), ptr("state")
    io.d_energy, io.d_gate, io.win_stride, io.d_nwindows = ptr("energy"), ptr("gate"), win_stride, ptr("nwindows")
    io.d_spans, io.span_cap = ptr("spans"), span_cap
    io.d_nspans = pools["nspans"][1].data_ptr() if "spans" in want or "nspans" in want else None
    if audio is not None:
        io.d_audio, io.audio_stride = ptr("audio"), audio.shape[1]
    torch.cuda.synchronize()
    M._call("mifsk_fm_squelch_batch", ctx.handle, C.byref(io), stream=None)
    torch.cuda.synchronize()
    assert same_bits(_inside(pin, iq.shape), iq), "the input rows were written"
    if state is not None and not in_place:
        assert _inside(pools["state_in"][0], (rows, 4)).tobytes() == state.tobytes(), "d_state was written"
    got = {name: _inside(pool, tuple(view.shape)) for name, (pool, view) in pools.items() if name != "state_in"}
    got["energy"], got["spans"] = got["energy"].view(np.uint64), got["spans"].view(np.uint64)
    got["nwindows"], got["nspans"] = got["nwindows"].view(np.uint32), got["nspans"].view(np.uint32)
    got["state"] = np.ascontiguousarray(got["state"]).view(STATE).reshape(rows)
    return got


def assert_same(name, got, want):
    if got.dtype == STATE:
        got, want = got.view(np.uint64).reshape(-1, 4), want.view(np.uint64).reshape(-1, 4)
    if not same_bits(got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        diff = got != want
        if got.dtype.kind == "f":
            diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
        bad = np.argwhere(diff)
        raise AssertionError("%s: %d elements differ, first at %s: %r != %r" % (
            name, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def check(gpu, iq, window, open_level, close_level=None, want=("energy", "gate", "spans", "state"), in_place=False, **kw):
    """the device's call == the restatement's, array by array, the cells that neither writes included"""
    got = squelch(gpu, iq, window, open_level, close_level, want=want, in_place=in_place, **kw)
    ref = Sq.ref_squelch(iq, kw.pop("lens", None), window, open_level, close_level, want=want, **kw)
    for name in ("nwindows", "energy", "gate", "nspans", "spans", "state"):
        assert_same(name, got[name], ref[name])
    if ref["audio"] is not None:
        assert_same("audio", got["audio"], ref["audio"])
    return got


def envelope_rows(rng, rows, stride, s16):
    """noise whose level steps between 0.3 and 1.3 every few hundred samples, each row at a level of its own"""
    env = np.repeat(rng.choice([0.3, 1.3], (rows, stride // 150 + 1)), 150, axis=1)[:, :stride]
    x = rng.standard_normal((rows, stride, 2)) * 0.5 * env[:, :, None] * rng.uniform(0.85, 1.15, (rows, 1, 1))
    return np.clip(np.round(x * 8192), -32768, 32767).astype(np.int16) if s16 else x.astype(F32)


def random_state(rng, rows, window, hang):
    """records in mid flight: `seen` no multiple of 4, of the window or of the tile (but for a few rows), an energy
    so far, a gate either way with a run of low windows inside the hang time"""
    state = np.zeros(rows, STATE)
    state["seen"] = rng.integers(0, 1 << 40, rows) * 2 + 1
    state["seen"][::5] = rng.integers(0, 1 << 20, len(state["seen"][::5])) * window     # on the grid
    state["acc"] = rng.integers(0, 1 << 40, rows) * (state["seen"] % window != 0)
    state["span_first"] = rng.integers(0, 1 << 50, rows)
    state["open"] = rng.integers(0, 2, rows)
    state["low"] = rng.integers(0, hang + 1, rows) * state["open"]
    return state


def levels(window, s16):
    """around the rows' mean energy, so that windows fall on either side"""
    mean = 0.5 * 0.9 * (1.0 / 16.0 if s16 else 1.0) * window * 2.0 ** 40     # 2 (0.5 env)^2; PCM16 at a quarter of the amplitude
    return int(mean * 1.2), int(mean * 0.8)


# ---------------------------------------------------------------------------
# row lengths and windows
# ---------------------------------------------------------------------------
WINDOWS = (1, 3, 4, 5, 96, TILE, TILE + 4, 32768)
STRIDE = 5 * TILE + 4


@KINDS
@pytest.mark.parametrize("window", WINDOWS)
def test_rows_of_every_length(gpu, s16, window):
    """rows that end inside a thread, a wave, a tile and behind five tiles in one call, per-row lengths (one above
    the stride), states in mid flight so that windows cross thread, wave, tile and call edges, the audio muted"""
    rng = np.random.default_rng(1000 + window + s16)
    B = window
    lens = [0, 1, 2, 3, 4, 5, B - 1, B, B + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 5 * TILE + 1, 777, STRIDE]
    rows = len(lens)
    iq = envelope_rows(rng, rows, STRIDE, s16)
    state = random_state(rng, rows, B, 1)
    if B == 32768:                                              # rows shorter than a window: some complete one
        state["seen"][9:] += np.uint64(B - 1) - (state["seen"][9:] + np.uint64(1500)) % np.uint64(B)
    audio = rng.standard_normal((rows, STRIDE + 4)).astype(F32)
    audio[:, ::97] = NAN
    open_level, close_level = levels(B, s16)
    got = check(gpu, iq, B, open_level, close_level, hang=1, lens=lens, state=state, audio=audio, span_cap=3)
    for s, ln in enumerate(lens):
        assert same_bits(got["audio"][s, min(ln, STRIDE):], audio[s, min(ln, STRIDE):]), s      # behind W: untouched
    assert got["nwindows"].max() > 0 and (B > 96 or (0 < got["gate"][13, :got["nwindows"][13]].mean() < 1))
    # uniform lengths: above the stride and below it; no state; no muting
    check(gpu, iq, B, open_level, close_level, hang=0, nsamples=1 << 20)
    got = check(gpu, iq, B, open_level, close_level, hang=3, nsamples=TILE + 9, state=state)
    assert (got["state"]["seen"] == state["seen"] + TILE + 9).all()


def test_input_strides_of_an_odd_number_of_vectors(gpu):
    """float32 rows 2 (mod 4) elements apart, whose last thread loads one vector of its four; an audio stride that
    is no multiple of 4: scalar stores"""
    rng = np.random.default_rng(5)
    iq = envelope_rows(rng, 3, TILE + 6, False)
    audio = rng.standard_normal((3, TILE + 7)).astype(F32)
    open_level, close_level = levels(5, False)
    check(gpu, iq, 5, open_level, close_level, hang=1, audio=audio, state=random_state(rng, 3, 5, 1))
    check(gpu, iq[:, :2].copy(), 1, open_level, audio=audio[:, :2].copy())
    check(gpu, envelope_rows(rng, 2, 4, True), 3, open_level, lens=[3, 1])


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("window", [4, 96])
def test_samples_are_data(gpu, window):
    """NaN, Inf and 1e30 are full scale and open the gate; subnormals and zeros are nothing; a row of zeros"""
    rng = np.random.default_rng(19)
    iq = envelope_rows(rng, 6, 1200, False) * F32(0.01)
    iq[0, 5] = (np.nan, 0.25)
    iq[0, 409] = (0.5, np.inf)
    iq[1, 7] = (-np.inf, np.inf)
    iq[1, 576:768] = 1e30
    iq[2] = 0.0
    iq[3] = -0.0
    iq[4] = np.uint32(12345).view(F32)                          # subnormals
    iq[5, :, 1] = 16.0                                          # p = 256 and a little: full scale
    got = check(gpu, iq, window, Sq.FULL, Sq.FULL >> 1, hang=0)
    assert got["gate"][0, 5 // window] == 1 and got["gate"][0, 409 // window] == 1 and got["nspans"][0] == 2
    assert got["energy"][1, 600 // window] == window * Sq.FULL and got["nspans"][1] == 2
    assert not got["energy"][2:5, :1200 // window].any() and not got["gate"][2:5, :1200 // window].any()
    assert (got["energy"][5, :1200 // window] == window * Sq.FULL).all() and got["spans"][5, 0].tolist() == [0, 1200 // window]
    check(gpu, iq, window, 1, 0, hang=2)                        # levels that everything but nothing reaches
    check(gpu, iq, window, (1 << 64) - 1, 0, hang=1 << 31)      # ... and that nothing reaches


# ---------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------
def test_a_row_of_more_windows_than_a_wave_takes_at_once(gpu):
    """65 x 64 + 1 windows of 4 elements: the gate launch's second round and its last, with one window; spans that
    cross the rounds"""
    rng = np.random.default_rng(31)
    n = (65 * 64 + 1) * 4
    iq = envelope_rows(rng, 2, n + 2, False)
    open_level, close_level = levels(4, False)
    got = check(gpu, iq, 4, open_level, close_level, hang=3, lens=[n, 64 * 64 * 4 + 3], span_cap=400)
    assert got["nwindows"].tolist() == [65 * 64 + 1, 64 * 64] and got["nspans"][0] > 20
    assert got["state"]["acc"][0] == 0 and got["state"]["acc"][1] != 0
    check(gpu, iq, 4, open_level, close_level, hang=200, lens=[n, n - 1], state=random_state(rng, 2, 4, 200), span_cap=2)


def test_more_rows_than_one_launch_holds(gpu):
    """65 537 rows of 4 elements: a second block of rows in the energy and the mute launch, every row's state"""
    rng = np.random.default_rng(53)
    n = 65537
    iq = envelope_rows(rng, n, 4, False)
    lens = np.full(n, 4, np.int32)
    lens[[3, 65535]] = 2
    lens[65534] = 0
    state = random_state(rng, n, 3, 1)
    audio = rng.standard_normal((n, 4)).astype(F32)
    open_level, close_level = levels(3, False)
    got = check(gpu, iq, 3, open_level, close_level, hang=1, lens=lens, state=state, audio=audio, span_cap=2)
    assert got["nwindows"][65536] >= 1 and got["nwindows"][65534] == 0
    assert got["state"][65534].tobytes() == Sq.ref_squelch(iq[65534:65535], [0], 3, open_level, close_level, 1,
                                                          state=state[65534:65535])["state"].tobytes()


# ---------------------------------------------------------------------------
# state and spans
# ---------------------------------------------------------------------------
HANGS = [(0, False), (1, False), (3, False), (1, True)]


@KINDS
@pytest.mark.parametrize("hang,same", HANGS, ids=["hang0", "hang1", "hang3", "close==open"])
def test_state_handed_on_in_place_through_seven_pieces(gpu, s16, hang, same):
    """two rows of 3 tiles and 70 elements in seven pieces of unequal length, two of which complete no window, the
    state array read and written in place: the whole capture's energies, gates, merged spans, state and audio"""
    rng = np.random.default_rng(41 + s16 + hang)
    B, n = 96, 3 * TILE + 70
    vec = 4 if s16 else 2
    iq = envelope_rows(rng, 2, n + (-n) % vec, s16)
    audio = rng.standard_normal((2, n)).astype(F32)
    audio[:, ::61] = NAN
    open_level, close_level = levels(B, s16)
    close_level = open_level if same else close_level
    whole = Sq.ref_squelch(iq, None, B, open_level, close_level, hang, nsamples=n, audio=audio, span_cap=64)
    assert 1 <= whole["nspans"].min() and whole["nspans"].max() < 64
    cuts = [5, TILE - 5, 1, 37, TILE + 400, 50, n - (2 * TILE + 488)]
    assert sum(cuts) == n and len(cuts) == 7
    state, at, energy, gate, spans, muted = np.zeros(2, STATE), 0, [], [], ([], []), []
    for k in cuts:
        width = k + (-k) % vec
        piece = np.zeros((2, width, 2), iq.dtype)
        piece[:, :k] = iq[:, at:at + k]
        part = np.zeros((2, width), F32)
        part[:, :k] = audio[:, at:at + k]
        got = check(gpu, piece, B, open_level, close_level, hang=hang, nsamples=k, state=state, audio=part, span_cap=64,
                    in_place=True)
        for s in range(2):
            energy.append((s, got["energy"][s, :got["nwindows"][s]]))
            gate.append((s, got["gate"][s, :got["nwindows"][s]]))
            spans[s].append((got["spans"][s], int(got["nspans"][s])))
        muted.append(got["audio"][:, :k])
        state, at = got["state"], at + k
    assert any(got_k < B for got_k in cuts) and cuts[2] == 1            # (pieces that complete no window)
    for s in range(2):
        nw = int(whole["nwindows"][s])
        assert_same("energy", np.concatenate([e for r, e in energy if r == s]), whole["energy"][s, :nw])
        assert_same("gate", np.concatenate([g for r, g in gate if r == s]), whole["gate"][s, :nw])
        assert Sq.merge_spans(spans[s]) == [tuple(x) for x in whole["spans"][s, :whole["nspans"][s]].tolist()]
    assert_same("state", state, whole["state"])
    assert_same("audio", np.concatenate(muted, axis=1), whole["audio"])


def test_the_python_entry_hands_the_state_on(gpu):
    """fm_squelch(state=, audio=): pieces of a capture through the wrapper, levels in dBFS"""
    M, torch, ctx = gpu
    rng = np.random.default_rng(77)
    B, n = 96, 2 * TILE + 100
    iq = envelope_rows(rng, 3, n, False)
    audio = rng.standard_normal((3, n)).astype(F32)
    open_level, close_level = Sq.ref_level(-4.0, B), Sq.ref_level(-7.0, B)
    whole = Sq.ref_squelch(iq, None, B, open_level, close_level, 2, audio=audio)
    d_iq, d_audio = torch.from_numpy(iq).cuda(), torch.from_numpy(audio).cuda()
    state, gates = None, []
    for a, b in ((0, 600), (600, TILE + 4), (TILE + 4, n)):
        out = M.fm_squelch(ctx, d_iq[:, a:b], window=B, open_db=-4.0, close_db=-7.0, hang=2, state=state, audio=d_audio[:, a:b])
        state = out["state"]
        torch.cuda.synchronize()
        nw = out["nwindows"].cpu().numpy()
        gates.append([out["gate"][s, :nw[s]].cpu().numpy() for s in range(3)])
    for s in range(3):
        assert_same("gate", np.concatenate([g[s] for g in gates]), whole["gate"][s, :whole["nwindows"][s]])
    assert state.cpu().numpy().tobytes() == whole["state"].tobytes()
    assert_same("audio", d_audio.cpu().numpy(), whole["audio"])
    with pytest.raises(ValueError):
        M.fm_squelch(ctx, d_iq, window=40000, open_db=-4.0)
    assert M.squelch_level(-4.0, B) == open_level


def test_a_span_cap_of_one_with_three_spans_and_every_pointer_null_in_turn(gpu):
    rng = np.random.default_rng(61)
    iq = np.zeros((2, 40, 2), F32)
    iq[0, [2, 3, 8, 14, 15, 16], 0] = 1.0
    iq[1, 30:, 1] = 1.0
    got = check(gpu, iq, 1, 1 << 40, span_cap=1)
    assert got["nspans"].tolist() == [3, 1] and got["spans"][:, 0].tolist() == [[2, 4], [30, 40]]
    state = random_state(rng, 2, 1, 0)
    audio = rng.standard_normal((2, 40)).astype(F32)
    everything = ("energy", "gate", "spans", "state")
    for want in [tuple(w for w in everything if w != drop) for drop in everything] + [("nspans",), ()]:
        check(gpu, iq, 1, 1 << 40, want=want, state=state, audio=audio, span_cap=2)
    check(gpu, iq, 1, 1 << 40, want=("energy", "gate", "state"), span_cap=0)
    check(gpu, iq, 1, 1 << 40, state=state, in_place=True)
    check(gpu, iq, 1, 1 << 40, win_stride=64, span_cap=2)       # rows of outputs further apart than they need be


# ---------------------------------------------------------------------------
# end to end: transmitter -> FM modulator -> keyed carrier -> channel -> discriminator + squelch -> receiver
# ---------------------------------------------------------------------------
E2E_WINDOW, E2E_HANG, E2E_OPEN_DB, E2E_CLOSE_DB, E2E_CNR_DB = 96, 1, -6.0, -10.0, 20.0


def test_bell_202_bursts_through_a_squelched_fm_channel(gpu):
    """8 Bell-202 streams of 16 bytes, each keyed once: synthesize_batch with leading silence -> fm_modulate -> the
    I/Q set to zero in front of the burst (behind it the modulator leaves zeros) -> impair over the whole rows at a
    carrier-to-noise ratio of 20 dB -> fm_demod + fm_squelch(audio=) -> demod_batch over the whole rows.  The
    carrier is keyed within 20 samples in front of a window's edge and the data begin within 25 samples behind the
    next edge, because the gate opens one window late; window 96 (2 ms), open at -6 dBFS, close at -10 dBFS, hang 1:
    chosen on the host chain, which decodes every row down to 14 dB.  That chain runs first: one span per row that
    covers the burst to within 1 + hang windows, every byte of every message from the muted audio, and no frame
    that starts outside the span widened by a window.  Then the device's arrays equal the host's bit for bit."""
    M, torch, ctx = gpu
    rng = np.random.default_rng(81)
    cfg, ocfg = M.rx_config("1200"), O.oracle_config("1200")
    n, B, hang = 8, E2E_WINDOW, E2E_HANG
    words = rng.integers(0x20, 0x7F, size=(n, 16), dtype=np.uint8)
    edge = 3 + np.arange(n) % 3                                 # the window that the carrier fills first
    lead = ((edge + 1) * B + rng.integers(0, 25, n)).astype(np.int32)
    key_on = edge * B - rng.integers(0, 20, n)
    stride = 7600                                               # the longest row and four windows of noise behind it
    clean, lens = M.synthesize_batch(ctx, cfg, torch.from_numpy(words).cuda(), amplitude=1.0,
                                     leading_silence=torch.from_numpy(lead).cuda(), stride=stride)
    sigma, seed = M.snr_sigma(1.0, E2E_CNR_DB), 0xF00D00000000CAFE
    dev, gain = M.fm_step(3000.0, 48000.0), M.fm_gain(48000.0, 3000.0)
    open_level, close_level = M.squelch_level(E2E_OPEN_DB, B), M.squelch_level(E2E_CLOSE_DB, B)
    assert (open_level, close_level) == (Sq.ref_level(E2E_OPEN_DB, B), Sq.ref_level(E2E_CLOSE_DB, B))

    host_clean, host_lens = clean.cpu().numpy(), lens.cpu().numpy().astype(np.uint32)
    assert host_lens.max() + 4 * B <= stride and (host_lens > lead + 6000).all()
    ref_iq, _phase = Fm.ref_modulate(host_clean, host_lens, False, stride, dev)
    for i in range(n):
        ref_iq[i, :key_on[i]] = 0.0
    ref_noisy = Im.ref_impair(ref_iq.reshape(n, 2 * stride), None, False, 2 * stride, seed=seed, sigma=sigma).reshape(n, stride, 2)
    ref_audio, _last = Fm.ref_demod(ref_noisy, None, stride, gain=gain)
    ref = Sq.ref_squelch(ref_noisy, None, B, open_level, close_level, hang, audio=ref_audio)
    assert not same_bits(ref["audio"], ref_audio)
    for i in range(n):                                          # the precondition, on the host alone
        assert ref["nspans"][i] == 1, i
        first, end = (int(w) for w in ref["spans"][i, 0])
        burst = (int(key_on[i]) // B, (int(host_lens[i]) - 1) // B + 1)
        assert burst[0] <= first <= burst[0] + 1 and burst[1] <= end <= burst[1] + 1 + hang, (i, first, end, burst)
        rx = O.oracle_rx_stream(ocfg, ref["audio"][i])
        assert rx["bytes"] == words[i].tobytes(), i
        assert len(rx["frames"]) == 16 and all((first - 1) * B <= int(f["start"]) < (end + 1) * B for f in rx["frames"]), i

    iq = M.fm_modulate(ctx, clean, nsamples=lens, deviation=dev)
    for i in range(n):
        iq[i, :int(key_on[i])] = 0.0
    noisy = M.impair(ctx, iq.view(n, 2 * stride), seed=seed, sigma=sigma).view(n, stride, 2)
    audio = M.fm_demod(ctx, noisy, gain=gain)
    sq = M.fm_squelch(ctx, noisy, window=B, open_db=E2E_OPEN_DB, close_db=E2E_CLOSE_DB, hang=hang, audio=audio)
    out = M.demod_batch(ctx, cfg, audio, want=("bytes", "frames", "episodes"))
    torch.cuda.synchronize()
    assert_same("noisy", noisy.cpu().numpy(), ref_noisy)
    nw = stride // B
    assert sq["nwindows"].cpu().numpy().tolist() == [nw] * n == ref["nwindows"].tolist()
    assert_same("energy", sq["energy"].cpu().numpy().view(np.uint64)[:, :nw], ref["energy"][:, :nw])
    assert_same("gate", sq["gate"].cpu().numpy()[:, :nw], ref["gate"][:, :nw])
    assert sq["nspans"].cpu().numpy().tolist() == [1] * n
    assert_same("spans", sq["spans"].cpu().numpy().view(np.uint64)[:, :1], ref["spans"][:, :1])
    assert sq["state"].cpu().numpy().tobytes() == ref["state"].tobytes()
    assert_same("audio", audio.cpu().numpy(), ref["audio"])
    res = M.results_to_host(out)
    bad, _groups, _secs = O.oracle_batch_mismatches(ocfg, ref["audio"], None, res, threads=4)
    assert bad == []
    for i in range(n):
        assert res["bytes"][i, :int(res["nbytes"][i])].tobytes() == words[i].tobytes(), i
