"""mifsk_detect_carrier_batch and its two host helpers (include/mifsk.h): what the entry
refuses -- before any HIP call, so every code below comes back on a machine without a device: the
context is a block of zeroed host memory and the device pointers are numbers -- and the helpers
against brute force."""
import ctypes as C

import numpy as np
import pytest

import minimodem_amd as M
from minimodem_amd import _lib

from _abi import EINVAL, ERANGE, fake_ctx, lib  # noqa: F401

F32 = np.float32


def test_the_python_names_are_public():
    for name in ("carrier_survey", "carrier_windows", "carrier_tones"):
        assert name in M.__all__ and callable(getattr(M, name)), name


def _io(**kw):
    base = 1 << 20                                  # 16-byte aligned; never dereferenced
    io = _lib.CarrierIO()
    io.d_samples, io.stream_stride, io.nsamples, io.nstreams = base, 96000, 96000, 2
    io.kind, io.rxnoise = _lib.FEED_F32, 0.0
    io.first, io.window, io.hop, io.nwindows, io.threshold = 0, 0, 0, 64, 0.001
    io.d_band, io.d_mag, io.d_spectrum = base + (1 << 24), base + (1 << 25), None
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_argument_checks_come_back_without_a_device(lib, fake_ctx):
    ctx, _keep = fake_ctx
    cfg = M.rx_config("1200")
    spec = (1 << 20) + (1 << 26)

    def rc(ctx=ctx, cfg=cfg, io=True, **kw):
        return lib.mifsk_detect_carrier_batch(ctx, C.byref(cfg) if cfg is not None else None,
                                              C.byref(_io(**kw)) if io else None, None)

    assert rc(ctx=None) == EINVAL and rc(cfg=None) == EINVAL and rc(io=False) == EINVAL
    for name in ("d_samples", "d_band"):
        assert rc(**{name: None}) == EINVAL, name
    assert rc(nstreams=0) == EINVAL and rc(nstreams=-2) == EINVAL
    assert rc(nwindows=0) == EINVAL
    assert rc(kind=2) == EINVAL and rc(kind=0xFFFFFFFF) == EINVAL
    assert rc(rxnoise=0.1) == EINVAL                                # float32 rows take no --Xrxnoise term
    assert rc(rxnoise=float("nan")) == EINVAL
    # 16-byte rows: the base, and a stride of whole vectors -- 4 floats, 8 PCM16 samples
    assert rc(d_samples=(1 << 20) + 8) == EINVAL and rc(d_samples=(1 << 20) + 4) == EINVAL
    assert rc(stream_stride=96002) == EINVAL and rc(stream_stride=95999) == EINVAL
    assert rc(kind=_lib.FEED_S16, stream_stride=96004) == EINVAL    # a multiple of 4, not of 8
    assert rc(kind=_lib.FEED_S16, d_samples=(1 << 20) + 8) == EINVAL
    # mifsk_check_cfg's verdict, and a plan without a band above 0
    for field, v in (("expect_n_bits", 0), ("expect_n_bits", 65), ("bit_nsamples", 0), ("fftsize", 1),
                     ("nbands", 0), ("nbands", 1)):
        bad = M.rx_config("1200")
        setattr(bad, field, v)
        assert rc(cfg=bad) == EINVAL, field
    # the window: at most fftsize (240), and the default must not be empty
    assert rc(window=241) == EINVAL and rc(window=0xFFFFFFFF) == EINVAL
    empty = M.rx_config("1200")
    empty.nsamples_per_bit = 0.5
    assert rc(cfg=empty) == EINVAL
    # b * n is reduced in 32 bits
    wide = M.rx_config("1200")
    wide.fftsize, wide.nbands = 1 << 30, 1 << 29
    assert rc(cfg=wide, window=8) == EINVAL
    # the spectrum's rows are indexed in 32 bits
    assert rc(d_spectrum=spec, nwindows=(1 << 32) // 121 + 1) == EINVAL
    # the earlier checks win over the later ones
    assert rc(window=241, ctx=None) == EINVAL
    late = dict(window=241, d_spectrum=spec, nwindows=0xFFFFFFFF)
    for early in (dict(d_band=None), dict(nstreams=0), dict(kind=7), dict(rxnoise=1.0), dict(stream_stride=96002)):
        assert rc(**dict(late, **early)) == EINVAL, early


def test_threshold_and_auto_carrier_are_not_among_the_checks(lib, fake_ctx):
    """Any threshold is accepted and cfg->auto_carrier_threshold is not looked at: with the window as
    the one violation, the call comes back with that violation's code whatever they hold."""
    ctx, _keep = fake_ctx
    cfg = M.rx_config("1200")
    for thr in (0.0, -1.0, float("inf"), float("nan"), 1e9):
        io = _io(window=241, threshold=thr)
        assert lib.mifsk_detect_carrier_batch(ctx, C.byref(cfg), C.byref(io), None) == EINVAL
    auto = M.rx_config("1200", auto_carrier_threshold=0.001)
    assert lib.mifsk_detect_carrier_batch(ctx, C.byref(auto), C.byref(_io(window=241)), None) == EINVAL


def _brute_windows(nsamples, first, window, hop):
    hop = hop or window
    n, a = 0, first
    while a + window <= nsamples:
        n += 1
        a += hop
    return n


def test_carrier_windows_against_a_brute_force_count(lib):
    for nsamples in range(0, 51):
        for first in range(0, 6):
            for window in range(1, 9):
                for hop in range(0, 10):
                    got = lib.mifsk_carrier_windows(nsamples, first, window, hop)
                    assert got == _brute_windows(nsamples, first, window, hop), (nsamples, first, window, hop)
    assert lib.mifsk_carrier_windows(3 + 7 * 40 + 40, 3, 40, 40) == 8           # an exact fit
    assert lib.mifsk_carrier_windows(3 + 7 * 40 + 39, 3, 40, 40) == 7           # one sample short
    assert lib.mifsk_carrier_windows(40, 0, 40, 0) == 1 and lib.mifsk_carrier_windows(39, 0, 40, 0) == 0
    assert lib.mifsk_carrier_windows(10, 11, 1, 1) == 0                          # first beyond the row
    assert lib.mifsk_carrier_windows((1 << 40) + 39, 0, 40, 8) == 1 << 37          # 64-bit lengths
    assert M.carrier_windows(480000, 40) == 12000 and M.carrier_windows(480000, 40, hop=8) == 59996
    assert M.carrier_windows(100, 40, hop=7, first=3) == _brute_windows(100, 3, 40, 7)


def _shift(cfg):
    """the expression of minimodem.c:1203-1206 in float32"""
    bw = F32(cfg.band_width)
    s = int(np.trunc(-(F32(cfg.autodetect_shift) + bw / F32(2.0)) / bw))
    return -s if cfg.inverted_freqs else s


def _tones(lib, cfg, band):
    bm, bs, fm, fs = C.c_uint(77), C.c_uint(77), C.c_float(-1), C.c_float(-1)
    rc = lib.mifsk_carrier_tones(C.byref(cfg), band, C.byref(bm), C.byref(bs), C.byref(fm), C.byref(fs))
    return rc, bm.value, bs.value, F32(fm.value), F32(fs.value)


def test_carrier_tones(lib):
    """Bell 202: autodetect_shift is -(1200 * 5 / 6) = -1000 (minimodem.c:904), so the reference's
    b_shift = -(float)(-1000 + 200 / 2) / 200 truncates 4.5 to +4: the space tone it tunes to lies 800 Hz
    ABOVE the mark, and a mark band above nbands - 5 is dropped; with -i the shift is -4."""
    cfg = M.rx_config("1200")
    assert cfg.autodetect_shift == -1000 and _shift(cfg) == 4 and cfg.nbands == 121
    rc, bm, bs, fm, fs = _tones(lib, cfg, 11)
    assert (rc, bm, bs) == (0, 11, 15)
    assert fm == F32(11) * F32(cfg.band_width) and fs == F32(15) * F32(cfg.band_width)
    assert _tones(lib, cfg, 1)[:3] == (0, 1, 5) and _tones(lib, cfg, 4)[:3] == (0, 4, 8)
    assert _tones(lib, cfg, 116)[:3] == (0, 116, 120)
    assert _tones(lib, cfg, 117)[0] == ERANGE and _tones(lib, cfg, 120)[0] == ERANGE
    assert _tones(lib, cfg, 117)[1:3] == (77, 77)                    # a refusal writes nothing
    assert _tones(lib, cfg, 0)[0] == EINVAL and _tones(lib, cfg, 121)[0] == EINVAL and _tones(lib, cfg, -3)[0] == EINVAL
    assert lib.mifsk_carrier_tones(None, 11, None, None, None, None) == EINVAL
    assert lib.mifsk_carrier_tones(C.byref(cfg), 11, None, None, None, None) == 0
    assert M.carrier_tones(cfg, 11) == {"b_mark": 11, "b_space": 15, "mark_f": float(fm), "space_f": float(fs)}
    with pytest.raises(IndexError):
        M.carrier_tones(cfg, 120)
    with pytest.raises(ValueError):
        M.carrier_tones(cfg, 0)

    inv = M.rx_config("1200", inverted_freqs=1)
    assert _shift(inv) == -4
    assert _tones(lib, inv, 4)[0] == ERANGE and _tones(lib, inv, 1)[0] == ERANGE
    assert _tones(lib, inv, 5)[:3] == (0, 5, 1)
    assert _tones(lib, inv, inv.nbands - 1)[:3] == (0, inv.nbands - 1, inv.nbands - 5)

    # a positive autodetect_shift gives a negative band shift: rtty (170 Hz, 10 Hz bands) -17
    assert _shift(M.rx_config("rtty")) == -17
    assert _tones(lib, M.rx_config("rtty"), 17)[0] == ERANGE and _tones(lib, M.rx_config("rtty"), 159)[:3] == (0, 159, 142)

    for mode in ("rtty", "same", "300", "12000"):
        c = M.rx_config(mode)
        sh = _shift(c)
        if sh == 0:                     # same: -(-434 + 260.4) / 520.8 truncates to 0, which the loop refuses too
            assert mode == "same" and _tones(lib, c, 4)[0] == EINVAL and _tones(lib, c, 1)[0] == EINVAL
            continue
        for band in (1, 2, abs(sh), abs(sh) + 1, c.nbands // 2, c.nbands - 1):
            rc, bm, bs, fm, fs = _tones(lib, c, band)
            space = band + sh
            if 1 <= space < c.nbands:
                assert (rc, bm, bs) == (0, band, space), (mode, band)
                assert fm == F32(band) * F32(c.band_width) and fs == F32(space) * F32(c.band_width)
            else:
                assert rc == ERANGE, (mode, band)
        assert _tones(lib, c, 0)[0] == EINVAL and _tones(lib, c, c.nbands)[0] == EINVAL

    # no shift at all: fsk_set_tones_by_bandshift asserts it
    flat = M.rx_config("1200")
    flat.autodetect_shift = 0
    flat.band_width = 100.0
    assert _shift(flat) == 0 and _tones(lib, flat, 11)[0] == EINVAL
