"""ofsk_frame_confidence (oracle/fsk_oracle.c) is the tail of ofsk_frame_analyze and nothing else:
on frames cut from three goldens, ofsk_bit_analyze per bit window followed by
ofsk_frame_confidence gives ofsk_frame_analyze's confidence, amplitude and bits bit for bit --
frames rejected by a required bit included (0.0, out-params untouched).  tests/test_gpu_devmath.py
hands the function magnitudes that no recording produces."""
import ctypes as C

import numpy as np
import pytest

import _golden as G
import _oracle as O

_BITS0, _AMPL0 = 0xDEADBEEFCAFEF00D, -123.5         # what "untouched" out-params still hold


@pytest.mark.parametrize("name", ["t01_1200", "t03_rtty", "t80_same"])
def test_bit_analyze_then_frame_confidence_is_frame_analyze(name):
    g = G.load(name)
    cfg = O.oracle_config(**g["cfg_kwargs"])
    lib = O.oracle_lib()
    plan = lib.ofsk_plan_new(float(cfg.sample_rate), cfg.mark_f, cfg.space_f, cfg.band_width)
    nb, B = int(cfg.expect_n_bits), int(cfg.bit_nsamples)
    offs = [int(cfg.bit_offset[k]) for k in range(nb)]
    x = np.ascontiguousarray(np.concatenate([g["samples"], np.zeros(offs[-1] + B + 8, np.float32)]))
    # a few hundred frame starts spread over the recording, at a stride that is no multiple of
    # the bit length: every alignment of the windows to the signal's bits
    starts = np.unique(np.linspace(0, len(g["samples"]) - 1, 300).astype(np.int64)
                       + np.arange(300) % 7)
    mark, space = np.zeros(nb, np.float32), np.zeros(nb, np.float32)
    accepted = rejected = 0
    try:
        for expect in {bytes(cfg.expect_data), bytes(cfg.expect_sync)}:
            for t in starts.tolist():
                base = x.ctypes.data + 4 * t
                bits_a, ampl_a = C.c_ulonglong(_BITS0), C.c_float(_AMPL0)
                conf_a = lib.ofsk_frame_analyze(plan, base, C.c_float(cfg.find_samples_per_bit), nb,
                                                expect, C.byref(bits_a), C.byref(ampl_a))
                for k in range(nb):
                    bit, sig, noise = C.c_uint(0), C.c_float(0), C.c_float(0)
                    lib.ofsk_bit_analyze(plan, base + 4 * offs[k], B, C.byref(bit), C.byref(sig),
                                         C.byref(noise))
                    mark[k], space[k] = (sig.value, noise.value) if bit.value else (noise.value, sig.value)
                bits_c, ampl_c = C.c_ulonglong(_BITS0), C.c_float(_AMPL0)
                conf_c = lib.ofsk_frame_confidence(mark.ctypes.data, space.ctypes.data, nb, expect,
                                                   C.byref(bits_c), C.byref(ampl_c))
                got = np.array([conf_c, ampl_c.value], np.float32).view(np.uint32).tolist()
                want = np.array([conf_a, ampl_a.value], np.float32).view(np.uint32).tolist()
                assert got == want and bits_c.value == bits_a.value, (name, expect, t)
                if bits_a.value == _BITS0:
                    assert conf_a == 0.0 and ampl_a.value == _AMPL0
                    rejected += 1
                else:
                    accepted += 1
    finally:
        lib.ofsk_plan_destroy(plan)
    # both ends of the function were exercised (SAME's data string requires nothing: its
    # rejections come from the sync string alone)
    assert accepted > 50 and rejected > 50, (accepted, rejected)
