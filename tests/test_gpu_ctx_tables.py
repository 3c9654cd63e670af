"""The collector of the context's device tables (cache_gc in minimodem_amd/csrc/mifsk_ctx.cpp) between
two uses of a configuration, on the device: ONE context decodes a 0.1 s clean stream at each of 66
distinct configurations -- 66 bit lengths of test_gpu_bitlengths.py's sweep, wavefront engine -- which
is more than the 64 the cache holds, so the collector has dropped every table by the time the
first three configurations are decoded again.  Every result equals the oracle's, frame for frame.
(tests/test_ctx_tables.py runs the same code without a device, table by table.)"""
import numpy as np
import pytest

import _oracle as O
from test_gpu_bitlengths import bit_lengths
from test_gpu_parity import assert_stream_equal, run_gpu_streams

NSAMPLES = 4800         # 0.1 s at 48 kHz
B_LO, B_HI = 24, 89     # 66 bit lengths: 5 .. 20 frames in a stream


def streams():
    """[(B, baudmode, cfg, ocfg, stream)]"""
    import minimodem_amd as M
    out = []
    for B, mode in bit_lengths("exact", B_LO, B_HI):
        cfg, ocfg = M.rx_config(mode), O.oracle_config(mode)
        rng = np.random.default_rng([41, B])
        payload = rng.integers(32, 127, size=NSAMPLES // (10 * B) + 2, dtype=np.uint8)
        x = M.synthesize(cfg, payload, leading_silence=int(rng.integers(0, 201)))
        assert len(x) >= NSAMPLES
        out.append((B, mode, cfg, ocfg, np.ascontiguousarray(x[:NSAMPLES])))
    return out


@pytest.mark.gpu
def test_a_flush_between_two_uses_of_a_configuration():
    import torch
    import minimodem_amd as M
    cases = streams()
    assert len(cases) == 66 and len({int(c[2].bit_nsamples) for c in cases}) == 66
    ctx = M.Context()
    try:
        frames = 0
        for B, mode, cfg, ocfg, x in cases + cases[:3]:
            ref = O.oracle_rx_stream(ocfg, x)
            res = run_gpu_streams(M, torch, ctx, cfg, [x], engine="wave")
            assert_stream_equal(res, 0, ref, "B=%d %s" % (B, mode))
            frames += len(ref["frames"])
        assert frames >= 3 * len(cases)         # (the oracle's own count: the streams are worth decoding)
    finally:
        ctx.close()
