/* mifsk/mux_iq.h -- extension of include/mifsk.h: the multiplexer's I/Q entry.  It adds one function
 * to the library and nothing else: no struct, no macro, no change of MIFSK_ABI_VERSION; everything
 * mifsk.h declares stays where it is.
 *
 * mifsk_multiplex_iq_batch is mifsk_multiplex_batch (mifsk.h, "multiplexer") with complex rows in:
 * each input row is interleaved I, Q float32, what mifsk_fm_modulate_batch writes for float32 output
 * and what mifsk_channelize_iq_batch (mifsk/channel_iq.h) writes as d_rows.  So several FM channels
 * made at the narrow rate are put on the carriers of one wideband capture in one launch
 * (synthesize -> fm_modulate -> multiplex -> impair -> channelize -> fm_demod -> demodulate, all on
 * the device).
 *
 *   Definition.  mifsk_multiplex_batch's, word for word, with one change: G and W from the plan as
 * they are, M_s = (Nmax_s - 1) L + T in 64 bits cut at nout_cap with N_k = min(nsamples[s K + k],
 * stream_stride), a term whose sample lies outside its row skipped, the gain step,
 * p = (((q[k] - r) mod P) * (n mod P)) mod P, the o / oi chains in channel order, the PCM16 write
 * conversion, zeros from the count to out_stride and d_nout[s].  The one change is the tap step: with
 * (a, b) = (I, Q) of x_k[i], each widened to double,
 *   re = fma(a, G[t].re, re);   re = fma(-b, G[t].im, re);
 *   im = fma(a, G[t].im, im);   im = fma(b,  G[t].re, im);
 * in this order, every fma rounded once and nothing else fused: the product of the complex sample
 * and the complex table entry, as mifsk_channelize_batch forms it for complex rows.
 *
 *   Meaning.  The rows are complex envelopes whose content sits at in_centre (0 for
 * mifsk_fm_modulate_batch with centre = 0; G is then the low-pass (h, +-0)).  The filter keeps that
 * image of the zero-stuffed row and channel k is moved to centres[k].  A complex row is one-sided
 * already, so unit gain wants taps that sum to L, mifsk_channel_taps(T, fc, fs_out, L), not 2 L.
 *
 *   It takes any mifsk_mux_plan (real or complex output, float32 or PCM16) and the real entry's
 * mifsk_mux_io, with d_samples pointing at [nstreams * nchannels][stream_stride] complex elements of
 * two floats each (cast the pointer); stream_stride, nsamples and d_nsamples count complex elements.
 * PCM16 I/Q input is not taken: the plan's `kind` means the output's scalars, and
 * mifsk_mux_plan_create goes on refusing flags beyond MIFSK_MUX_COMPLEX.
 *   It checks, in the real entry's order and before any HIP call: -EINVAL for a NULL plan, io,
 * d_samples, d_out or d_nout; for nstreams <= 0; for an input base that is not 16-byte aligned or a
 * stream_stride that is not a whole number of 16-byte vectors of complex float32, that is odd; for
 * what the real entry refuses of d_out and out_stride for the plan's kind; for nout_cap > out_stride;
 * for nstreams * nchannels above 2^31 - 1.  Asynchronous on `stream`; it allocates nothing and
 * synchronises nothing.  Whatever the arguments hold, nothing outside nstreams * nchannels *
 * stream_stride complex input elements is read and nothing outside the two output arrays is
 * written.  The outputs are plain vector stores.  tools/mux_ref.c (mux_ref_iq) restates the
 * definition for the host; the device's output equals it bit for bit. */
#ifndef MIFSK_MUX_IQ_H
#define MIFSK_MUX_IQ_H

#include "../mifsk.h"

#ifdef __cplusplus
extern "C" {
#endif

int  mifsk_multiplex_iq_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream );

#ifdef __cplusplus
}
#endif

#endif
