/* mifsk/channel_iq.h -- extension of include/mifsk.h: the channelizer's I/Q entry.  It adds one
 * function to the library and nothing else: no struct, no macro, no change of MIFSK_ABI_VERSION;
 * everything mifsk.h declares stays where it is.
 *
 * mifsk_channelize_iq_batch is mifsk_channelize_batch (mifsk.h, "channelizer") with the output kept
 * whole: each channel of each row as interleaved I, Q float32, so that the FM channels of one
 * wideband capture reach mifsk_fm_demod_batch on the device (survey -> channelize -> discriminate ->
 * demodulate).
 *
 *   Definition.  Everything up to (re, im) is mifsk_channelize_batch's, word for word: the tables G
 * and W, every scalar widened to double, the two (real rows) or four (complex rows) fma chains from
 * 0.0 in tap order, p = (((r - q) mod P) * ((m D) mod P)) mod P, (C, S) = W[p], whole windows only
 * (output m of a row of N valid elements exists when m D + T <= N: M_s of them).  Then
 *   I[m] = (float) fma(re, C, -(im * S))        exactly mifsk_channelize_batch's out[m]
 *   Q[m] = (float) fma(re, S,   im * C )
 * every product and every fma rounded once.  Element m of row s * nchannels + k of d_rows is
 * (I[m], Q[m]) of channel k of stream s.  With out_centre == 0 the row is the channel's complex
 * envelope at fs_in / D samples per second, what mifsk_fm_demod_batch takes as d_samples; any other
 * out_centre keeps its meaning, the envelope moved to r fs_in / P Hz.  NaN and Inf propagate as the
 * arithmetic says.  Elements from min(M_s, nout_cap) to out_stride are (+0.0f, +0.0f), and
 * d_nout[s * nchannels + k] = min(M_s, nout_cap), as in the real entry.
 *
 *   It takes the same plan (any kind: real or complex input, float32 or PCM16) and the same
 * mifsk_channel_io, with d_rows pointing at [nstreams * nchannels][out_stride] complex elements of
 * two floats each (cast the pointer); out_stride and nout_cap count complex elements.
 *   It checks, in this order and before any HIP call: -EINVAL for a NULL plan, io, d_samples, d_rows
 * or d_nout; for nstreams <= 0; for an input base that is not 16-byte aligned or a stream_stride
 * that is not a whole number of 16-byte vectors (4 real floats, 8 real PCM16, 2 complex floats, 4
 * complex PCM16); for an output base that is not 16-byte aligned, out_stride == 0, out_stride % 2 !=
 * 0 or out_stride above 2^31 - 2; for nout_cap > out_stride; for nstreams * nchannels above
 * 2^31 - 1.  Asynchronous on `stream`; it allocates nothing and synchronises nothing.  Whatever the
 * arguments hold, nothing outside nstreams * stream_stride input elements is read and nothing
 * outside the two output arrays is written.  The outputs are plain vector stores, one 8-byte store
 * per element.  tools/channel_ref.c (channel_ref_iq) restates the definition for the host; the
 * device's output equals it bit for bit. */
#ifndef MIFSK_CHANNEL_IQ_H
#define MIFSK_CHANNEL_IQ_H

#include "../mifsk.h"

#ifdef __cplusplus
extern "C" {
#endif

int  mifsk_channelize_iq_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream );

#ifdef __cplusplus
}
#endif

#endif
