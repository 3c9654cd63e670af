/* mifsk/channel_stream.h -- extension of include/mifsk.h: the channelizer fed in pieces.  It adds six
 * functions, one opaque type and one flag to the library and nothing else: no struct, no change of
 * MIFSK_ABI_VERSION; everything mifsk.h and the other extension headers declare stays where it is.
 *
 * mifsk_channelize_batch and mifsk_channelize_iq_batch know whole rows.  A capture that arrives in
 * pieces cannot be cut by their caller: a window that straddles a cut needs the last T - 1 elements of
 * the piece before, and the output rotation uses the absolute output index m, which the entries count
 * from 0.  A channel stream keeps both, on the device: the concatenated outputs of its feeds are the
 * batch entry's outputs on the concatenated capture, bit for bit, and every output is delivered by the
 * feed in which its last input element arrives.
 *
 *   Definition.  A channel stream belongs to a mifsk_channel_plan (T = ntaps, D = decim, K = nchannels,
 * P = phase_steps) and a number of streams.  With M(n) = n >= T ? (n - T) / D + 1 : 0, per stream s
 * it holds in device memory
 *   seen[s]   a uint64_t: the elements fed so far.  Outputs 0 .. M(seen) have been delivered;
 *   a tail    those of the elements it has seen that a later output can still read: elements
 *             [M(seen) D, seen) of the stream, or none when M(seen) D >= seen.  (That occurs with D > T:
 *             the elements up to M(seen) D of later pieces are then read by nobody.)  The tail never
 *             holds more than T - 1 elements (seen - M(seen) D < T: minimodem_amd/csrc/
 *             mifsk_channel_stream_check.h has the proof); its room is that, rounded up to whole 16-byte
 *             vectors.
 * A feed gives stream s the k_s = min(nsamples[s], stream_stride) new elements of row s (nsamples[s]:
 * d_nsamples[s], or nsamples without d_nsamples).  Let X be the stream's elements 0 .. seen + k_s.  For
 * every m in [M(seen), M(seen + k_s)), output m is exactly what mifsk_channelize_batch defines for
 * output m of the row X -- the same G and W, every scalar widened to double, the two (real rows) or four
 * (complex rows) fma chains from 0.0 in tap order, p = (((r - q) mod P) * ((m D) mod P)) mod P with the
 * absolute m, in 64-bit integers -- and with MIFSK_CHANNEL_STREAM_IQ exactly what
 * mifsk_channelize_iq_batch defines (mifsk/channel_iq.h).  It is written to element m - M(seen) of
 * output row s * K + k.  The feed then writes d_nout[s * K + k] = M(seen + k_s) - M(seen), zeros behind
 * the count up to out_stride, the new tail, and seen += k_s.  k_s = 0 leaves a stream as it was and
 * delivers nothing.
 *   A feed delivers at most ceil(k_s / D) outputs per row.  The host knows a bound kmax on k_s:
 * min(nsamples, stream_stride) without d_nsamples, stream_stride with it.  An out_stride or a nout_cap
 * below ceil(kmax / D) is refused: a cap that drops outputs would break the continuation.
 *
 *   mifsk_channel_stream_create allocates the counters and tails of `nstreams` streams on the plan's
 * device, zeroed.  -EINVAL for a NULL plan or out, or nstreams <= 0; -ENOMEM; -EIO.  The object must be
 * destroyed before its plan.  mifsk_channel_stream_destroy synchronises the device before it frees, as
 * mifsk_channel_plan_destroy does; NULL is allowed.
 *
 *   mifsk_channel_stream_feed takes mifsk_channel_io as the batch entries do; with
 * MIFSK_CHANNEL_STREAM_IQ d_rows points at [nstreams * nchannels][out_stride] (I, Q) pairs and
 * out_stride and nout_cap count pairs.  It checks, in this order and before any HIP call: -EINVAL for a
 * NULL object or io; then everything the batch entry of the same flag checks of the io, in its order
 * (NULL d_samples, d_rows or d_nout; nstreams <= 0; an input base that is not 16-byte aligned or a
 * stream_stride that is not a whole number of 16-byte vectors; an output base that is not 16-byte
 * aligned, out_stride == 0, out_stride % 4 != 0 (pairs: % 2) or above 2^32 - 4 (pairs: 2^31 - 2);
 * nout_cap > out_stride; nstreams * nchannels above 2^31 - 1); nstreams other than the object's; a flag
 * bit it does not know; out_stride below ceil(kmax / D); nout_cap below it.  A refused feed changes
 * nothing.  Asynchronous on `stream`; it allocates nothing and synchronises nothing.  Feeds of one
 * object are ordered by the caller: the same HIP stream, or events; so are a feed and the seek or seen
 * that follows it on another stream.  Whatever the arguments hold, nothing is read outside nstreams *
 * stream_stride input elements and the object's own memory, and nothing is written outside the two
 * output arrays and the object.  No launch reads what it writes: counters and tails are kept twice, a
 * feed reads one side and writes the other.  The outputs are plain vector stores.
 *
 *   mifsk_channel_stream_seek sets seen[s] from a host array of nstreams values, each 2^63 at most
 * (-EINVAL beyond); NULL means all 0, which is the reset.  It empties the tails: after a seek to n0 the
 * first output delivered is the first m with m D >= n0 (the outputs from M(n0) to there would read
 * elements in front of n0 and are never delivered), and a feed's count is M(seen + k_s) less that m or
 * M(seen), whichever is greater.  It is there so that a capture can be joined in mid flight.  It waits
 * for `stream` and blocks.  mifsk_channel_stream_seen copies the counters to seen_out[nstreams]; it waits
 * for `stream` and blocks.
 *
 *   mifsk_channel_stream_outputs is host only: M(seen + k) - M(seen) for T = ntaps, D = decim, in 64-bit
 * integers; 0 for ntaps == 0 or decim == 0.  A host that feeds known lengths keeps its books with it
 * and never has to read d_nout back.
 *
 *   tools/channel_ref.c (channel_ref_stream, channel_ref_stream_iq) restates the outputs of one feed
 * for the host; the device's output equals it bit for bit. */
#ifndef MIFSK_CHANNEL_STREAM_H
#define MIFSK_CHANNEL_STREAM_H

#include "../mifsk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mifsk_channel_stream mifsk_channel_stream;

#define MIFSK_CHANNEL_STREAM_IQ 1u

int  mifsk_channel_stream_create ( const mifsk_channel_plan *plan, int nstreams, mifsk_channel_stream **out );
void mifsk_channel_stream_destroy( mifsk_channel_stream *cs );
int  mifsk_channel_stream_feed   ( mifsk_channel_stream *cs, const mifsk_channel_io *io, uint32_t flags, void *stream );
int  mifsk_channel_stream_seek   ( mifsk_channel_stream *cs, const uint64_t *seen, void *stream );
int  mifsk_channel_stream_seen   ( mifsk_channel_stream *cs, uint64_t *seen_out, void *stream );
uint64_t mifsk_channel_stream_outputs( uint32_t ntaps, uint32_t decim, uint64_t seen, uint64_t k );

#ifdef __cplusplus
}
#endif

#endif
