/* mifsk/mux_stream.h -- extension of include/mifsk.h: the multiplexer fed in pieces.  It adds six
 * functions, one opaque type and one flag to the library and nothing else: no struct, no change of
 * MIFSK_ABI_VERSION; everything mifsk.h and the other extension headers declare stays where it is.
 *
 * mifsk_multiplex_batch and mifsk_multiplex_iq_batch (mifsk/mux_iq.h) know whole rows.  Rows that arrive
 * in pieces cannot be cut by their caller: an output n = m L + phi reads the samples m, m - 1, ...,
 * m - ceil(T / L) + 1, so the first outputs of a piece need the last ceil(T / L) - 1 samples of the piece
 * before, and the rotation p = (dq (n mod P)) mod P uses the absolute output index n, which the entries
 * count from 0.  A multiplexer stream keeps both, on the device: the concatenated outputs of its feeds are
 * the batch entry's outputs on the concatenated rows, bit for bit.  It is the mirror of
 * mifsk/channel_stream.h on the transmit side.
 *
 *   Definition.  A multiplexer stream belongs to a mifsk_mux_plan (T = ntaps, L = interp, K = nchannels,
 * P = phase_steps, G, W, the gains, the centres q and in_centre r are the plan's), a number of streams and
 * an input kind: rows of floats, or with MIFSK_MUX_STREAM_IQ rows of (I, Q) float pairs as
 * mifsk_multiplex_iq_batch takes them.  The kind is given at creation, not per feed: it fixes the size of
 * a tail element (4 or 8 bytes).  With H = ceil(T / L) - 1, per stream s the object holds in device memory
 *   seen[s]   a uint64_t: the input samples taken so far;
 *   first[s]  a uint64_t: the absolute sample index in front of which samples do not exist;
 *   a tail    per row s K + k: the row's last H samples as they came, float or float pair; its room is H
 *             elements rounded up to whole 16-byte vectors, one vector at least.
 * seen and first are 0 after create and n0 after a seek to n0; tails and records are zeroed at create.  A
 * tail sample whose absolute index is below first is never read as a sample: the index compare excludes
 * it, not what the memory holds.
 *   A feed reads the row lengths as the batch entry does, N_k = min(nsamples[s K + k], stream_stride)
 * (nsamples[.]: d_nsamples[.], or nsamples without d_nsamples).  The stream advances by k_s = max_k N_k,
 * the batch entry's Nmax.  A row whose piece is shorter than k_s is continued with +0.0 samples up to k_s;
 * a channel that has ended is fed length 0 from then on.  The feed delivers exactly k_s L outputs: the
 * absolute outputs n in [seen L, (seen + k_s) L), at elements n - seen L of output row s.  Each is what
 * mifsk_multiplex_batch (with MIFSK_MUX_STREAM_IQ: mifsk_multiplex_iq_batch) defines for output n of the
 * rows so far: the same tables, every scalar widened to double, the re / im chains from 0.0 in tap order,
 * the gain step, the o / oi chains in channel order, the PCM16 write conversion.  A term whose sample
 * index i is below first is skipped, not multiplied by zero.  p = (((q[k] - r) mod P) (n mod P)) mod P
 * comes from the absolute n in 64-bit integers: n mod P is ((seen mod P) (L mod P) + the feed's own
 * output index) mod P, every factor reduced first.  The feed then writes d_nout[s] = k_s L, zeros behind
 * the count up to out_stride, the new tails, and seen += k_s.  k_s = 0 leaves a stream as it was and
 * delivers nothing.
 *
 *   What follows.  (1) With first = 0, and in every feed all K rows of a stream equally long, the
 * concatenated outputs of the feeds equal the batch entry's row on the concatenated inputs on elements
 * [0, N L), N the rows' length, bit for bit, whatever taps, gains and samples hold: NaN, +-Inf, -0.0,
 * subnormals.  No term beyond a row's end is read there.  (2) With finite taps and gains, feeding H more
 * samples of +0.0 behind the last piece (mifsk_mux_stream_drain) delivers elements [N L, (N + H) L) of
 * the batch row: below the batch's count (N - 1) L + T the filter's tail, behind it the zero fill;
 * fma(+0.0, g, re) = re for finite g, and re is never -0.0 on a chain that starts from +0.0.  (3) With
 * finite taps and gains, rows that end at different lengths give the batch's outputs too.  (4) With
 * non-finite taps or gains the drain and the ragged case differ from the batch, which skips the terms
 * beyond a row's end where the stream multiplies by +0.0: 0 Inf is NaN.  That is why there is no FINAL
 * flag: the object does not claim to know where a row ends.
 *
 *   Capacity.  The host knows kmax >= k_s: min(nsamples, stream_stride) without d_nsamples,
 * stream_stride with it.  An out_stride or a nout_cap below kmax L, computed in 64 bits, is refused: a
 * cap that dropped an output would break the continuation.
 *
 *   mifsk_mux_stream_create allocates the records and tails of `nstreams` streams on the plan's device,
 * zeroed.  -EINVAL for a NULL plan or out, nstreams <= 0, or a flag bit other than MIFSK_MUX_STREAM_IQ;
 * -ENOMEM; -EIO.  The object must be destroyed before its plan.  mifsk_mux_stream_destroy synchronises
 * the device before it frees, as mifsk_mux_plan_destroy does; NULL is allowed.
 *
 *   mifsk_mux_stream_feed takes mifsk_mux_io as the batch entries do; with MIFSK_MUX_STREAM_IQ d_samples
 * points at (I, Q) pairs and stream_stride, nsamples and d_nsamples count pairs.  It checks, in this order
 * and before any HIP call: -EINVAL for a NULL object or io; then everything the batch entry of the
 * object's input kind checks of the io, in its order (NULL d_samples, d_out or d_nout; nstreams <= 0; an
 * input base that is not 16-byte aligned or a stream_stride that is not a whole number of 16-byte vectors;
 * what the entry refuses of d_out and out_stride for the plan's kind; nout_cap > out_stride; nstreams *
 * nchannels above 2^31 - 1); nstreams other than the object's; out_stride below kmax L; nout_cap below
 * it.  A refused feed changes nothing.  Asynchronous on `stream`; it allocates nothing and synchronises
 * nothing.  Feeds of one object are ordered by the caller: the same HIP stream, or events; so are a feed
 * and the seek or seen that follows it on another stream.  Whatever the arguments hold, nothing is read
 * outside nstreams * nchannels * stream_stride input elements and the object's own memory, and nothing is
 * written outside the two output arrays and the object.  No launch reads what it writes: records and
 * tails are kept twice, a feed reads one side and writes the other.  The outputs are plain vector stores.
 *
 *   mifsk_mux_stream_seek sets seen[s] and first[s] from a host array of nstreams values, each 2^46 at
 * most (-EINVAL beyond: seen L stays below 2^62 for any L <= 65535); NULL means all 0, which is the
 * reset.  After a seek to n0 the next feed delivers the outputs from n0 L on, with no sample in front of
 * n0.  It is there so that a capture can be joined in mid flight.  It waits for `stream` and blocks.
 * mifsk_mux_stream_seen copies the counters to seen_out[nstreams]; it waits for `stream` and blocks.
 *
 *   mifsk_mux_stream_drain is host only: H = ceil(ntaps / interp) - 1; 0 for interp == 0.
 *
 *   tools/mux_ref.c (mux_ref_stream, mux_ref_stream_iq) restates the outputs of one feed for the host; the
 * device's output equals it bit for bit. */
#ifndef MIFSK_MUX_STREAM_H
#define MIFSK_MUX_STREAM_H

#include "../mifsk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mifsk_mux_stream mifsk_mux_stream;

#define MIFSK_MUX_STREAM_IQ 1u

int  mifsk_mux_stream_create ( const mifsk_mux_plan *plan, int nstreams, uint32_t flags, mifsk_mux_stream **out );
void mifsk_mux_stream_destroy( mifsk_mux_stream *ms );
int  mifsk_mux_stream_feed   ( mifsk_mux_stream *ms, const mifsk_mux_io *io, void *stream );
int  mifsk_mux_stream_seek   ( mifsk_mux_stream *ms, const uint64_t *seen, void *stream );
int  mifsk_mux_stream_seen   ( mifsk_mux_stream *ms, uint64_t *seen_out, void *stream );
uint32_t mifsk_mux_stream_drain( uint32_t ntaps, uint32_t interp );

#ifdef __cplusplus
}
#endif

#endif
