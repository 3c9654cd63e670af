/* mifsk/squelch.h -- extension of include/mifsk.h: the FM stage's power squelch.  It adds two functions
 * and three structs to the library and nothing else: no macro, no change of MIFSK_ABI_VERSION; everything
 * mifsk.h and the other extension headers declare stays where it is.
 *
 * An FM discriminator turns an empty channel into full-scale noise.  The squelch measures the energy of the
 * I/Q rows that mifsk_fm_demod_batch reads, window by window, runs a gate with hysteresis and a hang time
 * over the windows, reports when each row was keyed, and writes zeros over the discriminator's audio where
 * the gate is closed.  Every sum is an integer, so the result does not depend on the order of the additions
 * nor on where a row was cut into pieces: a capture fed in pieces, the state handed from call to call,
 * gives the whole capture's energies, gates, spans and muted audio bit for bit.
 *
 *   Rows.  The discriminator's: interleaved I, Q, float32 (MIFSK_FEED_F32) or PCM16 (MIFSK_FEED_S16, a
 * scalar is (float)v / 32768.0f); an element is one complex sample, strides and lengths count elements.
 * W_s = min(nsamples[s], stream_stride) (nsamples[.]: d_nsamples[.], or nsamples without d_nsamples).
 *
 *   Sample energy.  An integer with 40 fractional bits.  With (a, b) = (I, Q) widened to double:
 *     p = fma(a, a, b * b)                                  one product and one fma, each rounded once
 *     e = (p < 256.0) ? (uint64_t)rint(p * 2^40) : 2^48     rint: to nearest, ties to even
 * NaN and +Inf fail the compare and count as full scale: a broken sample must open the gate and not hide.
 * For PCM16 every step is exact and e = (vi^2 + vq^2) * 2^10.
 *
 *   Windows.  They lie on the absolute element grid: element n of the stream (n = seen + the element's
 * index in the call) belongs to window n / B, B = window, 1 <= B <= 32768.  The energy of a window is the
 * sum of its B values of e, at most 2^63: it never wraps, and it is the same number in any order.
 *
 *   State.  One mifsk_fm_squelch_state per stream, 32 bytes:
 *     seen        elements taken so far
 *     acc         energy of the window that is not yet complete (its elements so far)
 *     span_first  absolute index of the window that opened the gate; meaningful while open
 *     open        the gate: 0 or 1 (anything but 0 is read as 1)
 *     low         the run of consecutive low windows while open (read as 0, and written as 0, while closed)
 * d_state is the input array, NULL for all records zero; d_state_out the output array, NULL for none.  The
 * two may be the same array: the lane that reads record s is the one that writes it.  A host that joins a
 * capture in mid flight writes `seen` itself.  All arithmetic on seen, acc and the window indices is
 * modulo 2^64.
 *
 *   What a call completes.  With r = seen mod B, the call completes nw_s = (r + W_s) / B windows, which is
 * (seen + W_s) / B - seen / B; entry j < nw_s describes absolute window seen / B + j.  Its energy E_j is the
 * sum of e over the call's elements of that window, and for j = 0 acc is added.  The new state has seen +
 * W_s, and as acc the sum of e over the call's elements behind the last completed window (plus the old acc
 * when nw_s = 0).
 *
 *   Gate.  For each window completed by the call, in index order, with energy E and absolute index w:
 *     if E >= open_level:        { if (!open) span_first = w;  open = 1;  low = 0; }
 *     else if open:
 *         if E >= close_level:   low = 0;
 *         else                   { low += 1;  if (low > hang) { open = 0;  low = 0; } }
 *     gate[w] = open
 * close_level <= open_level, hang <= 2^31.  It is written as a serial machine; every step is an integer
 * compare, so "the last window at or above open_level is behind the last window that completed a run of
 * hang + 1 low ones" is the same bits, and the device may compute either.
 *
 *   Outputs.  Every pointer but d_nwindows is optional.
 *     d_energy[s * win_stride + j] = E_j (uint64_t), d_gate[s * win_stride + j] = gate (uint8_t), j < nw_s;
 *         entries from nw_s on are not touched.
 *     d_nwindows[s] = nw_s.
 *     d_spans[s * span_cap + i] = {first_window, end_window}: the maximal runs of open windows (gate = 1)
 *         among the call's completed windows, in order; only the first span_cap are stored, and entries
 *         behind the count are not touched.  d_nspans[s] is the true count.  A run that begins with the
 *         call's first window while the state was open reports the state's span_first; every other run
 *         reports its first window.  end_window is the index behind the run's last window; for a run that
 *         is still open at the end that is seen / B + nw_s, and the run appears again, with the same
 *         first_window, in the next call that completes a window.  Consumers merge on first_window.
 *     d_state_out[s]: the new state.
 *   Capacity.  The host knows kmax >= W_s as mifsk/mux_stream.h defines it: min(nsamples, stream_stride)
 * without d_nsamples, stream_stride with it (2^32 - 1 at most).  A win_stride below kmax / B + 1, in 64-bit
 * arithmetic, is refused when d_energy or d_gate is given: a cap that dropped a window would break the
 * continuation.
 *
 *   Muting.  d_audio (float rows, audio_stride floats apart) holds what mifsk_fm_demod_batch wrote for the
 * same I/Q rows: element i is absolute sample seen + i.  The gate applied to a sample is the one a radio has
 * at that moment: the value of `open` after every window before the sample's own window -- for the call's
 * leading partial window the input state's open, for a later window w gate[w - 1].  Where that gate is 0
 * the element becomes +0.0f; every other element is left as it is, bits and NaN payloads included: the
 * launch only writes zeros and never reads the audio.  Elements from W_s on are not touched.  An
 * audio_stride below kmax is refused.  Because the gate is causal, pieces cut anywhere give the whole
 * capture's muted audio bit for bit.  The price: the squelch opens one window late -- the first window of a
 * transmission is still muted -- and `hang` windows of tail are what keep the end of one open.
 *
 *   mifsk_fm_squelch_level(dbfs, B) = rint(10^(dbfs / 10) * 2^40 * B) in double, clamped to [1, B * 2^48]:
 * the window energy of B samples of |z|^2 = 10^(dbfs / 10); 0 dBFS is |z| = 1.  B = 0 gives 0.  Host only.
 *
 *   mifsk_fm_squelch_batch checks, in this order and before any HIP call: -EINVAL for a NULL ctx, io,
 * d_samples or d_nwindows; for nstreams <= 0; for a kind that is neither MIFSK_FEED_F32 nor
 * MIFSK_FEED_S16; for flags != 0; for an input base that is not 16-byte aligned or a stream_stride that is
 * not whole 16-byte vectors of complex elements (2 of float32, 4 of PCM16); for a window outside 1 .. 32768;
 * for close_level > open_level; for hang > 2^31; for a win_stride below kmax / B + 1 while d_energy or d_gate
 * is given; for d_spans without d_nspans; with d_audio, for an audio_stride below kmax or a d_audio that is
 * not 16-byte aligned.  A refused call changes nothing.  Asynchronous on `stream`: three launches (the
 * windows' sums tile by tile, one wave per row over the windows, the zeros), none of which waits for
 * another workgroup; it synchronises nothing and allocates only stream-ordered scratch (-ENOMEM when there
 * is none).  Whatever the arguments hold, nothing is read outside nstreams * stream_stride input elements
 * and d_state, and nothing is written outside the arrays given; nothing written is read back, and the
 * outputs are plain vector stores.
 *
 *   tools/squelch_ref.c restates all of this for the host; the device's output equals it bit for bit. */
#ifndef MIFSK_SQUELCH_H
#define MIFSK_SQUELCH_H

#include "../mifsk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mifsk_fm_squelch_state {
    uint64_t		seen;		/* elements taken so far                                 */
    uint64_t		acc;		/* energy of the window that is not yet complete         */
    uint64_t		span_first;	/* the window that opened the gate; meaningful while open */
    uint32_t		open;		/* the gate                                              */
    uint32_t		low;		/* consecutive low windows while open                    */
} mifsk_fm_squelch_state;		/* 32 bytes */

typedef struct mifsk_fm_squelch_span {
    uint64_t		first_window;	/* absolute index of the run's first open window         */
    uint64_t		end_window;	/* ... behind its last one                               */
} mifsk_fm_squelch_span;		/* 16 bytes */

typedef struct mifsk_fm_squelch_io {
    const void		*d_samples;	/* nstreams rows of interleaved I, Q of `kind`           */
    size_t		stream_stride;	/* complex elements between input rows                   */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                    */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16: the input scalars    */
    uint32_t		flags;		/* 0 */
    uint32_t		window;		/* B: elements per window, 1 .. 32768                    */
    uint32_t		hang;		/* low windows that leave the gate open, 0 .. 2^31       */
    uint64_t		open_level;	/* a window energy at or above it opens the gate         */
    uint64_t		close_level;	/* ... below it counts as low; <= open_level             */
    const mifsk_fm_squelch_state *d_state;	/* [nstreams], or NULL: all zero                 */
    mifsk_fm_squelch_state *d_state_out;	/* [nstreams], or NULL; may be d_state           */
    uint64_t		*d_energy;	/* [nstreams][win_stride], or NULL                       */
    uint8_t		*d_gate;	/* [nstreams][win_stride], or NULL                       */
    size_t		win_stride;	/* entries between rows of d_energy and d_gate           */
    uint32_t		*d_nwindows;	/* [nstreams]: windows completed by the call             */
    mifsk_fm_squelch_span *d_spans;	/* [nstreams][span_cap], or NULL                         */
    uint32_t		*d_nspans;	/* [nstreams]: the true count of spans, or NULL          */
    uint32_t		span_cap;
    uint32_t		reserved;
    float		*d_audio;	/* [nstreams][audio_stride]: the discriminator's rows, or NULL */
    size_t		audio_stride;	/* floats between audio rows, kmax at least              */
} mifsk_fm_squelch_io;			/* 152 bytes */

int      mifsk_fm_squelch_batch( mifsk_ctx *ctx, const mifsk_fm_squelch_io *io, void *stream );
uint64_t mifsk_fm_squelch_level( double dbfs, uint32_t window );

#ifdef __cplusplus
}
#endif

#endif
