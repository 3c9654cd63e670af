/*
 * include/mifsk.h -- batch C ABI of the MI355X-native FSK demodulator.
 *
 * include/fsk.h keeps the reference's five-function API.  One fsk_find_frame()
 * call covers <= ~10 kB of audio, so offloading it call by call is launch-
 * and PCIe-bound.  This header is the extension that makes the path worth
 * running on a GPU: whole streams resident in HBM, and the reference's
 * receive loop (main() in src/minimodem.c:1137-1463 -- the only caller of
 * fsk_find_frame) executed on the device, one workgroup per stream.
 *
 * Everything here is plain C: PODs, pointers and sizes.  Pointers whose name
 * starts with d_ are DEVICE pointers (hipMalloc / torch.cuda tensors); all
 * others are host pointers.  `stream` arguments are a hipStream_t passed as
 * void* (NULL = the default stream).  Functions return 0 on success or a
 * negative errno value; nothing aborts across this boundary.
 *
 *   entry point                   stands in for (reference file:line)
 *   mifsk_modem_args_default      option defaults        minimodem.c:492-553
 *   mifsk_rx_config_init          preset + derived state minimodem.c:819-965,1037-1131
 *                                 and plan bins          fsk.c:52-57
 *   mifsk_ctx_create/destroy      fsk_plan_new/destroy   fsk.c:33-104
 *   mifsk_find_frame_batch        fsk_find_frame         fsk.c:449-538 (N problems)
 *   mifsk_demod_batch             the --rx main loop     minimodem.c:1137-1463
 *   mifsk_pipeline_*              ... several batches in flight (lanes of context + stream)
 *   mifsk_gather_*                (none: one process per GPU) decoded bytes to rank 0, RCCL
 *   mifsk_demod_slab[_ring]       the loop over a stream that arrives in pieces  minimodem.c:1144-1174
 *   mifsk_session_*               ... fed from host memory, bookkeeping included
 *   mifsk_session_feed_ex/_device ... the tails kept on the device; float32, PCM16, device samples
 *   mifsk_demod_long[_batch]      the loop over one long stream, or a few, cut in time across the chip
 *   mifsk_demod_long_batch_s16    ... from PCM16 in device memory (rows gathered straight from it)
 *   mifsk_demod_long_batch_host   ... from host memory, float32 or PCM16
 *   mifsk_demod_batch_host[_ex]   same, host buffers     (chunked H2D | demod | D2H, overlapped)
 *   mifsk_demod_files             --rx --file, N files   simpleaudio-sndfile.c:42-74,
 *                                                        minimodem.c:1014-1032
 *   mifsk_demod_files_long        ... long recordings: every group cut in time across the chip
 *   mifsk_frame_softbits          fsk_bit_analyze on every bit window of the frames found  fsk.c:107-169
 *   mifsk_detect_carrier_batch    fsk_detect_carrier     fsk.c:543-581 (windows of every stream)
 *   mifsk_fm_demod_batch          (none: the FM receiver in front of the audio input) I/Q rows -> audio rows
 *   mifsk_fm_modulate_batch       (none: the FM transmitter behind the audio output)  audio rows -> I/Q rows
 */
#ifndef MIFSK_H
#define MIFSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIFSK_MAX_FRAME_BITS	64	/* fsk.c:185-187,463 */
#define MIFSK_ABI_VERSION	8

/* which databits decoder main() would have selected (minimodem.c:549-553,
 * 675,820,856,866,892).  Decoding frame bits to text is O(1)/frame host work
 * on the gathered frames; the device emits frame bits. */
enum mifsk_decoder {
    MIFSK_DECODE_ASCII8	= 0,
    MIFSK_DECODE_BAUDOT	= 1,
    MIFSK_DECODE_BINARY	= 2,
    MIFSK_DECODE_CALLERID = 3,
    MIFSK_DECODE_UIC_GROUND = 4,
    MIFSK_DECODE_UIC_TRAIN = 5
};

/* The --rx command line, as data.  Zero / negative means "not given".
 * confidence_threshold, search_limit: the reference takes a negative -c or -l
 * literally (below every confidence: each search result counts); passed on in
 * this struct it would silently mean 1.5 / 2.3.  A caller that parses a command
 * line refuses a negative value, as the batch program (mifsk_cli.c) does. */
typedef struct mifsk_modem_args {
    const char	*baudmode;	/* "1200" "300" "rtty" "tdd" "same" "callerid"
				   "uic-train" "uic-ground" "V.21" or a number */
    unsigned	sample_rate;	/* -R            (0 -> 48000)              */
    float	mark_f;		/* -M            (0 -> mode default)       */
    float	space_f;	/* -S            (0 -> mode default)       */
    float	band_width;	/* -b            (0 -> mode default)       */
    int		n_data_bits;	/* -8 / -7 / -5  (0 -> mode default)       */
    int		baudot;		/* -5 also selects the baudot decoder      */
    int		nstartbits;	/* --startbits   (<0 -> 1)                 */
    float	nstopbits;	/* --stopbits    (<0 -> 1.0)               */
    int		invert_start_stop;	/* --invert-start-stop             */
    int		inverted_freqs;	/* -i                                      */
    int		msb_first;	/* --msb-first                             */
    int		have_sync_byte;	/* --sync-byte given                       */
    long long	sync_byte;
    float	confidence_threshold;	/* -c (<0 -> 1.5)                  */
    float	search_limit;	/* -l            (<0 -> 2.3)               */
    int		binary_output;	/* --binary-output                         */
    int		binary_raw_nbits;	/* --binary-raw N                  */
    int		rx_one;		/* --rx-one                                */
    float	auto_carrier_threshold;	/* -a -> 0.001, -A x -> x: find the mark
					   tone per stream before the first
					   search (minimodem.c:1179-1220)  */
} mifsk_modem_args;

/* Everything main() derives before entering the receive loop, computed on the
 * host in C `float` with the reference's own expressions and truncations. */
typedef struct mifsk_rx_config {
    /* modem */
    unsigned	sample_rate;
    float	data_rate;
    float	mark_f, space_f, band_width;
    unsigned	n_data_bits;
    int		nstartbits;
    float	nstopbits;
    int		invert_start_stop;
    int		msb_first;
    int		do_rx_sync;
    unsigned long long sync_byte;
    int		decoder;		/* enum mifsk_decoder */
    int		rx_one;
    float	confidence_threshold;
    float	search_limit;
    float	auto_carrier_threshold;
    int		autodetect_shift;
    int		inverted_freqs;

    /* plan (fsk.c:52-57) */
    int		fftsize;
    unsigned	nbands;
    unsigned	b_mark, b_space;

    /* framing (minimodem.c:943,1037,1105-1131) */
    unsigned	frame_n_bits;		/* unsigned = n_data + nstart + nstop(float) */
    float	nsamples_per_bit;
    unsigned	nsamples_overscan;
    unsigned	frame_nsamples;
    unsigned	expect_n_bits;
    unsigned	expect_nsamples;
    char	expect_data[MIFSK_MAX_FRAME_BITS + 4];
    char	expect_sync[MIFSK_MAX_FRAME_BITS + 4];
    unsigned	samplebuf_size;		/* minimodem.c:1063-1070 */

    /* search grid; index 0 = no carrier, 1 = carrier (minimodem.c:1236-1263,1366) */
    unsigned	try_first[2];
    unsigned	try_max[2];
    unsigned	try_step[2];
    unsigned	try_step_fine[2];

    /* bit windows inside fsk_find_frame (fsk.c:183,204,465) */
    float	find_samples_per_bit;	/* (float)expect_nsamples / expect_n_bits */
    unsigned	bit_nsamples;
    unsigned	bit_offset[MIFSK_MAX_FRAME_BITS];
} mifsk_rx_config;

void mifsk_modem_args_default( mifsk_modem_args *args );
int  mifsk_rx_config_init( mifsk_rx_config *cfg, const mifsk_modem_args *args );

/* upper bound on frames one stream of nsamples can yield */
size_t mifsk_max_frames( const mifsk_rx_config *cfg, size_t nsamples );
/* How far past a stream's last sample a search may logically look (last
 * candidate position + last bit window, fsk.c:204-206,480).  Informational:
 * those samples read as 0.0 whatever the memory holds, so no padding is
 * required.  (The kernels may load -- and ignore -- floats between a row's
 * nsamples[s] and the end of the batch: all nstreams * stream_stride floats
 * must be readable, nothing beyond them is touched.  The reference reads
 * stale ring-buffer memory there -- DESIGN.md "past-the-end reads".) */
size_t mifsk_stream_padding( const mifsk_rx_config *cfg );

/* ---- device context --------------------------------------------------- */

typedef struct mifsk_ctx mifsk_ctx;

/* device < 0: use the current HIP device.  -ENODEV when none is usable. */
int  mifsk_ctx_create( mifsk_ctx **ctx_out, int device );
void mifsk_ctx_destroy( mifsk_ctx *ctx );
const char *mifsk_ctx_device_name( const mifsk_ctx *ctx );
int  mifsk_abi_version( void );
/* sizeof() of the public struct `name` ("mifsk_demod_io", ...) as this library was built, 0
 * for a name it does not know: lets a foreign-function binding check its mirror of the
 * layouts before it passes one across (tests/test_config.py does, for the ctypes mirror). */
size_t mifsk_abi_sizeof( const char *name );

/* Diagnostic: the kernels take (float)sqrt(fr^2 + fi^2) of a bit window's sums (the reference's
 * hypotf, fsk.c:107-114) by a short sequence wherever that is provably the float the correctly
 * rounded one gives, and by the exact sequence otherwise (csrc/mifsk_devmath.h).  This runs both
 * on `nvalues` sums of squares (half of them placed at float rounding boundaries) and counts:
 * [0] short results accepted as safe that differ from the exact ones -- must be 0, [1] values
 * the guard sent to the exact sequence, [2] values whose unguarded short result differs,
 * [3] values evaluated.  Synchronous. */
int mifsk_selftest_sqrt( mifsk_ctx *ctx, uint64_t seed, uint64_t nvalues, uint64_t counts[4] );

/* Diagnostics: the device arithmetic the receive kernels rest on (csrc/mifsk_devlib.h,
 * csrc/mifsk_devmath.h), evaluated per value on HOST arrays (copied in and out; synchronous) so
 * that a caller can compare it with a reference of its own (tests/test_gpu_devmath.py).  The
 * kernels call the routines themselves.  -EINVAL for a null pointer; n = 0 does nothing.
 *
 * _rcp: rcp_out[i] = the double reciprocal of c[i] that stands in for a float division,
 *   quot_out[i] = x[i] / c[i] made with it (exact for finite non-zero c[i] and a quotient that
 *   is not subnormal).
 * _mag: with s = (float)re[i]^2 + (float)im[i]^2 as the magnitude of a band builds it:
 *   sqrt_out[i] = the exact sequence's sqrt(s), g_out[i] / unsafe_out[i] = the short sequence's
 *   root and its verdict (1: this value needs the exact sequence), mag_out[i] = the band
 *   magnitude (float)sqrt(s) * scalar.
 * _confidence: `ncases` frames of `n_bits` bits, mags[case][bit] = { mark, space } magnitude,
 *   through the confidence pass -- variant 0: the generic one, 1: the wavefront engine's choice
 *   (specialised at 8, 10 and 11 bits), 2: the workgroup engine's.  Case i runs on lane i % 64 of
 *   wave i / 64: the specialised passes send a whole wave through their division arm when any of
 *   its lanes needs it, and say so in fell_back_out[i].  req_mask / req_val: the required bits;
 *   a frame that misses them gives 0, 0, 0.  -EINVAL for n_bits = 0 or > MIFSK_MAX_FRAME_BITS
 *   and for a variant that does not exist. */
int mifsk_selftest_rcp( mifsk_ctx *ctx, const float *c, const float *x, uint64_t n,
	double *rcp_out, float *quot_out );
int mifsk_selftest_mag( mifsk_ctx *ctx, const double *re, const double *im, float scalar, uint64_t n,
	double *sqrt_out, double *g_out, uint8_t *unsafe_out, float *mag_out );
int mifsk_selftest_confidence( mifsk_ctx *ctx, int variant, uint32_t n_bits, uint64_t req_mask,
	uint64_t req_val, const float *mags, uint64_t ncases, float *conf_out, float *ampl_out,
	uint64_t *bits_out, uint32_t *fell_back_out );
/* _gauss: the transform of the channel model's noise field (mifsk_impair_batch below;
 * csrc/mifsk_gauss.h) for chosen words, which cannot be steered through Philox: z_out[i] =
 * { R(words[i][0]) C(words[i][1]), R(words[i][0]) S(words[i][1]) }, words [n][2], z_out [n][2]. */
int mifsk_selftest_gauss( mifsk_ctx *ctx, const uint32_t *words, uint64_t n, double *z_out );
/* _turn: the FM stage's angle (mifsk_fm_demod_batch below; csrc/mifsk_angle.h) for chosen pairs,
 * most of which no pair of float samples reaches: out[i] = mifsk_turn(y[i], x[i]). */
int mifsk_selftest_turn( mifsk_ctx *ctx, const double *y, const double *x, uint64_t n, double *out );

/* Diagnostics, wave-wide routines (csrc/mifsk_devlib.h) on HOST arrays, synchronous, like the
 * three above; tests/test_gpu_correlators.py and tests/test_gpu_scans.py compare them with the
 * oracle's double sums and with a serial float loop.
 *
 * _corr: bit windows through ONE of the correlators, the four double accumulators (mark re, im,
 *   space re, im) of every window returned unrounded.  The twiddle table and the derived kernel
 *   configuration are the ones mifsk_demod_batch uses for `cfg` (bit length cfg->bit_nsamples,
 *   bands cfg->b_mark / b_space of cfg->fftsize).  Case i -- the window samples[starts[i] ..
 *   + bit length) -- runs on lane i % 64 of wave i / 64; every lane of a wave runs the routine,
 *   lanes beyond the last case on a copy of the wave's first.  `routine`:
 *     _LDS_FIXED, _LDS_FIXED_HALVES  window of 4 .. 48 (8 .. 48) samples, a multiple of 4, in LDS
 *     _LDS_STREAM, _LDS_STREAM_LEAN  window of any multiple of 4 samples in LDS, read in whole
 *                                    groups of 16 samples
 *     _GLOBAL_STREAM                 any window, read from memory in whole groups of 16
 *     _GLOBAL_TILED                  any window, through the LDS tile in whole steps of 32; the
 *                                    instantiation depends on whether a wave has more than 32 cases
 *     _SLAB_PLAIN                    any window in LDS, at any alignment
 *     _SKEWED_STREAM                 any window in a slab staged row by row from the lowest start
 *                                    on, `param` (0 / 1) pad words between the rows
 *     _SEG_GROUP                     segments of lens[i] <= bit length samples summed in lock step
 *                                    over the wave's longest, unmasked below its shortest
 *                                    (`param` 1: masked throughout); esum_out[i] = the float sum
 *                                    of squares the shared segments' error bound is made from
 *   `param` is 0 elsewhere; lens and esum_out may be NULL but for _SEG_GROUP.  The LDS routines
 *   hold all of `samples` in LDS (at most 12288).  -EINVAL, and nothing is launched, for a case
 *   that breaks its routine's precondition: a start that is no multiple of 4 (the first four
 *   routines); a window -- for _LDS_STREAM / _LDS_STREAM_LEAN / _GLOBAL_STREAM rounded up to
 *   whole groups of 16, for _GLOBAL_TILED to whole steps of 32 -- or a segment that does not end
 *   within nsamples; a bit length the routine does not take; a segment of no or more than a bit
 *   length's samples.
 * _scan: the lane scans of the bulk replay, seeded as the receive loops seed them.  Wave w starts
 *   from state[w] = { track amplitude, peak confidence, confidence total, amplitude total } and
 *   replays k[w] (1 .. 64) frames of confidence cv[w][l] and amplitude av[w][l]; x_out[w][l] is
 *   the state after frame l, b_out[w][l] the state before it, both four floats in that order and
 *   meaningful for l < k[w].  routine 0: replay_scan_asm, 1: replay_scan_soft, 2:
 *   replay_scan_track (which leaves the peak alone); totals 0: the two totals are left alone.
 * _wave_max: max_out[w] = wave_max_f32 over v[w][0 .. 63]. */
#define MIFSK_SELFTEST_CORR_LDS_FIXED		0
#define MIFSK_SELFTEST_CORR_LDS_FIXED_HALVES	1
#define MIFSK_SELFTEST_CORR_LDS_STREAM		2
#define MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN	3
#define MIFSK_SELFTEST_CORR_GLOBAL_STREAM	4
#define MIFSK_SELFTEST_CORR_GLOBAL_TILED	5
#define MIFSK_SELFTEST_CORR_SLAB_PLAIN		6
#define MIFSK_SELFTEST_CORR_SKEWED_STREAM	7
#define MIFSK_SELFTEST_CORR_SEG_GROUP		8
int mifsk_selftest_corr( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int routine, int param,
	const float *samples, uint32_t nsamples, const uint32_t *starts, const uint32_t *lens,
	uint32_t ncases, double *acc_out, float *esum_out );
int mifsk_selftest_scan( mifsk_ctx *ctx, int routine, int totals, const float *state, const float *cv,
	const float *av, const uint32_t *k, uint32_t nwaves, float *x_out, float *b_out );
int mifsk_selftest_wave_max( mifsk_ctx *ctx, const float *v, uint32_t nwaves, float *max_out );

/* ---- N independent fsk_find_frame() problems --------------------------- */

typedef struct mifsk_search {
    uint64_t	sample_offset;	/* window start, in floats, into d_samples  */
    uint32_t	navail;		/* readable floats from there; beyond = 0.0 */
    uint32_t	try_first;
    uint32_t	try_max;
    uint32_t	try_step;
    float	search_limit;
    uint32_t	use_sync_string;	/* 0: cfg->expect_data, 1: cfg->expect_sync */
} mifsk_search;

typedef struct mifsk_search_result {
    uint64_t	bits;
    float	confidence;
    float	amplitude;
    uint32_t	frame_start;
    uint32_t	n_positions;	/* positions the reference would have analysed */
} mifsk_search_result;

int mifsk_find_frame_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const float *d_samples,
	const mifsk_search *d_problems, mifsk_search_result *d_results,
	int nproblems, void *stream );

/* ---- whole-stream receive loop ----------------------------------------- */

/* one decoded frame, in loop order (optional detailed output) */
typedef struct mifsk_frame {
    uint64_t	bits;		/* data bits handed to the databits decoder
				   (after >>1, bit_window, bit_reverse)     */
    uint64_t	start;		/* absolute sample index of the frame start */
    float	confidence;
    float	amplitude;
    uint32_t	flags;		/* MIFSK_FRAME_* */
    uint32_t	reserved;
} mifsk_frame;

#define MIFSK_FRAME_ACQUIRE	1u	/* carrier was acquired on this frame   */
#define MIFSK_FRAME_SYNC	2u	/* == sync byte: suppressed from output */
#define MIFSK_FRAME_REFINED	4u	/* a fine rescan was run for this frame */

/* one carrier episode = what "### CARRIER" ... "### NOCARRIER" brackets */
typedef struct mifsk_episode {
    uint64_t	carrier_nsamples;
    uint32_t	first_frame;	/* index of its first frame in loop order   */
    uint32_t	nframes;	/* nframes_decoded                          */
    float	confidence_total;
    float	amplitude_total;
    uint32_t	end_reason;	/* 1: carrier lost, 2: end of stream        */
    uint32_t	b_mark;		/* the plan's mark band when the carrier was
				   acquired ("### CARRIER ... @ f Hz" is
				   b_mark * band_width; with --auto-carrier it
				   can change from episode to episode)      */
} mifsk_episode;

#define MIFSK_STREAM_FRAMES_TRUNCATED	1u
#define MIFSK_STREAM_EPISODES_TRUNCATED	2u
#define MIFSK_STREAM_ABORTED		4u	/* internal error: the loop was cut short */

typedef struct mifsk_demod_io {
    /* inputs */
    const float		*d_samples;	/* nstreams rows, stream-major       */
    size_t		stream_stride;	/* floats between rows (16 B aligned)*/
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples*/
    uint32_t		nsamples;
    int			nstreams;
    /* outputs (any of bytes/bits/frames may be NULL) */
    uint8_t		*d_bytes;	/* [nstreams][frames_cap]: low 8 data
					   bits of every unsuppressed frame  */
    uint32_t		*d_nbytes;	/* [nstreams]                        */
    uint64_t		*d_bits;	/* [nstreams][frames_cap] data bits of
					   every frame incl. suppressed ones */
    mifsk_frame		*d_frames;	/* [nstreams][frames_cap]            */
    uint32_t		*d_nframes;	/* [nstreams] frames in loop order   */
    size_t		frames_cap;
    mifsk_episode	*d_episodes;	/* [nstreams][episodes_cap]          */
    uint32_t		*d_nepisodes;	/* [nstreams]                        */
    size_t		episodes_cap;
    uint32_t		*d_status;	/* [nstreams] MIFSK_STREAM_* or NULL */
    uint64_t		*d_counters;	/* [nstreams][MIFSK_NCOUNTERS] work
					   counters (MIFSK_CNT_*) or NULL    */
    int32_t		*d_carrier_band;/* [nstreams] or NULL; --auto-carrier
					   only: the band the mark tone was
					   FIRST detected in, -1 = never (the
					   stream then yields nothing); later
					   re-detections (minimodem.c:1297)
					   show in mifsk_episode.b_mark      */
    uint32_t		flags;		/* MIFSK_IO_*                        */
    uint32_t		reserved;	/* 0                                 */
} mifsk_demod_io;

/* Buffer addressing of a search that reads past samples_nvalid (minimodem.c:
 * 1153,1229; fsk.c:204-206).  Default ("flat"): it sees the stream itself and
 * 0.0 beyond the stream's end.  MIFSK_IO_RING_EXACT: it sees what the
 * reference's samplebuf holds there -- the stale cells memmove left behind,
 * 0.0 where nothing was ever written (the reference: uninitialised heap) -- the
 * reference's buffer is kept cell for cell in device memory and every frame
 * goes through the general path: exact, and several times slower. */
#define MIFSK_IO_RING_EXACT	1u
/* Run the receive loop with one workgroup per stream (192 or 256 threads: master wave +
 * worker waves; the round-1 kernel) instead of one wavefront per stream.
 * Flat addressing only; --auto-carrier looks for the tone once per stream. */
#define MIFSK_IO_ENGINE_WORKGROUP 2u
/* ... or with one wavefront per stream whatever the mode.  With neither flag the
 * library chooses (the workgroup engine in the modes whose bit windows it
 * stages through LDS and that have at least 16 samples per bit). */
#define MIFSK_IO_ENGINE_WAVE	4u

/* per-stream work counters (diagnostics; cycle counts are s_memtime ticks) */
#define MIFSK_NCOUNTERS		32
#define MIFSK_CNT_ITERATIONS	0	/* passes through the general loop body  */
#define MIFSK_CNT_BATCHES	1	/* candidate batches evaluated           */
#define MIFSK_CNT_STAGES	2	/* LDS slab (re)loads                    */
#define MIFSK_CNT_BULK_FRAMES	3	/* frames accepted from the run-ahead    */
#define MIFSK_CNT_REFINES	4	/* fine rescans                          */
#define MIFSK_CNT_CACHE_HITS	5	/* searches answered from the cache      */
#define MIFSK_CNT_POSITIONS	6	/* candidate positions evaluated (SCAN)  */
#define MIFSK_CNT_LATTICE_BATCHES 7	/* pipelined lattice batches scored      */
#define MIFSK_CNT_CYC_TOTAL	8
#define MIFSK_CNT_CYC_PARALLEL	9	/* SCAN: stage + correlate + barriers    */
#define MIFSK_CNT_CYC_WAIT	10	/* LATTICE: master waiting for workers   */
#define MIFSK_CNT_CYC_CONFIDENCE 11
#define MIFSK_CNT_CYC_BULK	12
/* (13 .. 23: cycle totals of the profile build; 20 .. 22 double as event counts of the
 * shared-segment scans and of --auto-carrier) */
#define MIFSK_CNT_CONF_FALLBACKS 24	/* confidence passes that took the divisions proper (a
					   zero / non-finite class mean or a subnormal quotient
					   somewhere in the wave: frame_confidence_fixed).  A LOWER
					   bound: lane 0 does the counting, and a pass whose lane 0
					   had left already (its candidate's required bits mismatch)
					   is not counted -- counting it through a ballot moved the
					   register allocation of the loop kernels and cost 1-2 %
					   (profiles/r06_history.md)                               */
#define MIFSK_CNT_SEG_SECOND_LOOKS 25	/* shared-segment scans in which the second look (the running
					   error bound, csrc/mifsk_wave.hip) settled a window the
					   a-priori bound had not                                  */

/* Asynchronous on `stream`: the outputs are complete when `stream` reaches the point
 * behind the call.  (A large wavefront-engine batch is run as several launches on
 * streams of the context's own, forked from and joined back into `stream` with events --
 * mifsk_launch_info.chain_groups below; nothing changes for the caller.)  Calls on ONE
 * context are ordered by the caller (a context owns its launch scratch); to keep several
 * batches in flight -- a launch ends well after its mean stream, so the next one fills the
 * chip -- use a mifsk_pipeline (below), which gives each pass a context and a stream. */
int mifsk_demod_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io, void *stream );

/* ---- several batches in flight ---------------------------------------------- */

/* A launch ends well after its mean stream (the streams of a batch are serial chains of unequal
 * length), so the way to keep the chip full is to have the next batch running under the tail of
 * this one.  A pipeline owns what that needs: `depth` lanes -- each a context, a HIP stream and a
 * completion event of its own -- and, if asked, `depth` sets of output arrays.  Pass number t
 * (its "ticket", counting from 0) runs on lane t % depth, behind whatever ran on that lane
 * before.  For the reference's call site -- one file after another through the batch entry,
 * src/minimodem.c:1265,1373 via integration/minimodem-rx-batch.patch -- this is "decode the
 * next batch of files while the last streams of this one finish".
 *
 * HIP runs a process's streams on GPU_MAX_HW_QUEUES hardware queues (4 unless the environment
 * said otherwise when the runtime started) and the null stream takes one: lanes beyond that
 * would share a queue and run one behind the other, which measures slower than fewer lanes.
 * The depth is therefore clamped to the queues there are; mifsk_pipeline_info_get says what
 * was asked for, what is in effect and how many queues the runtime has.  (Export
 * GPU_MAX_HW_QUEUES=8 before the first HIP call for a depth above 3.)
 *
 * Results are identical to mifsk_demod_batch's, pass for pass: a lane is an ordinary context
 * and stream.  The calls are serialised per pipeline; submit never blocks on the device. */
typedef struct mifsk_pipeline mifsk_pipeline;
#define MIFSK_PIPELINE_MAX_DEPTH	8
#define MIFSK_PIPELINE_NO_PRODUCER	((void *)(intptr_t)-1)

typedef struct mifsk_pipeline_info {
    uint32_t	depth_requested;
    uint32_t	depth;		/* lanes in effect: min(requested, hw_queues - 1), at least 1 */
    uint32_t	hw_queues;	/* GPU_MAX_HW_QUEUES as this process's environment has it (4: unset) */
    uint32_t	output_sets;	/* `depth` once mifsk_pipeline_outputs_alloc has run, else 0 */
} mifsk_pipeline_info;

#define MIFSK_WANT_BYTES	1u
#define MIFSK_WANT_BITS		2u
#define MIFSK_WANT_FRAMES	4u
#define MIFSK_WANT_EPISODES	8u

/* device < 0: the current HIP device.  -ENODEV without a usable device. */
int  mifsk_pipeline_create( mifsk_pipeline **out, int device, int depth );
void mifsk_pipeline_destroy( mifsk_pipeline *p );	/* waits for what is in flight */
int  mifsk_pipeline_info_get( const mifsk_pipeline *p, mifsk_pipeline_info *info );

/* One set of output arrays per lane, for batches of up to `nstreams` streams: counts and status
 * always, the arrays `want` names (MIFSK_WANT_*).  Replaces sets made before (after waiting for
 * what is in flight).  mifsk_pipeline_outputs_get fills the output fields of *io (pointers and
 * capacities, nothing else) with the set pass `ticket` writes or wrote. */
int  mifsk_pipeline_outputs_alloc( mifsk_pipeline *p, int nstreams, size_t frames_cap,
	size_t episodes_cap, unsigned want );
int  mifsk_pipeline_outputs_get( mifsk_pipeline *p, uint64_t ticket, mifsk_demod_io *io );

/* mifsk_demod_batch(cfg, io) as the pipeline's next pass; *ticket (may be NULL) receives its
 * number (= mifsk_pipeline_next_ticket before the call).  `after`: the hipStream_t the batch
 * was produced on -- the lane waits for the point that stream has reached now (NULL is the
 * null stream) -- or MIFSK_PIPELINE_NO_PRODUCER.  An io without any output pointer is given the
 * lane's own set (mifsk_pipeline_outputs_alloc).  The set a pass writes is the set pass
 * ticket - depth wrote: whatever reads that one must be ordered before this submit -- on the
 * lane's stream (mifsk_pipeline_stream: what a gather of the results is queued on), or by a
 * mifsk_pipeline_wait. */
int  mifsk_pipeline_submit( mifsk_pipeline *p, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io, void *after, uint64_t *ticket );
uint64_t mifsk_pipeline_next_ticket( const mifsk_pipeline *p );
/* the host waits until pass `ticket` is complete (and with it everything submitted on its lane
 * up to now); -EINVAL for a ticket not yet issued */
int  mifsk_pipeline_wait( mifsk_pipeline *p, uint64_t ticket );
/* ... or `stream` does, on the device */
int  mifsk_pipeline_join( mifsk_pipeline *p, uint64_t ticket, void *stream );
/* everything submitted so far */
int  mifsk_pipeline_drain( mifsk_pipeline *p );
/* the lane of pass `ticket`: its hipStream_t and its context */
void *mifsk_pipeline_stream( mifsk_pipeline *p, uint64_t ticket );
mifsk_ctx *mifsk_pipeline_ctx( mifsk_pipeline *p, uint64_t ticket );

/* ---- one process per GPU: decoded bytes to one rank -------------------------- */

/* Streams are independent: rank r of `world` demodulates mifsk_shard_range(nstreams, r, world)
 * and nothing is exchanged on the way.  Where ONE rank must end up holding every stream's bytes
 * (a job launched as one process per GPU; the reference is one process and has no counterpart,
 * src/minimodem.c:1014-1032), the results are gathered to rank 0 over RCCL: every peer sends on
 * its own xGMI link, the root posts all its receives as one group.  RCCL is opened at run time
 * (dlopen of librccl.so.1, the copy the process already has if there is one) and only by these
 * calls: -ENOSYS when it cannot be.
 *
 * Rendezvous: rank 0 makes an id (mifsk_gather_unique_id) and the job's launcher carries its
 * MIFSK_GATHER_ID_BYTES bytes to every rank (MPI, a socket, torch.distributed, a file); every
 * rank then calls mifsk_gather_create -- a collective call, like ncclCommInitRank.
 *
 * mifsk_gather_start enqueues ONE gather on `stream` behind whatever produced the arrays there
 * (the lane's stream of a pipeline pass: mifsk_pipeline_stream) and returns its ticket; it is
 * complete when `stream` reaches the point behind the call.  Only the first `cols` columns of
 * every [row_pitch]-wide row travel (a stream's bytes cannot exceed mifsk_max_frames of its
 * length), through a dense staging copy made on `stream`.  rows[world]: streams per rank (NULL:
 * every rank holds `nstreams`).  The root keeps `slots` receive sets and the k-th gather fills
 * set k % slots, the senders as many staging copies: with up to `slots` gathers in flight none
 * overwrites what an older one delivered.  mifsk_gather_received (rank 0) names what peer
 * `peer` >= 1 sent in gather `ticket`: rows x cols bytes, dense, and the counts.
 *
 * MIFSK_GATHER_LOOPBACK (world == 1 only): the one rank sends to ITSELF through the same calls
 * and receives it as peer 0 -- the whole transport on one GPU (tests/test_gpu_gather.py).
 * Without it a world of one makes no communicator and start() has nothing to do. */
typedef struct mifsk_gather mifsk_gather;
#define MIFSK_GATHER_ID_BYTES	128
#define MIFSK_GATHER_LOOPBACK	1u

typedef struct mifsk_gather_info {
    int		rank, world, device;
    uint32_t	slots;
    uint32_t	loopback;
    uint32_t	communicator;	/* 1: an RCCL communicator was made */
} mifsk_gather_info;

int  mifsk_gather_unique_id( void *id /* [MIFSK_GATHER_ID_BYTES] */ );
/* device < 0: the current HIP device; slots clamped to 2 .. 16 */
int  mifsk_gather_create( mifsk_gather **out, const void *id, int rank, int world, int device,
	int slots, unsigned flags );
void mifsk_gather_destroy( mifsk_gather *g );	/* synchronises the device first */
int  mifsk_gather_info_get( const mifsk_gather *g, mifsk_gather_info *info );
int  mifsk_gather_start( mifsk_gather *g, const uint8_t *d_bytes, size_t row_pitch,
	const int32_t *d_nbytes, int nstreams, int cols, const int *rows, void *stream,
	uint64_t *ticket );
int  mifsk_gather_received( mifsk_gather *g, uint64_t ticket, int peer,
	const uint8_t **d_bytes, const int32_t **d_nbytes, int *rows, int *cols );

/* What mifsk_demod_batch would launch for `cfg`, a batch of `nstreams` streams and
 * `flags` (MIFSK_IO_*): the kernel instantiation, its launch geometry and the
 * occupancy its LDS allows -- what rocprofv3 does not report for dynamic LDS. */
typedef struct mifsk_launch_info {
    char	kernel[64];
    uint32_t	engine;			/* MIFSK_IO_ENGINE_WAVE or _WORKGROUP   */
    uint32_t	workgroup_size;		/* threads (64: a workgroup is a wave)  */
    uint32_t	lds_bytes_per_workgroup;/* dynamic LDS                          */
    uint32_t	workgroups_per_cu;	/* min(160 KiB / LDS, 32 waves / size): VGPRs
					   may lower it (4 waves per SIMD at 128) */
    uint32_t	lattice_mode;		/* 0 none, 1 LDS-staged rounds, 2 streamed */
    uint32_t	frames_per_block;	/* LATTICE frames scored at once, at most */
    uint32_t	compute_units;
    /* Chained launches: a flat-addressed wavefront-engine batch of more streams than the
     * chip holds at once is cut into chain_groups groups of streams x chain_chunks time
     * chunks, every (group, chunk) one launch of the resumable kernel, each group's chunks
     * in order on a HIP stream of the context's -- so that the slots one group's
     * stragglers leave are filled with another group's next chunk instead of staying
     * empty until the round ends.  Same frames, bit for bit (mifsk_demod_slab's
     * guarantee).  0 / 0: one launch. */
    uint32_t	chain_groups, chain_chunks;
} mifsk_launch_info;

int mifsk_demod_plan( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int nstreams,
	unsigned flags, mifsk_launch_info *out );
/* ... for rows of `nsamples` samples (mifsk_demod_io.nsamples): whether a batch is cut in
 * time depends on how long its streams are (mifsk_demod_plan assumes long ones) */
int mifsk_demod_plan_ex( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int nstreams,
	uint32_t nsamples, unsigned flags, mifsk_launch_info *out );

/* ---- streams that start in host memory (SURVEY 8 d "H2D-inclusive") -------- */

/* How a zig-zag scan with long bit windows is evaluated (diagnostic; DESIGN.md "shared
 * segments"): kind = 2 * fine + carrier.  valid == 0: every window is correlated by
 * itself.  Otherwise the span the scan's windows cover is cut into nseg segments, each
 * summed once in one of npass passes of lanes (lock-step length pass_len[p]); window w
 * (= candidate in scan order * expect_n_bits + bit) is the sum of segments
 * win_first[w] .. win_first[w] + win_count[w] - 1, rotated. */
typedef struct mifsk_scan_plan {
    uint32_t	valid, nseg, npass, nwin, span_hi;
    uint32_t	pass_len[2], pass_min[2];
    float	bound_c;
    uint32_t	seg_rel[128];
    uint16_t	seg_len[128], slot_seg[128], win_first[128], win_count[128];
    uint32_t	p_slot[128], p_win[128];	/* the same, packed as the kernel reads it */
    uint8_t	p_slot_seg[128];
} mifsk_scan_plan;

int mifsk_scan_plan_get( const mifsk_rx_config *cfg, int kind, mifsk_scan_plan *out );

/* Same, for HOST pointers in `io` (all fields, d_ prefix notwithstanding).  The
 * batch is cut into chunks of whole streams (~64 MB of input); chunk k+1 crosses
 * PCIe on a copy stream while chunk k is demodulated and chunk k-1's results are
 * copied back, so the call runs at the speed of the bus.  Input rows in
 * page-locked memory (mifsk_host_alloc, hipHostMalloc, hipHostRegister) are
 * copied by DMA from where they are; anything else is first moved into the
 * context's own pinned staging buffers by worker threads.  Synchronous: results
 * are in place on return.  One host call at a time per context (calls on one
 * context serialise; use one context per device and per concurrent caller). */
int mifsk_demod_batch_host( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io );

/* `io->d_samples` points to int16_t rows (`stream_stride` counts int16 elements):
 * PCM16 as a WAV file holds it.  It crosses the bus as 16-bit and is converted on
 * the device the way libsndfile converts it for the reference (value / 32768,
 * simpleaudio-sndfile.c:42-56).  Host entry points only. */
#define MIFSK_IO_HOST_S16	0x100u

typedef struct mifsk_host_stats {
    double	seconds_total;		/* wall time of the call                          */
    double	seconds_staging;	/* of which: worker threads filling pinned memory */
    uint64_t	bytes_h2d, bytes_d2h;
    uint32_t	chunks, streams;
    uint32_t	source_pinned;		/* 1: input rows were DMA'd from the caller's memory */
    uint32_t	reserved;
} mifsk_host_stats;

/* ... with the --Xrxnoise term (0 = off; see mifsk_ingest_s16) applied on the
 * device, and what the pipeline did reported in *stats (may be NULL). */
int mifsk_demod_batch_host_ex( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io, float rxnoise, mifsk_host_stats *stats );

/* page-locked host memory for the inputs of the host entry points */
void *mifsk_host_alloc( size_t bytes );
void  mifsk_host_free( void *p );

/* upper bound on carrier episodes one stream of nsamples can yield */
size_t mifsk_max_episodes( const mifsk_rx_config *cfg, size_t nsamples );

/* ---- streams that arrive in pieces (minimodem.c:1144-1174; SURVEY 8 e) ------- */

/* The receive loop's state between two calls, one per stream, in DEVICE memory;
 * all zero = a stream that has not started.  Everything the reference carries
 * from one pass of its loop to the next (minimodem.c:1079-1088,1132-1133,
 * 1144-1174): the buffer arithmetic, the carrier episode's running totals, the
 * tracker's amplitude and peak confidence, the --auto-carrier band. */
typedef struct mifsk_stream_state {
    uint64_t	base;		/* stream index of samplebuf[0]: the caller may drop
				   every sample before it                         */
    uint64_t	rp;		/* the reference's file position                  */
    uint64_t	carrier_nsamples;
    uint64_t	nframes_total;	/* frames emitted by all calls so far             */
    uint32_t	advance;
    uint32_t	flags;		/* MIFSK_STATE_*                                  */
    float	confidence_total, amplitude_total;
    uint32_t	nframes_decoded;
    uint32_t	noconfidence;
    float	track_amplitude, peak_confidence;
    int32_t	carrier_band, first_band;
    uint32_t	b_mark, ep_b_mark;
    uint32_t	ep_first;
    uint32_t	nbytes_total;	/* bytes, episodes emitted by all calls so far    */
    uint32_t	nepisodes_total;
    uint32_t	status;		/* MIFSK_STREAM_* bits of all calls so far        */
} mifsk_stream_state;

#define MIFSK_STATE_STARTED	1u
#define MIFSK_STATE_CARRIER	2u
#define MIFSK_STATE_FINISHED	4u	/* the final slab has been processed */

/* mifsk_demod_batch for streams that are longer than what is resident, or that
 * arrive in pieces.  Row s of io->d_samples holds the samples of stream s from
 * stream index d_origin[s] on (NULL: every row starts at index 0 -- only right
 * for the first slab), io->d_nsamples[s] of them; d_origin[s] must not exceed
 * d_state[s].base, i.e. the caller keeps what the loop has not passed yet and
 * appends the new samples behind it.  With final == 0 the loop stops, and saves
 * its state, at the first pass that could read beyond the row (it needs a whole
 * samplebuf -- cfg->samplebuf_size samples -- beyond the cursor to be sure of
 * seeing exactly what one call over the whole stream sees); with final != 0 the
 * row's end is the stream's end.  Per call the outputs start at index 0 of their
 * arrays (frames in loop order, episodes as they END); mifsk_frame.start and
 * mifsk_episode.first_frame count from the start of the stream.  Any cut of a
 * stream into slabs gives the frames and episodes of the single call, bit for
 * bit.  Flat addressing; io->flags may force an engine (MIFSK_IO_ENGINE_WAVE /
 * _WORKGROUP), otherwise the library chooses as mifsk_demod_batch does -- the
 * state record is the same for both, a stream may even change engines between
 * slabs.  Asynchronous on `stream`. */
int mifsk_demod_slab( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const mifsk_demod_io *io,
	mifsk_stream_state *d_state, const uint64_t *d_origin, int final, void *stream );

/* The same with the reference's buffer semantics (MIFSK_IO_RING_EXACT): what a search
 * reads behind samples_nvalid is what the reference's samplebuf holds there -- stale
 * samples that memmove left behind (minimodem.c:1150-1156) -- also across calls.
 * d_ring is [nstreams][mifsk_ring_floats(cfg)] floats of device memory that the
 * caller zeroes before a stream's first slab and keeps with d_state; a pass of the
 * loop needs only the refill the reference's fread would deliver (half a samplebuf)
 * to be in the row, not a whole samplebuf beyond the cursor.  Any cut gives the
 * one-shot MIFSK_IO_RING_EXACT result, i.e. `minimodem --rx --file`'s, digit for
 * digit.  Wavefront engine. */
size_t mifsk_ring_floats( const mifsk_rx_config *cfg );
int mifsk_demod_slab_ring( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const mifsk_demod_io *io,
	mifsk_stream_state *d_state, const uint64_t *d_origin, float *d_ring, int final,
	void *stream );

/* ---- one long recording across the whole chip (DESIGN.md "cutting a stream in time") --- */

/* Every entry point above gets its parallelism from having many streams: one stream's loop
 * runs on one wavefront.  mifsk_demod_long decodes ONE long recording (an hour of SDR audio,
 * a day of SAME monitoring) on the whole chip, bit for bit what one mifsk_demod_batch call
 * over it gives.  The recording is cut into K chunks starting at s_k = k * chunk; every chunk
 * but the first is first run for `warmup` samples from a zeroed state (pass A, a guess at the
 * loop's state there), then every chunk runs from its guess to `warmup` samples into the next
 * chunk (pass B).  A chunk is accepted when the state its guess paused in equals, in every
 * CONTROL field (the header comment of minimodem_amd/csrc/mifsk_timesplit.hip), the state the
 * chunk before paused in at the same sample; a rejected chunk is run again from that state.
 * Re-runs go in rounds: every chunk whose starting state disagrees with its predecessor's
 * current pause (settled or not) is run again in one batch, and the consistent prefix is
 * settled -- so the rounds follow the longest chain of rejections, not their number.  The
 * result is always exact.
 *
 * chunk: samples between chunk starts, a multiple of lcm(samplebuf_size / 2, 4) (0: the
 * library's choice: the chip's worth of chunks); warmup: >= 2 * samplebuf_size (0: the
 * library's choice, 10 s of audio); chunks: how many chunks the library's choice aims at (0:
 * as many as the engine keeps resident, 4 per compute unit).  flags: MIFSK_IO_ENGINE_* as for
 * mifsk_demod_batch; MIFSK_IO_RING_EXACT is -ENOTSUP (the reference's stale cells matter only
 * at the end of the stream); MIFSK_TIME_SPLIT_REJECT_ALL (tests) rejects every guess, so that
 * every chunk goes through the re-run path.  With the library's choices a recording shorter
 * than 4 * warmup is one chunk: the single call. */
typedef struct mifsk_time_split {
    uint64_t	chunk;
    uint64_t	warmup;
    uint32_t	chunks;
    uint32_t	flags;
} mifsk_time_split;

#define MIFSK_TIME_SPLIT_REJECT_ALL	0x10000u

typedef struct mifsk_time_split_stats {
    uint64_t	nsamples;
    uint64_t	chunk;			/* L: samples between chunk starts       */
    uint64_t	warmup;			/* W                                     */
    uint64_t	lattice;		/* lcm(samplebuf_size / 2, 4)            */
    uint64_t	samples_speculative;	/* pass A and the warm-up overlaps       */
    uint64_t	samples_rerun;		/* loop samples of the re-runs           */
    uint32_t	nchunks;		/* K (1: the single call)                */
    uint32_t	accepted;		/* guesses accepted (of K - 1)           */
    uint32_t	rerun;			/* chunks run again                      */
    uint32_t	rounds;			/* serial rounds of re-runs              */
} mifsk_time_split_stats;

/* The planner (host only): what mifsk_demod_long would do with `nsamples` samples -- nchunks,
 * chunk, warmup, lattice and samples_speculative (the rest 0).  Without a device the library's
 * choice of chunk aims at 1024 chunks (fewer where their warm-up overlap would pass 4 GiB).
 * -EINVAL: a chunk off the lattice, a warmup below 2 * samplebuf_size, unknown or contradictory
 * flags, rows of 2^31 samples or more, a single chunk of 2^32 samples or more;
 * -ENOTSUP: MIFSK_IO_RING_EXACT. */
int mifsk_time_split_plan_get( const mifsk_rx_config *cfg, uint64_t nsamples,
	const mifsk_time_split *params, mifsk_time_split_stats *out );

/* Decode d_samples[0 .. nsamples) (16-byte aligned; nothing beyond nsamples is read) as one
 * stream.  The outputs go to io_out's output fields exactly as mifsk_demod_batch writes those of
 * a batch of one stream (size them with mifsk_max_frames / mifsk_max_episodes of nsamples); its
 * input fields, d_counters and flags are ignored.  params may be NULL (the library's choices),
 * stats too.  Synchronous: verification reads the chunks' states back, so the call waits for
 * `stream` before it returns.  Device memory: the chunks' rows are a copy of the recording laid
 * out apart, K * (chunk + warmup) floats -- about (1 + warmup / chunk) times the recording; the
 * library's choice of chunk keeps the extra (K - 1) * warmup floats within 4 GiB -- plus the
 * rows' output arrays (about 32 bytes per possible frame), allocated on `stream` and freed before
 * the return.  Length: a row (chunk + warmup) must stay below 2^31 samples, so the longest
 * recording is about 2^31 times the chunk count (at 1024 chunks about 2 * 10^12 samples, 500
 * days at 48 kHz); -EINVAL beyond.  A recording the planner leaves in one chunk must be shorter
 * than 2^32 samples. */
int mifsk_demod_long( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const float *d_samples,
	uint64_t nsamples, const mifsk_time_split *params, const mifsk_demod_io *io_out,
	mifsk_time_split_stats *stats, void *stream );

/* Several long recordings at once: eight receivers' one-hour recordings, 32 ten-minute files --
 * too few streams to fill the chip with one wavefront each.  One `warmup` W and one `chunk` L cut
 * the whole batch, so that every chunk of every stream is a row of one flat batch and a pass is one
 * launch.  W is chosen as for one recording; with chunk == 0, L = ceil(sum_m max(0, n_m - W) /
 * target) rounded up to the lattice, target being params->chunks or the chip's worth (1024 in the
 * host-only planner), capped so that the rows' warm-up overlap stays within 4 GiB; stream m gets
 * K_m = (n_m - W) / L + 1 chunks (1 where n_m <= W).  With the library's choices the batch is one
 * mifsk_demod_batch call (nchunks 1 everywhere, chunk = the stream's length) when no stream is as
 * long as 4 * W; so it is whenever the plan leaves every stream in one chunk.  Limits and error
 * codes are mifsk_time_split_plan_get's, the row count (sum of K_m) standing in for K; nstreams
 * <= 0 or a NULL array is -EINVAL.  For nstreams == 1 the plan is mifsk_time_split_plan_get's.
 * out[m]: nsamples, chunk, warmup, lattice, nchunks = K_m and samples_speculative of stream m. */
int mifsk_time_split_plan_batch_get( const mifsk_rx_config *cfg, const uint64_t *nsamples,
	int nstreams, const mifsk_time_split *params, mifsk_time_split_stats *out /* [nstreams] */ );

/* mifsk_demod_long over `nstreams` recordings: row m of d_samples (16-byte aligned, rows
 * stream_stride floats apart, stream_stride % 4 == 0) holds nsamples[m] <= stream_stride samples;
 * nsamples is a HOST array.  Nothing beyond nstreams * stream_stride floats is read.  io_out's
 * output fields are those of a mifsk_demod_batch over nstreams streams ([nstreams][frames_cap] and
 * so on), bit for bit; its input fields, d_counters and flags are ignored.  A chunk is verified
 * against its predecessor only inside its own stream, every pass and every round of re-runs is one
 * launch over the rows of all streams, and the streams' tails run as one batch: the call's rounds
 * are the longest chain of rejections in any one stream, not the sum over the streams.  A stream
 * that finishes early (--rx-one) drops only its own later chunks.  stats (NULL or [nstreams]): the
 * plan of stream m plus its accepted, rerun, samples_rerun and the rounds in which one of its
 * chunks was run again (the call's rounds are the largest of them).  Device memory: sum of K_m *
 * (chunk + warmup) floats plus the rows' output arrays.  Synchronous, as mifsk_demod_long is --
 * which is this call with nstreams == 1. */
int mifsk_demod_long_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const float *d_samples,
	size_t stream_stride, const uint64_t *nsamples /* host, [nstreams] */, int nstreams,
	const mifsk_time_split *params, const mifsk_demod_io *io_out,
	mifsk_time_split_stats *stats /* [nstreams] or NULL */, void *stream );

/* mifsk_demod_long_batch over PCM16 as a WAV file holds it: row m of d_pcm (16-byte aligned, rows
 * pcm_stride int16 elements apart, pcm_stride % 8 == 0) holds nsamples[m] <= pcm_stride samples.
 * The chunks' rows are gathered straight from the PCM16 -- value / 32768 plus the --Xrxnoise term
 * (rxnoise: the option's factor, 0 = off), mifsk_ingest_s16's arithmetic -- so the recording never
 * exists as floats: device memory is the 2-byte source plus the rows, not source, a float copy and
 * the rows.  The outputs are bit for bit those of mifsk_ingest_s16(..., rxnoise) into float rows
 * followed by one mifsk_demod_batch; nstreams == 1 is the single recording.  A batch the plan
 * leaves uncut is converted by mifsk_ingest_s16 into a temporary buffer and decoded by one
 * mifsk_demod_batch call.  Checked in this order, before any HIP call: -EINVAL for a NULL ctx, cfg,
 * io_out or nsamples; for nstreams <= 0; for a base that is not 16-byte aligned or a pcm_stride
 * that is not a multiple of 8; for nsamples[m] > pcm_stride; then the planner's codes
 * (MIFSK_IO_RING_EXACT: -ENOTSUP).  Everything else is mifsk_demod_long_batch's. */
int mifsk_demod_long_batch_s16( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const int16_t *d_pcm, size_t pcm_stride /* int16 elements, % 8 == 0 */,
	const uint64_t *nsamples /* host, [nstreams] */, int nstreams, float rxnoise,
	const mifsk_time_split *params, const mifsk_demod_io *io_out,
	mifsk_time_split_stats *stats /* [nstreams] or NULL */, void *stream );

/* mifsk_demod_long_batch for recordings in HOST memory: rows[m] points to nsamples[m] samples,
 * float32 (src_flags 0) or PCM16 (MIFSK_IO_HOST_S16) -- one pointer per recording, long recordings
 * do not sit at a common stride.  The samples cross the bus as they are (PCM16 as 16-bit) into one
 * device buffer with a common stride, in pieces of the size mifsk_demod_batch_host uses: by DMA
 * from where they are when every row is page-locked, otherwise through the context's pinned
 * staging buffers, one piece being staged by the worker threads while the piece before is copied;
 * no pinned memory of the recording's size is made.  PCM16 is then decoded by
 * mifsk_demod_long_batch_s16, floats by mifsk_ingest_rxnoise_f32 (rxnoise != 0) and
 * mifsk_demod_long_batch.  io_out holds HOST pointers, laid out as mifsk_demod_batch_host writes
 * them; stats ([nstreams] or NULL) as mifsk_demod_long_batch fills it; hstats (may be NULL): bytes
 * each way, staging seconds, source_pinned, chunks = the number of pieces.  -EINVAL for a NULL
 * argument, nstreams <= 0, other src_flags or a NULL row of samples, then the planner's codes for
 * `params`, all before any HIP call.  Synchronous; one host call at a time per context. */
int mifsk_demod_long_batch_host( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const void *const *rows /* host, [nstreams]: one pointer per recording */,
	const uint64_t *nsamples, int nstreams, unsigned src_flags /* 0 or MIFSK_IO_HOST_S16 */,
	float rxnoise, const mifsk_time_split *params, const mifsk_demod_io *io_out /* HOST pointers */,
	mifsk_time_split_stats *stats, mifsk_host_stats *hstats /* may be NULL */ );

/* ---- streams fed in pieces from host memory ---------------------------------- */

/* mifsk_demod_slab with the bookkeeping done (reference: the loop that reads its stream half a
 * samplebuf at a time, src/minimodem.c:1144-1174 -- a recording longer than memory, live audio).
 * A session holds `nstreams` streams: per stream the samples the loop has not passed yet (host
 * memory), where they start in the stream, the loop state and (RING) the samplebuf cells on the
 * device, and arrays sized for every feed.  mifsk_session_feed takes each stream's NEW samples
 * -- samples[s] / nsamples[s], any amount, none (NULL / 0) included -- runs the loop as far as
 * the data allows (`final`: no more will come, the rows' ends are the streams' ends) and waits
 * for the results: mifsk_session_get(s, i) is what THIS feed made of stream i -- frames in loop
 * order, episodes as they end, frame starts and episode frame indices counted from the start of
 * the stream -- in host memory the session owns, valid until the next feed.  Any cut gives,
 * concatenated, the results of one call over the whole streams, bit for bit.
 * flags: MIFSK_IO_RING_EXACT (the reference's buffer semantics across the feeds: `minimodem
 * --rx --file`'s frames digit for digit), MIFSK_IO_ENGINE_*, MIFSK_SESSION_WANT_FRAMES,
 * MIFSK_SESSION_RESIDENT (below).
 * One feed at a time per session; sessions on one context are ordered by the caller. */
typedef struct mifsk_session mifsk_session;
#define MIFSK_SESSION_WANT_FRAMES	0x1000u	/* the per-frame records too */

typedef struct mifsk_session_result {
    uint32_t		nframes, nbytes, nepisodes;	/* of this feed */
    uint32_t		status;		/* MIFSK_STREAM_* of this feed                 */
    int32_t		carrier_band;	/* --auto-carrier (see mifsk_demod_io)         */
    uint32_t		finished;	/* 1: the final piece has been decoded         */
    const uint64_t	*bits;		/* [nframes] data bits of every frame          */
    const uint8_t	*bytes;		/* [nbytes]                                    */
    const mifsk_frame	*frames;	/* [nframes], or NULL without WANT_FRAMES      */
    const mifsk_episode	*episodes;	/* [nepisodes]                                 */
    uint64_t		consumed;	/* stream index the loop has passed for good   */
} mifsk_session_result;

int  mifsk_session_create( mifsk_session **out, mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	int nstreams, unsigned flags );
void mifsk_session_destroy( mifsk_session *s );
int  mifsk_session_feed( mifsk_session *s, const float *const *samples, const uint32_t *nsamples,
	int final );
const mifsk_session_result *mifsk_session_get( const mifsk_session *s, int stream );
/* samples of stream `stream` the session still holds (fed, not yet passed by the loop) */
size_t mifsk_session_pending( const mifsk_session *s, int stream );

/* ---- the resident session: tails on the device, PCM16 and device samples ----- */

/* MIFSK_SESSION_RESIDENT (with any other flag of mifsk_session_create) keeps the unconsumed
 * samples in device memory: two row buffers of nstreams x row_capacity floats, used in turn.  A
 * feed uploads the new samples and one small per-stream table, in ONE copy, and nothing else --
 * PCM16 as 16-bit -- or takes the samples from device memory and uploads the table alone; a HIP
 * kernel moves what the loop has not passed to the front of each row of the other buffer, puts
 * the new samples behind it (converted, and with the --Xrxnoise term `rxnoise` added, by the
 * expressions of mifsk_ingest_s16 / mifsk_ingest_rxnoise_f32) and zero-fills up to the feed's
 * width.  The host keeps integers only.  The buffers grow as DevBuf does (25 % head-room) when a
 * feed needs more: -ENOMEM when the device has no room (0.5 baud needs 2 x 2.3 M floats per
 * stream and more).  Results, `pending`, `consumed`: exactly the host-tail session's, whatever
 * the source.
 *   mifsk_session_feed       on a resident session: feed_ex(MIFSK_FEED_F32, rxnoise 0).
 *   mifsk_session_feed_ex    host pointers, one per stream (NULL / 0: nothing new for it), all
 *                            of one `kind`.
 *   mifsk_session_feed_device one DEVICE array [nstreams][stride] of `kind` elements (rows may
 *                            start at any multiple of the element size); nsamples is a HOST
 *                            array; `producer` is the HIP stream the samples were written on
 *                            (the session's stream waits for an event recorded on it) or
 *                            MIFSK_PIPELINE_NO_PRODUCER: they are complete.  Only
 *                            d_samples[i][0 .. nsamples[i]) is read, until the call returns.
 * -EINVAL: a session without the flag, an unknown kind, a count without its pointer (d_samples ==
 * NULL with any count non-zero), a stride smaller than a count, a feed after the final one.
 * A FAILED FEED, refused or broken off, leaves a session of EITHER kind as it was before the call
 * -- the rows it built are in the other buffer (host-tail: in the staging rows), and what the
 * session holds of a stream changes only after the loop has run -- so the caller may repeat it.
 * A stream whose loop has FINISHED (--rx-one after its carrier loss, an aborted
 * loop) holds nothing from then on: later samples for it are ignored, its pending is 0 and its
 * results are empty; so a live stream's row stays below about two samplebufs plus the piece.
 * (The host-tail session keeps appending to such a stream's tail.) */
#define MIFSK_SESSION_RESIDENT	0x2000u	/* the unconsumed tails live in device memory */

#define MIFSK_FEED_F32	0u
#define MIFSK_FEED_S16	1u		/* PCM16: (float)v / 32768.0f, libsndfile's normalisation */

int mifsk_session_feed_ex( mifsk_session *s, const void *const *samples, const uint32_t *nsamples,
	unsigned kind, float rxnoise, int final );
int mifsk_session_feed_device( mifsk_session *s, const void *d_samples, size_t stride,
	const uint32_t *nsamples, unsigned kind, float rxnoise, int final, void *producer );

/* of either kind of session */
typedef struct mifsk_session_info {
    uint32_t	resident;		/* 1: MIFSK_SESSION_RESIDENT                       */
    uint32_t	feeds;			/* feeds that succeeded                            */
    uint64_t	row_capacity;		/* elements per stream in each of the two buffers  */
    uint64_t	device_bytes;		/* what the session holds on the device            */
    uint64_t	h2d_bytes_last;		/* host-to-device bytes of the last feed, tables included */
    uint64_t	h2d_bytes_total;
    uint64_t	reserved[2];
} mifsk_session_info;
int mifsk_session_info_get( const mifsk_session *s, mifsk_session_info *info );

/* ---- soft bits: the band magnitudes of every bit of every decoded frame -------- */

/* A second pass over frames a receive entry has written: what the loop makes `bits`, `confidence`
 * and `amplitude` of and then drops.  For stream s, frame j < min(d_nframes[s], frames_cap) and
 * bit k < cfg->expect_n_bits the window is x[a .. a + cfg->bit_nsamples) with
 * a = d_frames[s][j].start - d_origin[s] + cfg->bit_offset[k], where x[i] is the row's sample for
 * i < min(nsamples[s], stream_stride) and 0.0 beyond, whatever the memory holds there (flat
 * addressing).  d_mag[s][j][k] receives the two floats fsk_bit_analyze makes of that window
 * (fsk.c:107-169: the double sums in index order, hypotf, 2.0f / bit_nsamples) -- mark, then space;
 * bit k of d_rawbits[s][j] is mark > space (strict; a NaN gives 0), in time order, start and stop
 * bits included: the loop's shift, window and bit reversal have not been applied.  With an
 * all-'d' expect string fsk_frame_analyze's confidence pass over d_mag[s][j] gives the frame's
 * amplitude; with cfg->expect_data it gives its confidence, unless the frame is
 * MIFSK_FRAME_REFINED: that one keeps its coarse scan's confidence beside the fine scan's start
 * (minimodem.c:1357-1389), so the pass gives at least the frame's.
 *   A frame whose windows lie partly or wholly beyond the row's end -- an absurd start included
 * -- sees zeros there.  A frame with start < d_origin[s] refers to samples the caller no longer
 * holds: all its magnitudes are -1.0f and its rawbits 0.  Entries j >= d_nframes[s] are left
 * untouched.  PCM16 samples are (float)v / 32768.0f plus the --Xrxnoise term, mifsk_ingest_s16's
 * expression: the result is bit for bit that of mifsk_ingest_s16 and the float call.
 *   d_frames is caller data: whatever it holds, nothing outside nstreams * stream_stride elements
 * of d_samples is read and nothing outside the two output arrays is written.
 *   Frames of a MIFSK_IO_RING_EXACT call can be passed; they get the FLAT answer (where the loop
 * saw stale cells behind the stream's end, this pass sees zeros).
 *   Checked in this order, before any HIP call: -EINVAL for a NULL ctx, cfg, io, d_samples,
 * d_frames, d_nframes or d_mag; for nstreams <= 0 or frames_cap == 0; for an unknown kind, or
 * rxnoise != 0 with MIFSK_FEED_F32; for a base that is not 16-byte aligned or a stride that is no
 * multiple of 4 (float32) or 8 (PCM16); what mifsk_check_cfg says of cfg; -ENOTSUP for
 * cfg->auto_carrier_threshold > 0 -- with --auto-carrier a frame's bands are its episode's
 * (mifsk_episode.b_mark), and a table of bands per episode is a follow-up; -EINVAL for
 * frames_cap * cfg->expect_n_bits above 2^32 - 65 (a stream's cases are counted in 32 bits).
 * Asynchronous on `stream`; the context's tables are looked up as mifsk_demod_batch does. */
typedef struct mifsk_softbits_io {
    const void		*d_samples;	/* nstreams rows: float32, or PCM16 (kind)             */
    size_t		stream_stride;	/* elements between rows (16-byte aligned rows)        */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                  */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16                     */
    float		rxnoise;	/* S16 only: mifsk_ingest_s16's term; F32: must be 0   */
    const uint64_t	*d_origin;	/* stream index of each row's sample 0; NULL -> 0      */
    const mifsk_frame	*d_frames;	/* [nstreams][frames_cap], as the receive entries write */
    const uint32_t	*d_nframes;	/* [nstreams]; more than frames_cap is clamped         */
    size_t		frames_cap;
    float		*d_mag;		/* [nstreams][frames_cap][expect_n_bits][2]: mark, space */
    uint64_t		*d_rawbits;	/* [nstreams][frames_cap] or NULL: bit k = mark > space */
} mifsk_softbits_io;

int mifsk_frame_softbits( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_softbits_io *io, void *stream );

/* ---- a batch of fsk_detect_carrier() problems ------------------------------------ */

/* fsk_detect_carrier (fsk.c:543-581) on windows of every stream of a batch: "where is there a
 * tone, and in which band?" -- the question that comes before any decoding.  Window w of stream s
 * is x[a .. a + window) with a = first + w * hop (64 bits), where x is the row as
 * mifsk_frame_softbits defines it: valid length min(nsamples[s], stream_stride), PCM16 as
 * (float)v / 32768.0f plus the --Xrxnoise term (mifsk_ingest_s16's expression).  A window that
 * ends inside the valid length is evaluated; any other (the reference never calls the function on
 * a partial window, minimodem.c:1179-1190) gets d_band = MIFSK_CARRIER_NO_WINDOW and d_mag = 0, and
 * its spectrum row is left untouched.
 *   An evaluated window's d_band is the reference's return value: the band b in 1 .. nbands-1 with
 * the largest magnitude among those for which `mag < threshold` is false, the lowest such band on
 * a tie (the first strict maximum), never one whose magnitude is NaN, MIFSK_CARRIER_NONE if there
 * is none; d_mag is that band's magnitude (0.0f with NONE); d_spectrum[s][w][b] the magnitude of
 * every band b in 0 .. nbands-1.  The sums are the reference's as the oracle restates them: re, im
 * from 0.0, n ascending, re = fma((double)x[n], cos, re), im = fma((double)x[n], -sin, im) of the
 * angle 2 pi ((b n) mod fftsize) / fftsize from the context's spectrum table, then hypotf of the
 * two floats times 1.0f / ((float)window / 2.0f).
 *   Checked in this order, before any HIP call: -EINVAL for a NULL ctx, cfg, io, d_samples or
 * d_band; for nstreams <= 0 or nwindows == 0; for an unknown kind, or rxnoise != 0 with
 * MIFSK_FEED_F32; for a base that is not 16-byte aligned or a stride that is no multiple of 4
 * (float32) or 8 (PCM16); what mifsk_check_cfg says of cfg, and cfg->nbands < 2; for a window
 * above cfg->fftsize (asserted at fsk.c:547) or a default window of 0; for cfg->nbands * window
 * above 2^32 - 1 (b * n is reduced in 32 bits on the device); for nwindows * cfg->nbands above
 * 2^32 - 1 when d_spectrum is given.  Any threshold is accepted (the two comparisons decide), and
 * cfg->auto_carrier_threshold is not looked at.  Asynchronous on `stream`; the context's tables
 * are looked up as mifsk_frame_softbits does.  Whatever the arguments hold, nothing outside
 * nstreams * stream_stride elements of d_samples is read and nothing outside the three output
 * arrays is written. */
#define MIFSK_CARRIER_NONE       (-1)   /* no band reached the threshold (the reference's -1) */
#define MIFSK_CARRIER_NO_WINDOW  (-2)   /* the window does not lie wholly inside the row      */

typedef struct mifsk_carrier_io {
    const void		*d_samples;	/* nstreams rows: float32, or PCM16 (kind)             */
    size_t		stream_stride;	/* elements between rows (16-byte aligned rows)        */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                  */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16                     */
    float		rxnoise;	/* S16 only: mifsk_ingest_s16's term; F32: must be 0   */
    uint64_t		first;		/* start of window 0 in every row                      */
    uint32_t		window;		/* samples per window, 1 .. cfg->fftsize; 0 -> what
					   --auto-carrier uses: (unsigned)min(cfg->nsamples_per_bit,
					   (float)cfg->fftsize)  (minimodem.c:1179-1190)       */
    uint32_t		hop;		/* samples between window starts; 0 -> window          */
    uint32_t		nwindows;	/* windows per stream the outputs have room for        */
    float		threshold;	/* min_mag_threshold (fsk.c:570)                       */
    int32_t		*d_band;	/* [nstreams][nwindows]                                */
    float		*d_mag;		/* [nstreams][nwindows] or NULL                        */
    float		*d_spectrum;	/* [nstreams][nwindows][cfg->nbands] or NULL           */
} mifsk_carrier_io;			/* 88 bytes */

int mifsk_detect_carrier_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_carrier_io *io, void *stream );
/* host only: how many whole windows a row of nsamples holds -- 0 when first + window > nsamples,
 * else (nsamples - first - window) / hop + 1; hop == 0 means window */
uint64_t mifsk_carrier_windows( uint64_t nsamples, uint64_t first, uint32_t window, uint32_t hop );
/* host only: the tone pair --auto-carrier tunes to when it detects `band` (minimodem.c:1203-1219):
 * b_mark = band, b_space = band + b_shift, the frequencies band * cfg->band_width as
 * fsk_set_tones_by_bandshift makes them (outputs may be NULL).  -EINVAL for a NULL cfg, band < 1,
 * band >= nbands or b_shift == 0; -ERANGE when the space band falls outside 1 .. nbands-1, the
 * case in which the loop drops the detection. */
int mifsk_carrier_tones( const mifsk_rx_config *cfg, int band, unsigned *b_mark, unsigned *b_space,
	float *mark_f, float *space_f );

/* ---- channelizer: every carrier of a recording as a row the receive entries take ---- */

/* Mix -> low-pass -> decimate -> move to one output tone, for nchannels centres of every row of a
 * batch: what acts on the survey's answer when a recording holds more than one signal.  A row x
 * of valid length N = min(nsamples[s], stream_stride) ELEMENTS is real float32, real PCM16, or --
 * MIFSK_CHANNEL_COMPLEX -- interleaved I, Q of either (an element is then one complex sample);
 * PCM16 scalars are (float)v / 32768.0f, mifsk_ingest_s16's expression without the --Xrxnoise
 * term; every scalar is widened to double.
 *   With P = phase_steps, T = ntaps, h = taps, D = decim, q = centres[k] reduced to [0, P) (a
 * centre is in steps of fs_in / P Hz, negative allowed), r = out_centre likewise, the tables are
 * made on the host in double with the C library (every product rounded once, integers in 64 bits):
 *   G[k][t] = ( (double)h[t] * c, -((double)h[t] * s) ),  (s, c) = sincos(2 pi ((q t) mod P) / P)
 *   W[p]    = ( cos, sin ) of 2 pi p / P,  p < P
 * Output m of a row exists when m D + T <= N (whole windows only: mifsk_carrier_windows(N, 0, T,
 * D) of them).  re = im = 0.0, then for t ascending from 0 with n = m D + t:
 *   real x:     re = fma(x[n], G.re, re);   im = fma(x[n], G.im, im)
 *   xr + j xi:  re = fma(xr, G.re, re);  re = fma(-xi, G.im, re);
 *               im = fma(xr, G.im, im);  im = fma(xi, G.re, im)
 * and with p = (((r - q) mod P) * ((m D) mod P)) mod P, (C, S) = W[p]:
 *   out[m] = (float) fma(re, C, -(im * S))
 * the real part of the filtered, down-mixed signal moved up to r fs_in / P Hz, at fs_in / D samples
 * per second.  Gain is the taps' business (a real input wants taps that sum to 2); NaN and Inf
 * propagate as the arithmetic says.
 *   mifsk_channel_plan_create checks, in this order and before any HIP call: -EINVAL for a NULL
 * ctx, params or out; for a kind that is neither MIFSK_FEED_F32 nor MIFSK_FEED_S16, or flags beyond
 * MIFSK_CHANNEL_COMPLEX; for phase_steps outside 1 .. 2^20; for ntaps outside 1 .. 4096 or NULL
 * taps; for decim outside 1 .. 65535; for nchannels outside 1 .. 4096 or NULL centres; for
 * nchannels * ntaps above 2^22; for a centre with |centre| >= phase_steps.  Then it builds G and W
 * and uploads them once (-ENOMEM, -EIO).  The plan belongs to ctx's device and must be destroyed
 * before the context; it may be used from several threads and streams at once (it is read only).
 * mifsk_channel_plan_destroy SYNCHRONISES THE DEVICE (hipDeviceSynchronize: every stream) before
 * it frees the tables, so a launch still in flight never reads freed memory; keep plans for as
 * long as their parameters are in use rather than making one per call.
 *   mifsk_channelize_batch writes row s * nchannels + k of d_rows: out[m] for m < min(M_s,
 * nout_cap), 0.0f from there to out_stride, and that count into d_nout[s * nchannels + k] -- what
 * mifsk_demod_batch takes as d_samples and d_nsamples.  It checks, in this order and before any
 * HIP call: -EINVAL for a NULL plan, io, d_samples, d_rows or d_nout; for nstreams <= 0; for an
 * input base that is not 16-byte aligned or a stream_stride that is not a whole number of 16-byte
 * vectors (4 real floats, 8 real PCM16, 2 complex floats, 4 complex PCM16); for an output base
 * that is not 16-byte aligned, out_stride == 0, out_stride % 4 != 0 or out_stride above 2^32 - 4;
 * for nout_cap > out_stride; for nstreams * nchannels above 2^31 - 1.  Asynchronous on `stream`;
 * it allocates nothing and synchronises nothing.  Whatever the arguments hold, nothing outside
 * nstreams * stream_stride input elements is read and nothing outside the two output arrays is
 * written. */
#define MIFSK_CHANNEL_COMPLEX	1u	/* rows are interleaved I, Q */

typedef struct mifsk_channel_params {
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16 (the scalars)        */
    uint32_t		flags;		/* MIFSK_CHANNEL_COMPLEX                                */
    uint32_t		phase_steps;	/* P: 1 .. 2^20                                         */
    uint32_t		ntaps;		/* T: 1 .. 4096                                         */
    const float		*taps;		/* [ntaps], host                                        */
    uint32_t		decim;		/* D: 1 .. 65535                                        */
    uint32_t		nchannels;	/* K: 1 .. 4096, K * T <= 2^22                          */
    const int32_t	*centres;	/* [nchannels], host; |centre| < P, in steps of fs_in/P */
    int32_t		out_centre;	/* r, same unit                                         */
} mifsk_channel_params;			/* 48 bytes */

typedef struct mifsk_channel_plan mifsk_channel_plan;

typedef struct mifsk_channel_io {
    const void		*d_samples;	/* nstreams rows of the plan's kind                     */
    size_t		stream_stride;	/* elements between rows (16-byte aligned rows)         */
    const uint32_t	*d_nsamples;	/* elements per stream; NULL -> all = nsamples          */
    uint32_t		nsamples;
    int			nstreams;
    float		*d_rows;	/* [nstreams * nchannels][out_stride]                   */
    size_t		out_stride;	/* floats between output rows, % 4 == 0                 */
    uint32_t		nout_cap;	/* outputs per row at most, <= out_stride               */
    uint32_t		*d_nout;	/* [nstreams * nchannels]                               */
} mifsk_channel_io;			/* 64 bytes */

int  mifsk_channel_plan_create( mifsk_ctx *ctx, const mifsk_channel_params *params, mifsk_channel_plan **out );
void mifsk_channel_plan_destroy( mifsk_channel_plan *plan );
int  mifsk_channelize_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream );
/* host only, no context: channel k's G as the plan makes it, [ntaps][2] doubles.  -EINVAL for what
 * mifsk_channel_plan_create refuses of params, for k >= nchannels or a NULL g_out. */
int  mifsk_channel_table( const mifsk_channel_params *params, uint32_t k, double *g_out );
/* host only: ntaps Hamming-windowed sinc taps, 2 fc/fs sinc(2 fc/fs (t - (T-1)/2)) (0.54 - 0.46
 * cos(2 pi t / (T-1))) in double, scaled so that they sum to `gain`, each rounded to float once;
 * ntaps == 1 gives {gain}.  -EINVAL for ntaps outside 1 .. 4096, a NULL out, or a cutoff or rate
 * that is not positive and finite. */
int  mifsk_channel_taps( uint32_t ntaps, double cutoff_hz, double sample_rate, double gain, float *out );

/* ---- multiplexer: a batch of transmitted rows on the carriers of one capture ---- */

/* The channelizer's mirror on the transmit side: interpolate -> analytic signal -> move to the
 * channel's carrier -> sum, for nchannels baseband rows per stream.  Input row s * nchannels + k
 * is channel k of stream s: float32, exactly the d_out / out_stride / d_nsamples_out that
 * mifsk_tx_synthesize_batch writes; its valid length is N_k = min(nsamples[s * nchannels + k],
 * stream_stride) (a length above the stride is legal, as it is there).  The output is one row per
 * stream at fs_out = L fs_in: real, or -- MIFSK_MUX_COMPLEX -- interleaved I, Q (an element is then
 * one complex sample), float32 or PCM16 (kind).
 *   With P = phase_steps, T = ntaps, h = taps, L = interp, q[k] = centres[k] and r = in_centre,
 * both reduced to [0, P) (a centre is in steps of fs_out / P Hz, negative allowed), the tables are
 * made on the host in double with the C library (every product rounded once, integers in 64 bits):
 *   G[t] = ( (double)h[t] * c, (double)h[t] * s ),  (s, c) = sincos(2 pi ((r t) mod P) / P),  t < T
 *   W[p] = ( cos, sin ) of 2 pi p / P,  p < P
 * G is ONE table for all channels: the band-pass at the input rows' tone centre r, which keeps the
 * positive-frequency image of the zero-stuffed row (so h wants a cutoff below r fs_out / P Hz and
 * r well inside 0 .. fs_in / 2).
 *   Stream s has M_s = (Nmax_s - 1) L + T outputs (the last sample's whole filter tail), Nmax_s the
 * largest N_k of its rows; M_s = 0 when Nmax_s = 0; M_s is computed in 64 bits and cut at nout_cap.
 * Output n: o = oi = 0.0, then for k ascending:
 *   m = n div L, phi = n mod L, re = im = 0.0
 *   for j = 0, 1, ... while t = phi + j L < T, with i = m - j:
 *     if 0 <= i < N_k:  re = fma((double)x_k[i], G[t].re, re);  im = fma((double)x_k[i], G[t].im, im)
 *     (a term whose i lies outside the row is skipped, not multiplied by zero)
 *   if gains:  re = re * (double)gains[k];  im = im * (double)gains[k]
 *   p = (((q[k] - r) mod P) * (n mod P)) mod P,  (C, S) = W[p]
 *   o = fma(re, C, o);  o = fma(-im, S, o)
 *   with MIFSK_MUX_COMPLEX also:  oi = fma(re, S, oi);  oi = fma(im, C, oi)
 * out[n] = (float)o, and (float)oi beside it for complex rows: the sum over the channels, in channel
 * order, of each row's analytic signal moved from r to q[k].  With L > T the phases phi >= T have no
 * tap and give re = im = 0.0.  For PCM16 output (kind == MIFSK_FEED_S16) each float v becomes a
 * 16-bit value by the write conversion of oracle/shim/sndfile_shim.c: t = v * 32767.0f, t > 32767.0f
 * -> 32767.0f, t < -32768.0f -> -32768.0f, (int16_t)lrintf(t) (round to nearest even); a NaN gives
 * 0.  Elements from min(M_s, nout_cap) to out_stride are written as zero and d_nout[s] = min(M_s,
 * nout_cap).  Gain is the taps' business: G keeps one of the L images of one side of the spectrum,
 * so unit gain for a real output wants taps that sum to 2 L (mifsk_channel_taps(T, fc, fs_out,
 * 2 L)); a complex output is then the rows' analytic signal, of that same amplitude in I and in
 * Q.  gains are data (finite or not); NaN and Inf propagate as the arithmetic says.
 *   The sum over the channels of one output is ONE chain in channel order, and the sum over the
 * taps one chain in tap order: no f64 MFMA and no split of either over lanes (the reason is the
 * carrier survey's: a tree is another sum).
 *   mifsk_mux_plan_create checks, in this order and before any HIP call: -EINVAL for a NULL ctx,
 * params or out; for a kind that is neither MIFSK_FEED_F32 nor MIFSK_FEED_S16, or flags beyond
 * MIFSK_MUX_COMPLEX; for phase_steps outside 1 .. 2^20; for ntaps outside 1 .. 4096 or NULL taps;
 * for interp outside 1 .. 65535; for nchannels outside 1 .. 4096 or NULL centres; for a centre with
 * |centre| >= phase_steps; for |in_centre| >= phase_steps.  Then it builds G and W and uploads them
 * once (-ENOMEM, -EIO).  The plan belongs to ctx's device and must be destroyed before the context;
 * it is read only and may be used from several threads and streams at once.
 * mifsk_mux_plan_destroy has mifsk_channel_plan_destroy's rule: it SYNCHRONISES THE DEVICE before
 * it frees the tables.
 *   mifsk_multiplex_batch checks, in this order and before any HIP call: -EINVAL for a NULL plan,
 * io, d_samples, d_out or d_nout; for nstreams <= 0; for an input base that is not 16-byte aligned
 * or a stream_stride that is no multiple of 4; for an output base that is not 16-byte aligned,
 * out_stride == 0, out_stride not a whole number of 16-byte vectors of the output kind (4 real
 * floats, 8 real PCM16, 2 complex floats, 4 complex PCM16) or above 2^32 - 8; for nout_cap >
 * out_stride; for nstreams * nchannels above 2^31 - 1.  Asynchronous on `stream`; it allocates
 * nothing and synchronises nothing.  Whatever the arguments hold, nothing outside nstreams *
 * nchannels * stream_stride input floats is read and nothing outside the two output arrays is
 * written; nothing written is read back, and the outputs are plain vector stores. */
#define MIFSK_MUX_COMPLEX	1u	/* output rows are interleaved I, Q */

typedef struct mifsk_mux_params {
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16 (the OUTPUT scalars)  */
    uint32_t		flags;		/* MIFSK_MUX_COMPLEX                                     */
    uint32_t		phase_steps;	/* P: 1 .. 2^20                                          */
    uint32_t		ntaps;		/* T: 1 .. 4096                                          */
    const float		*taps;		/* [ntaps], host                                         */
    uint32_t		interp;		/* L: 1 .. 65535                                         */
    uint32_t		nchannels;	/* K: 1 .. 4096                                          */
    const int32_t	*centres;	/* [nchannels], host; |centre| < P, in steps of fs_out/P */
    int32_t		in_centre;	/* r, same unit; |r| < P                                 */
    const float		*gains;		/* [nchannels], host, or NULL: no gain step              */
} mifsk_mux_params;			/* 56 bytes */

typedef struct mifsk_mux_plan mifsk_mux_plan;

typedef struct mifsk_mux_io {
    const float		*d_samples;	/* [nstreams * nchannels][stream_stride]                 */
    size_t		stream_stride;	/* floats between input rows, % 4 == 0                   */
    const uint32_t	*d_nsamples;	/* [nstreams * nchannels]; NULL -> all = nsamples        */
    uint32_t		nsamples;
    int			nstreams;
    void		*d_out;		/* [nstreams][out_stride] elements of the plan's kind    */
    size_t		out_stride;	/* elements between output rows, whole 16-byte vectors   */
    uint32_t		nout_cap;	/* outputs per stream at most, <= out_stride             */
    uint32_t		*d_nout;	/* [nstreams]                                            */
} mifsk_mux_io;				/* 64 bytes */

int  mifsk_mux_plan_create( mifsk_ctx *ctx, const mifsk_mux_params *params, mifsk_mux_plan **out );
void mifsk_mux_plan_destroy( mifsk_mux_plan *plan );
int  mifsk_multiplex_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream );
/* host only, no context: G as the plan makes it, [ntaps][2] doubles.  -EINVAL for what
 * mifsk_mux_plan_create refuses of params, or a NULL g_out. */
int  mifsk_mux_table( const mifsk_mux_params *params, double *g_out );

/* ---- channel model: reproducible AWGN, gain and DC offset for a batch ---- */

/* The stage between transmitter and receiver: out = gain x + dc + sigma z for a batch of rows, z a
 * standard normal NOISE FIELD that is a pure function of (seed, stream index, sample index), made
 * of integer arithmetic and IEEE double operations only -- so a batch cut into pieces, sharded over
 * ranks or fed in slabs gets the noise of the whole batch, and a host can regenerate any noisy row
 * from a handful of numbers (tools/impair_ref.c restates all of this; the device equals it bit for
 * bit).
 *   The field z(seed, S, n), for a 64-bit seed, stream index S and sample index n.  Philox4x32-10
 * (Salmon et al., SC'11) supplies the words: key (k0, k1) = (lo32(seed), hi32(seed)), counter
 * (c0, c1, c2, c3) = (lo32(j), hi32(j), lo32(S), hi32(S)) with j = n >> 2; ten rounds, each
 *   p0 = 0xD2511F53 * c0,  p1 = 0xCD9E8D57 * c2                       (64-bit products)
 *   c = ( hi32(p1) ^ c1 ^ k0,  lo32(p1),  hi32(p0) ^ c3 ^ k1,  lo32(p0) )
 *   k0 += 0x9E3779B9,  k1 += 0xBB67AE85
 * (counter 0,0,0,0 under key 0,0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8).  The four words
 * w0 .. w3 of block j are the four normals of samples 4 j .. 4 j + 3, by Box-Muller:
 *   z[4j] = R(w0) C(w1),  z[4j+1] = R(w0) S(w1),  z[4j+2] = R(w2) C(w3),  z[4j+3] = R(w2) S(w3)
 * Every operation below is ONE IEEE double operation, rounded once; every a * b + c written fma is
 * one fused operation and nothing else is fused (both sides compile with -ffp-contract=off).
 *   R(w) = sqrt(-2 ln u), u = (w + 1) / 2^32:
 *     t = w + 1 (a 64-bit integer);  e = floor(log2 t);  m = (double)t * 2^-e (exact, in [1, 2))
 *     if m > 0x1.6a09e667f3bcdp+0:  m = m * 0.5,  e = e + 1
 *     f = m - 1.0;  s = f / (2.0 + f);  y = s * s
 *     p = 1.0 / 23.0;  for k = 10 down to 0:  p = fma(p, y, 1.0 / (2 k + 1))
 *     lnm = (2.0 * s) * p;  ln = fma((double)(e - 32), 0x1.62e42fefa39efp-1, lnm)
 *     R = sqrt(-2.0 * ln)
 *   (w = 0xFFFFFFFF gives -0.0; signs of zero are whatever the expressions give.)
 *   C(w), S(w) = cos, sin of 2 pi w / 2^32, by octant:
 *     q = w >> 29;  fr = w & 0x1FFFFFFF;  a = fr for even q, 0x20000000 - fr for odd q
 *     phi = 0x1.921fb54442d18p-1 * ((double)a * 2^-29);  y = phi * phi
 *     ps = -1.0 / 19!;  for k = 8 down to 0:  ps = fma(ps, y, (-1)^k / (2 k + 1)!);  sn = phi * ps
 *     pc = 1.0 / 20!;   for k = 9 down to 0:  pc = fma(pc, y, (-1)^k / (2 k)!);      cs = pc
 *     (every constant is one double division of +-1.0 by the factorial, an exact double)
 *     (C, S) for q = 0 .. 7:  (cs, sn) (sn, cs) (-sn, cs) (-cs, sn) (-cs, -sn) (-sn, -cs) (sn, -cs) (cs, -sn)
 *   z(0, 0, 0 .. 3) = 0x1.fb7665db1b649p-1, -0x1.d96d5ff0aec98p-1, -0x1.3c373dd6d9558p-1,
 * -0x1.eda3633cd971p-2.  |z| <= sqrt(64 ln 2) < 6.67.
 *   The element.  Row s, element i < W_s, with x the input scalar widened to double (PCM16:
 * (float)v / 32768.0f, mifsk_ingest_s16's expression without the --Xrxnoise term; 0.0 when d_samples
 * is NULL) and g, sg, d row s's gain, sigma and dc -- d_gain[s] / d_sigma[s] / d_dc[s] where that
 * array is given, else the scalar; floats widened to double:
 *   v = fma(g, x, d);  v = fma(sg, z(seed, first_stream + s, first_sample + i), v);  out = (float)v
 * (the index sums wrap in 64 bits).  For PCM16 output the float goes through the multiplexer's write
 * conversion: * 32767.0f, clamp to [-32768, 32767], lrintf to nearest even, NaN -> 0.
 * W_s = min(nsamples[s], stream_stride, out_stride), or min(nsamples[s], out_stride) without input
 * rows; elements from W_s to out_stride are written as zero.  Parameters are data, finite or not:
 * NaN and Inf propagate as the arithmetic says, and nothing is skipped for sigma == 0 (fma(1, -0.0,
 * 0) = +0.0: the arithmetic decides).
 *   IN PLACE -- d_out == d_samples with out_kind == kind and out_stride == stream_stride -- is
 * legal; any other overlap of the two arrays is undefined.
 *   mifsk_impair_batch checks, in this order and before any HIP call: -EINVAL for a NULL ctx, io or
 * d_out; for nstreams <= 0; for a kind or out_kind that is neither MIFSK_FEED_F32 nor
 * MIFSK_FEED_S16; for flags != 0; for first_sample % 4 != 0; when d_samples is given, for an input
 * base that is not 16-byte aligned or a stream_stride that is not whole 16-byte vectors of `kind`
 * (4 floats, 8 PCM16); for an output base that is not 16-byte aligned, out_stride == 0, out_stride
 * not whole 16-byte vectors of out_kind, or above 2^32 - 8.  Asynchronous on `stream`; it
 * allocates nothing and synchronises nothing.  Whatever the arguments hold, nothing outside nstreams
 * * stream_stride input elements is read and nothing outside nstreams * out_stride output elements
 * is written; nothing written is read back, and the outputs are plain vector stores. */
typedef struct mifsk_impair_io {
    const void		*d_samples;	/* nstreams rows of `kind`, or NULL: x = 0 (noise rows)  */
    size_t		stream_stride;	/* elements between input rows                           */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                    */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16: the input scalars    */
    uint32_t		out_kind;	/* ... the output scalars                                */
    void		*d_out;		/* [nstreams][out_stride]                                */
    size_t		out_stride;	/* elements between output rows, whole 16-byte vectors   */
    uint64_t		seed;
    uint64_t		first_stream;	/* the field's stream index of row 0 (a rank's shard)    */
    uint64_t		first_sample;	/* the field's sample index of column 0, % 4 == 0 (a piece) */
    const float		*d_gain;	/* [nstreams] device arrays, or NULL: the scalars below  */
    const float		*d_sigma;
    const float		*d_dc;
    float		gain;
    float		sigma;
    float		dc;
    uint32_t		flags;		/* 0 */
} mifsk_impair_io;			/* 120 bytes */

int   mifsk_impair_batch( mifsk_ctx *ctx, const mifsk_impair_io *io, void *stream );
/* host only: the sigma of a signal-to-noise ratio, (float)sqrt((a * a / 2) / 10^(snr_db / 10)) in
 * double: the power of a tone of amplitude a is a^2 / 2. */
float mifsk_impair_sigma( float amplitude, double snr_db );

/* ---- FM stage: batched NBFM discriminator and phase-exact FM modulator ---- */

/* Audio FSK on the air (Bell-202 as APRS, SAME, UIC-751-3) sits inside a narrow-band FM channel.
 * These two entries are the FM receiver in front of mifsk_demod_batch and the FM transmitter behind
 * mifsk_tx_synthesize_batch, for a batch of rows, made of integer arithmetic and IEEE double
 * operations only (tools/fm_ref.c restates all of this; the device equals it bit for bit).  Every
 * operation below is ONE IEEE double operation, rounded once; every a * b + c written fma is one
 * fused operation and nothing else is fused (both sides compile with -ffp-contract=off).
 *   The angle turn(y, x): the argument of x + i y in TURNS, [-0.5, 0.5] (csrc/mifsk_angle.h):
 *     ax = |x|;  ay = |y|;  sw = ay > ax;  mx = sw ? ay : ax;  mn = sw ? ax : ay
 *     if mx == 0.0:  a = 0.0
 *     else:
 *       big = mn > mx * 0x1.a827999fcef32p-2                          (tan(pi/8))
 *       u = big ? (mn - mx) / (mn + mx) : mn / mx                     (one division; |u| <= tan(pi/8))
 *       v = u * u;  p = -1.0 / 23.0;  for k = 10 down to 0:  p = fma(p, v, (-1)^k / (2 k + 1))
 *       r = u * p
 *       a = fma(r, 0x1.45f306dc9c883p-3, big ? 0.125 : 0.0)           (1 / (2 pi))
 *     if sw:  a = 0.25 - a
 *     if x < 0.0:  a = 0.5 - a
 *     if y < 0.0:  a = -a
 *   (every constant of the series is one double division of +-1.0 by the odd number.)  The series
 * stops at u^23: at u = tan(pi/8) the next term is 1.7e-12 turns.  Nothing is special-cased: a NaN
 * on either side gives a NaN, and so does Inf / Inf, because the arithmetic says so -- but for y a
 * NaN beside x = +-0.0, where the comparisons make mx = 0.0 and the answer 0.0.  turn(0, 1) = 0,
 * turn(1, 0) = 0.25, turn(0, -1) = 0.5, turn(-1, 0) = -0.25, turn(0, 0) = 0 (a zero of either sign on either side).
 *   THE DISCRIMINATOR.  Rows are interleaved I, Q, float32 (MIFSK_FEED_F32) or PCM16
 * (MIFSK_FEED_S16, a scalar is (float)v / 32768.0f); an element is one complex sample and strides
 * count elements, as in the channelizer.  Row s, n < W_s = min(nsamples[s], stream_stride,
 * out_stride), with (a, b) = (I[n], Q[n]) and (c, d) = (I[n - 1], Q[n - 1]) widened to double:
 *   re = fma(a, c, b * d);  im = fma(b, c, -(a * d));  out[n] = (float)((double)gain * turn(im, re))
 * For n = 0 the sample before is d_prev[s] (two floats) where that array is given, else (0, 0),
 * which gives 0.0.  d_last[s] (may be NULL) receives the row's last valid sample as two floats --
 * d_prev[s], or (0, 0), when W_s = 0 -- so a recording demodulated in pieces with one call's d_last
 * as the next call's d_prev is the whole recording's output, bit for bit.  d_last must not overlap
 * d_prev or the rows.  Elements from W_s to out_stride are written as zero.  mifsk_fm_gain's gain
 * puts full deviation at +-1.0.
 *   mifsk_fm_demod_batch checks, in this order and before any HIP call: -EINVAL for a NULL ctx, io,
 * d_samples or d_out; for nstreams <= 0; for a kind that is neither MIFSK_FEED_F32 nor
 * MIFSK_FEED_S16; for flags != 0; for an input base that is not 16-byte aligned or a stream_stride
 * that is not whole 16-byte vectors of complex elements (2 of float32, 4 of PCM16); for an output
 * base that is not 16-byte aligned, out_stride == 0, out_stride % 4 != 0, or above 2^32 - 8.
 * Asynchronous on `stream`; it allocates nothing and synchronises nothing.  Whatever the arguments
 * hold, nothing outside nstreams * stream_stride input elements (and d_prev) is read and nothing
 * outside nstreams * out_stride output elements and d_last is written; nothing written is read
 * back, and the outputs are plain vector stores. */
typedef struct mifsk_fm_demod_io {
    const void		*d_samples;	/* nstreams rows of interleaved I, Q of `kind`           */
    size_t		stream_stride;	/* complex elements between input rows                   */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                    */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		kind;		/* MIFSK_FEED_F32 / MIFSK_FEED_S16: the input scalars    */
    uint32_t		flags;		/* 0 */
    float		*d_out;		/* [nstreams][out_stride]                                */
    size_t		out_stride;	/* floats between output rows, % 4 == 0                  */
    const float		*d_prev;	/* [nstreams][2]: the sample before each row, or NULL: (0, 0) */
    float		*d_last;	/* [nstreams][2]: each row's last valid sample, or NULL  */
    float		gain;
    uint32_t		reserved;
} mifsk_fm_demod_io;			/* 80 bytes */

int   mifsk_fm_demod_batch( mifsk_ctx *ctx, const mifsk_fm_demod_io *io, void *stream );
/* host only: (float)(sample_rate / deviation_hz), the gain that puts +-deviation_hz at +-1.0 */
float mifsk_fm_gain( double sample_rate, double deviation_hz );

/*   THE MODULATOR.  The phase is an INTEGER, 2^48 to the turn, summed mod 2^64: a sum of integers
 * does not depend on its order, so the device scans it in parallel and still equals a serial loop.
 * Input rows are real float32, what mifsk_tx_synthesize_batch writes; output rows are interleaved
 * I, Q, float32 or PCM16 (out_kind).  Row s, i < W_s = min(nsamples[s], stream_stride, out_stride):
 *   d = fma((double)x[i], deviation, centre)            (turns per sample; both are doubles)
 *   q[i] = |d| < 16384.0 ? (int64)rint(d * 2^48) : 0    (to nearest even; false for a NaN)
 *   phase[n] = phase0[s] + q[0] + ... + q[n]  mod 2^64  (phase0 = 0 without d_phase0)
 *   w = (uint32)(phase[n] >> 16);  (C, S) = C(w), S(w) of the channel model above
 *   I = (float)(A * C),  Q = (float)(A * S),  A = (double)amplitude
 * For PCM16 output each float goes through the multiplexer's write conversion.  Elements from W_s
 * to out_stride are written as zero.  d_phase_out[s] (may be NULL) receives phase[W_s - 1], or
 * phase0[s] when W_s = 0, so pieces continue exactly; d_phase_out may be d_phase0.  mifsk_fm_step
 * gives `deviation` (and `centre`) from Hertz.
 *   mifsk_fm_modulate_batch checks, in this order and before any HIP call: -EINVAL for a NULL ctx,
 * io, d_samples or d_out; for nstreams <= 0; for an out_kind that is neither MIFSK_FEED_F32 nor
 * MIFSK_FEED_S16; for flags != 0; for an input base that is not 16-byte aligned or a stream_stride
 * % 4 != 0; for an output base that is not 16-byte aligned, out_stride == 0, out_stride not whole
 * 16-byte vectors of complex elements of out_kind (2 of float32, 4 of PCM16), or above 2^32 - 8.
 * Asynchronous on `stream`: three launches (sums of tiles of 2048 samples, one wave per row over the
 * sums, the tiles' outputs) around nstreams * ceil(out_stride / 2048) * 8 bytes of stream-ordered
 * scratch (-ENOMEM when there is none); it synchronises nothing, and no workgroup waits for another.
 * Nothing outside nstreams * stream_stride input elements (and d_phase0) is read and nothing
 * outside nstreams * out_stride output elements and d_phase_out is written; the outputs are plain
 * vector stores. */
typedef struct mifsk_fm_mod_io {
    const float		*d_samples;	/* nstreams rows of float32                              */
    size_t		stream_stride;	/* floats between input rows, % 4 == 0                   */
    const uint32_t	*d_nsamples;	/* per stream; NULL -> all = nsamples                    */
    uint32_t		nsamples;
    int			nstreams;
    uint32_t		out_kind;	/* MIFSK_FEED_F32 / MIFSK_FEED_S16: the output scalars   */
    uint32_t		flags;		/* 0 */
    void		*d_out;		/* [nstreams][out_stride] interleaved I, Q               */
    size_t		out_stride;	/* complex elements between output rows, whole 16-byte vectors */
    double		deviation;	/* turns per sample at x = 1.0                           */
    double		centre;		/* turns per sample at x = 0.0                           */
    const uint64_t	*d_phase0;	/* [nstreams]: the phase before each row, or NULL: 0     */
    uint64_t		*d_phase_out;	/* [nstreams]: each row's last phase, or NULL            */
    float		amplitude;
    uint32_t		reserved;
} mifsk_fm_mod_io;			/* 96 bytes */

int    mifsk_fm_modulate_batch( mifsk_ctx *ctx, const mifsk_fm_mod_io *io, void *stream );
/* host only: deviation_hz / sample_rate, Hertz as turns per sample */
double mifsk_fm_step( double deviation_hz, double sample_rate );

/* ---- several GPUs (SURVEY 8 e) -------------------------------------------- */

/* Streams are independent: device k of `world` owns the contiguous, balanced
 * range [*lo, *hi) of the batch.  The same arithmetic shards a multi-process
 * job (one process per GPU; the decoded bytes are then gathered over RCCL). */
void mifsk_shard_range( int nstreams, int rank, int world, int *lo, int *hi );

/* mifsk_demod_batch_host over several devices of ONE process: ctxs[k] (one
 * context per GPU, mifsk_ctx_create(&c, k)) takes range k of the batch; inputs
 * are copied to, and every output array is filled from, the device that owns the
 * stream -- no collective, the gather is the copy back.  Returns 0 or the first
 * failing device's error. */
int mifsk_demod_batch_host_multi( mifsk_ctx *const *ctxs, int nctx,
	const mifsk_rx_config *cfg, const mifsk_demod_io *io );

/* ---- host post-pass: frame bits -> text -------------------- */

/* The databits decoders main() plugs in behind the search (databits.h:49-92:
 * databits_decode_ascii8 / _baudot / _binary / _callerid / _uic_ground /
 * _uic_train).  O(1) per frame, stateful (Baudot shift, caller-ID message
 * buffer), byte-serial: host work over the frame bits the device gathered.
 * One object = the decoder's static state in the reference. */
typedef struct mifsk_databits mifsk_databits;

int  mifsk_databits_create( mifsk_databits **out, int decoder /* enum mifsk_decoder */ );
void mifsk_databits_destroy( mifsk_databits *d );
/* bfsk_databits_decode(0, 0, 0, 0): minimodem.c:1351 */
void mifsk_databits_reset( mifsk_databits *d );
/* bfsk_databits_decode(out, out_size, bits, n_databits): returns the bytes
 * produced (never more than out_size; the reference's 4096-byte buffer is the
 * usual size) */
unsigned mifsk_databits_decode( mifsk_databits *d, char *out, unsigned out_size,
	unsigned long long bits, unsigned n_databits );

/* bfsk_databits_encode(words, c): the 1 or 2 data words character c is sent as
 * (Baudot: a shift code first when needed; 0 = cannot be sent).  Transmit-side
 * state (the Baudot shift) lives in the same object. */
unsigned mifsk_databits_encode( mifsk_databits *d, unsigned *words_out /* [2] */, char c );

#define MIFSK_TEXT_PRINT_FILTER	1u	/* -p, --print-filter (minimodem.c:1451-1460) */
#define MIFSK_TEXT_QUIET	2u	/* -q, --quiet: no CARRIER / NOCARRIER lines  */

/* Everything the reference writes for one stream: stdout (decoded text) and
 * stderr ("### CARRIER ..." at each acquisition, "\n### NOCARRIER ..." with
 * the episode statistics, minimodem.c:253-291,1336-1348) from the frame data
 * bits in loop order (mifsk_demod_io.d_bits) and the episodes.  *out_len /
 * *err_len receive the full lengths; at most the capacities are written.
 * Returns 0, -ENOSPC when something was cut, -EINVAL. */
int mifsk_stream_text( const mifsk_rx_config *cfg,
	const uint64_t *bits, uint32_t nframes,
	const mifsk_episode *episodes, uint32_t nepisodes, unsigned flags,
	char *out, size_t out_cap, size_t *out_len,
	char *err, size_t err_cap, size_t *err_len );

/* ---- input side: the step before the path ------------------- */

/* RIFF/WAVE header of a `--rx --file` input: PCM16 or IEEE float32, mono
 * (what the reference reads through libsndfile in its tests;
 * simpleaudio-sndfile.c:113-160).  -EINVAL: not a WAV file; -ENOTSUP: a
 * format or channel count the receive path does not take. */
typedef struct mifsk_wav_info {
    unsigned	sample_rate;
    unsigned	channels;
    unsigned	bits_per_sample;
    int		is_float;
    size_t	data_offset;	/* bytes from the start of the file */
    size_t	nframes;
} mifsk_wav_info;

int mifsk_wav_parse( const void *file, size_t len, mifsk_wav_info *info );

/* sf_readf_float() on 16-bit input, for a whole batch on the device:
 * d_samples[s][i] = d_pcm[s][i] / 32768 (+ the --Xrxnoise term) for
 * i < nsamples[s], 0.0 up to stream_stride.  `rxnoise` is the option's factor
 * (0 = off): the reference adds (rand()/RAND_MAX - 0.5f) * 2 * factor with an
 * INTEGER division, i.e. the constant -factor (simpleaudio-sndfile.c:64-69;
 * tests/40-noise.test sweeps it as a DC offset).  Strides in elements;
 * fastest when pcm_stride % 8 == 0, stream_stride % 4 == 0 and both bases are
 * 16-byte aligned.  Asynchronous on `stream`. */
int mifsk_ingest_s16( mifsk_ctx *ctx, const int16_t *d_pcm, size_t pcm_stride,
	float *d_samples, size_t stream_stride, const uint32_t *d_nsamples, uint32_t nsamples,
	int nstreams, float rxnoise, void *stream );
/* the --Xrxnoise term alone, in place, for input that is already float */
int mifsk_ingest_rxnoise_f32( mifsk_ctx *ctx, float *d_samples, size_t stream_stride,
	const uint32_t *d_nsamples, uint32_t nsamples, int nstreams, float rxnoise, void *stream );

/* ---- a list of audio files -> one batch ----------------------- */

/* `minimodem --rx --file F <mode>` for N files at once (reference:
 * simpleaudio-sndfile.c:113-160 open, :42-74 read, minimodem.c:1014-1032): every
 * file's RIFF/WAVE header is parsed (PCM16 or float32, mono), the files are
 * grouped by (sample rate, sample format) -- the reference takes the sample rate
 * from the file and derives the whole configuration from it, so each group gets
 * its own mifsk_rx_config from `args` -- and each group runs through the host
 * pipeline above: worker threads pread() the RAW samples into pinned memory, they
 * cross PCIe as they are in the file, PCM16 is converted and --Xrxnoise added on
 * the device, and the receive loop runs over the chunk while the next one is read
 * and copied.  Results are owned by the returned object. */
typedef struct mifsk_file_result {
    int			error;		/* 0, or -errno: open/read failed, not a WAV
					   (-EINVAL), unsupported format (-ENOTSUP)  */
    mifsk_wav_info	info;
    const mifsk_rx_config *cfg;		/* the configuration this file was decoded
					   with (its sample rate); NULL on error     */
    uint32_t		nframes, nbytes, nepisodes;
    uint32_t		status;		/* MIFSK_STREAM_*                            */
    int32_t		carrier_band;	/* --auto-carrier (see mifsk_demod_io)       */
    uint32_t		reserved;
    const uint64_t	*bits;		/* [nframes] data bits of every frame        */
    const uint8_t	*bytes;		/* [nbytes]                                  */
    const mifsk_frame	*frames;	/* [nframes], or NULL without WANT_FRAMES    */
    const mifsk_episode	*episodes;	/* [nepisodes]                               */
} mifsk_file_result;

typedef struct mifsk_files mifsk_files;

#define MIFSK_FILES_WANT_FRAMES	0x1000u	/* keep the per-frame records too */

/* flags: MIFSK_IO_RING_EXACT / _ENGINE_* / MIFSK_FILES_*.  Returns 0 when the
 * batch ran (per-file failures are in mifsk_file_result.error), -errno when it
 * could not. */
int mifsk_demod_files( mifsk_ctx *ctx, const mifsk_modem_args *args,
	const char *const *paths, int nfiles, float rxnoise, unsigned flags, mifsk_files **out );
/* mifsk_demod_files for long recordings: header parsing, per-file errors and the result object
 * are mifsk_demod_files's, but every group -- the files of one sample rate and one sample format
 * -- is decoded as one batch of long recordings cut in time: the files are pread() into pinned
 * pieces that are copied to the group's device buffer, PCM16 is decoded by
 * mifsk_demod_long_batch_s16 and float32 by mifsk_ingest_rxnoise_f32 and mifsk_demod_long_batch.
 * params: NULL for the library's choices (its flags are ORed with the engine flags of `flags`).
 * flags: MIFSK_IO_ENGINE_* and MIFSK_FILES_WANT_FRAMES; MIFSK_IO_RING_EXACT is -ENOTSUP, before
 * any file is opened.  -EINVAL as mifsk_demod_files, before any HIP call. */
int mifsk_demod_files_long( mifsk_ctx *ctx, const mifsk_modem_args *args,
	const char *const *paths, int nfiles, float rxnoise, unsigned flags,
	const mifsk_time_split *params /* NULL: the library's choices */, mifsk_files **out );
/* file i's plan and verification figures; NULL for a file with an error and for an object made by
 * mifsk_demod_files */
const mifsk_time_split_stats *mifsk_files_time_split( const mifsk_files *f, int i );
int mifsk_files_count( const mifsk_files *f );
const mifsk_file_result *mifsk_files_get( const mifsk_files *f, int i );
const mifsk_host_stats *mifsk_files_stats( const mifsk_files *f );
void mifsk_files_free( mifsk_files *f );

/* ---- transmit side (test and benchmark input generator) ------------------ */

/* (simpleaudio_tone_init, simple-tone-generator.c:60-89, has no counterpart: the generator's
 * state is per call -- mifsk_tx_synthesize takes the table length and the magnitude itself.) */
/* fsk_transmit_stdin + simpleaudio_tone for one stream of data words
 * (minimodem.c:81-250, simple-tone-generator.c:106-175): returns the stream's
 * length in samples (also when out is NULL or too small), or -errno */
long mifsk_tx_synthesize( const mifsk_rx_config *cfg, const uint8_t *words, size_t nwords,
	unsigned sin_table_len, float amplitude, unsigned leading_silence, int as_s16,
	float *out, size_t out_cap );

/* The same generator for a whole batch on the device: stream s is
 * d_words[s][0 .. nwords[s]) (uniform `nwords` when d_nwords is NULL) behind
 * leading_silence[s] zero samples, written to d_out[s][..out_stride) with the rest
 * of the row zeroed; d_nsamples_out[s] receives its length (which may exceed
 * out_stride: the row is then cut).  sin_table_len == 0 is --lut=0 (a sinf per
 * sample: glibc's algorithm restated on the device, csrc/mifsk_sinf.h).
 * Bit-identical to mifsk_tx_synthesize.  Asynchronous on `stream`. */
int mifsk_tx_synthesize_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const uint8_t *d_words, size_t words_stride, const uint32_t *d_nwords, uint32_t nwords,
	int nstreams, unsigned sin_table_len, float amplitude,
	const uint32_t *d_leading_silence, uint32_t leading_silence, int as_s16,
	float *d_out, size_t out_stride, uint32_t *d_nsamples_out, void *stream );

#ifdef __cplusplus
}
#endif

#endif /* MIFSK_H */
