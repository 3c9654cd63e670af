// mifsk_device.h -- types shared by the host glue and the HIP kernels, and what the two
// engines' launchers share (the launch plan, the slice of a batch, occupancy, the chained launch).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "mifsk.h"

namespace mifsk {

// ---------------------------------------------------------------------------
// Shared-segment plan of one zig-zag scan with long bit windows (SCAN in the tiled
// instantiation of the wavefront engine; DESIGN.md "shared segments").
//
// All windows of one fsk_find_frame -- every candidate x every bit (fsk.c:199-254,
// 477-502) -- cover one contiguous span of the stream, and windows of neighbouring
// candidates overlap by most of their length.  The span is cut at every window
// edge (and long pieces once more, to balance the lanes) into SEGMENTS; each
// segment's two-bin partial DFT, phase origin at its own start, is computed ONCE,
// one lane per segment in at most two passes of lanes; a window is then the sum of
// its segments' partials, each rotated by the table entry of its offset inside the
// window.  Indices in POSITION order: a window's segments are seg[first .. first+count).
// Made on the host (fill_devcfg), relative to the search cursor.
// ---------------------------------------------------------------------------
constexpr int SEG_MAX = 128;		// segments per plan (two passes of lanes)
constexpr int SEGW_MAX = 128;		// windows per plan

struct SegPlan {
    uint32_t	valid;			// 0: this scan correlates every window by itself
    uint32_t	nseg, npass, nwin;	// nwin = candidates x bits, w = candidate (scan order) * n_bits + bit
    uint32_t	span_hi;		// every segment ends at or before cursor + span_hi
    uint32_t	pass_len[2];		// longest segment of the pass (its lock-step length)
    uint32_t	pass_min[2];		// shortest segment of the pass (groups below it need no mask)
    float	bound_c;		// |assembled - index order| <= bound_c * 2^-53 * sum |x| over the window
    uint32_t	seg_rel[SEG_MAX];	// segment start, relative to the cursor
    uint16_t	seg_len[SEG_MAX];
    uint16_t	slot_seg[SEG_MAX];	// pass * 64 + lane -> segment, 0xFFFF: idle lane
    uint16_t	win_first[SEGW_MAX];	// window -> its first segment ...
    uint16_t	win_count[SEGW_MAX];	// ... and how many
    // the same, packed as the kernel reads it (one word per lane and pass / per window):
    uint32_t	p_slot[SEG_MAX];	// pass * 64 + lane -> seg_rel (20 bits) | seg_len << 20
    uint32_t	p_win[SEGW_MAX];	// window -> first | count << 8 | (window start rel. to the cursor) << 16
    uint8_t	p_slot_seg[SEG_MAX];	// pass * 64 + lane -> segment, 0xFF: idle lane
};

// Everything a kernel needs, as one POD passed by value in the kernarg
// segment (so it lands in SGPRs / the scalar cache, uniform for the launch).
struct DevCfg {
    uint32_t	n_bits;			// expect_n_bits (<= 64)
    uint32_t	bit_nsamples;		// samples per bit window   (fsk.c:183)
    uint32_t	last_reach;		// bit_offset[n_bits-1] + bit_nsamples
    float	magscalar;		// 2.0f / bit_nsamples      (fsk.c:132)
    uint32_t	frame_nsamples;
    uint32_t	expect_nsamples;
    uint32_t	overscan;
    uint32_t	try_first[2], try_max[2], try_step[2], try_step_fine[2];
    float	conf_threshold;
    float	search_limit;
    uint32_t	n_data_bits;
    uint32_t	nstartbits;
    uint32_t	has_stopbits;
    uint32_t	msb_first;
    uint32_t	do_rx_sync;
    uint32_t	rx_one;
    uint64_t	sync_byte;
    uint32_t	skew;			// LDS slab row padding (see mifsk_kernels.hip)
    uint32_t	div_magic;		// floor(2^32 / bit_nsamples)
    uint32_t	lock_advance;		// cursor step of a frame locked at its first try
    uint32_t	la_magic;		// floor(2^32 / lock_advance)
    uint32_t	nbits_magic;		// floor(2^32 / n_bits)
    uint32_t	lock_back;		// slab row 0 sits this far before a locked frame's first try
    uint32_t	lat_linear;		// lattice windows all start on 16-byte boundaries of their region
    // the windows of consecutive locked frames tile one grid of bit lengths
    // (bit_offset[k] = k B, lock_advance = (n_bits - 1) B): the last window of a
    // frame IS the first window of the next, and a round of F frames has only
    // F (n_bits - 1) + 1 distinct windows
    uint32_t	lat_grid;
    uint32_t	b_mark;			// the plan's mark band (episodes report it)
    uint32_t	b_space, fftsize;	// (with b_mark: what the shared segments' rotation tables are made for)
    // closed form of the four zig-zag scans of the receive loop (fsk.c:477-484; ZigZag in
    // mifsk_devlib.h): up / down candidate counts of [0] coarse without carrier, [1] coarse with
    // carrier, [2] fine without, [3] fine with (minimodem.c:1236-1263,1366)
    uint32_t	zz_up[4], zz_down[4];
    uint32_t	bit_offset[MIFSK_MAX_FRAME_BITS];	// fsk.c:204
    // expect strings as bit masks, [0]=data [1]=sync: bit k of req_mask is set
    // when bit k of the frame is required ('0'/'1'), req_val holds its value
    uint64_t	req_mask[2];
    uint64_t	req_val[2];
    // shared-segment plans of the four scans (index as zz_up / zz_down); valid only for
    // the long-window modes the tiled instantiation runs.  [4]: the carrier-held coarse scan
    // and the fine scan that may follow it at the same cursor (minimodem.c:1265,1373) as ONE
    // plan -- windows 0 .. nwin(1)-1 are the coarse scan's, the fine scan's follow: the span is
    // read and summed once, the fine scan's windows are assembled from sums already there
    SegPlan	seg[5];
    uint32_t	seg_union_first_fine;	// [4]: index of the fine scan's first window
};

// twiddles: tw[4*n + {0,1,2,3}] = cos_mark, -sin_mark, cos_space, -sin_space
// of angle 2*pi*((b*n) mod fftsize)/fftsize, in double.

// (the planner: mifsk_plan.cpp)
void fill_devcfg( DevCfg &d, const mifsk_rx_config &c );

// floats per stream of a RING row: the reference's samplebuf plus what a search at its top
// may touch beyond (mifsk_ring_floats; the per-call scratch of MIFSK_IO_RING_EXACT)
size_t ring_row_floats( const mifsk_rx_config &c );

// entries (samples) of a twiddle table for bit windows of B samples: whole
// groups of 16 plus one group of look-ahead, never fewer than three groups
inline size_t tw_entries( unsigned B )
{
    const size_t n = ( ( (size_t)B + 15 ) & ~(size_t)15 ) + 16;
    return n < 48 ? 48 : n;
}

// Tuning overrides for experiments (MIFSK_ENGINE, MIFSK_WAVES_PER_CU, MIFSK_SV, MIFSK_LDS_PAD,
// MIFSK_LAT_ROUNDS, MIFSK_LAT_FMIN, MIFSK_CHAIN: all read by the launch planner, mifsk_plan.cpp):
// honoured only when MIFSK_EXPERIMENT is set in the environment, so that a stray variable cannot
// change what production launches.
inline const char *experiment_env( const char *name )
{
    return std::getenv("MIFSK_EXPERIMENT") != nullptr ? std::getenv(name) : nullptr;
}

// launchers (mifsk_kernels.hip); `stream` is a hipStream_t
int launch_find_frame_batch( const DevCfg &cfg, const DevCfg *d_cfg, const double *d_tw,
	const float *d_samples, const mifsk_search *d_problems,
	mifsk_search_result *d_results, int nproblems, void *stream );

// ---- what the launch planner (mifsk_plan.cpp) and the kernels agree on ----
constexpr int P_CAP = 64;	// candidate positions per batch (= one wave of lanes)
constexpr int W_CAP = 448;	// bit windows per batch (LDS scratch)
constexpr int STAGE_VEC = 10;	// float4 per thread per staging round
// the wavefront engine's LDS tile for long windows (mifsk_devlib.h, corr_global_tiled)
constexpr uint32_t TILE_K = 32u;
constexpr uint32_t TILE_ROW = TILE_K + 4u;
constexpr uint32_t TILE_FLOATS = 64u * TILE_ROW;
constexpr uint32_t kTileMinBit = 256u;			// bit lengths from here on may go through the tile
// NQ of demod_wave_kernel (mifsk_wave.hip) beside the bit lengths with a resident table
constexpr int kTiled = -1;
constexpr int kDirect = -2;
constexpr size_t kCntBytes = ( MIFSK_NCOUNTERS * sizeof(uint32_t) + 15u ) & ~(size_t)15;	// work counters, first in LDS
// the workgroup engine's LDS in front of its slab: offsetof(StreamLds, slab) (mifsk_kernels.hip)
constexpr size_t kWgLdsHeader = 2u * W_CAP * 8u + P_CAP * ( 8u + 4u + 4u + 4u ) + 16u + MIFSK_NCOUNTERS * 4u + 2u * 32u;

// Every instantiation of demod_wave_kernel<SV, NQ, ST, RA> there is.  The resumable ones (ST)
// have generic correlators only; mifsk_demod_slab runs them with RA, a chain by --auto-carrier.
// The name mifsk_demod_plan reports does not spell RA; the waves per SIMD are what the
// instantiation is compiled for (its __launch_bounds__).
#define MIFSK_WAVE_KERNELS(X)										\
    X(10, -1, true, true)	X(10, 0, true, true)	X(10, -2, true, true)				\
    X(4, 0, true, true)		X(4, -2, true, true)							\
    X(10, -1, true, false)	X(10, 0, true, false)	X(10, -2, true, false)				\
    X(4, 0, true, false)	X(4, -2, true, false)							\
    X(10, -1, false, true)	X(10, -1, false, false)		/* RTTY and slower */			\
    X(10, 10, false, true)	X(10, 10, false, false)		/* 1200 baud at 48 kHz */		\
    X(10, 5, false, true)	X(10, 5, false, false)		/* 2400 baud; 1200 baud at 24 kHz */	\
    X(10, 0, false, true)	X(10, 0, false, false)							\
    X(10, -2, false, true)	X(10, -2, false, false)							\
    X(4, 1, false, true)	X(4, 1, false, false)		/* 12000 baud */			\
    X(4, 0, false, true)	X(4, 0, false, false)							\
    X(4, -2, false, true)	X(4, -2, false, false)		/* SAME */

// Every instantiation of demod_kernel there is: X(waves per SIMD its registers allow, key: slab,
// Bell-202, resumable, then the template arguments as the reported name spells them).  ST: the
// resumable ones (mifsk_demod_slab, chained launches).
#define MIFSK_WG_KERNELS(X)										\
    X(4u, false, false, true,  false, 0, 3, true)	/* no slab: e.g. 0.5 baud */			\
    X(3u, true,  true,  true,  true, 10, 2, true)	/* Bell-202: two workers, resident table */	\
    X(4u, true,  false, true,  true, 0, 3, true)							\
    X(3u, true,  true,  false, true, 10, 2)								\
    X(4u, true,  false, false, true, 0, 3)								\
    X(4u, false, false, false, false, 0, 3)

constexpr size_t kLdsPerCu = 160 * 1024;

// workgroups of `workgroup_size` threads a CU holds at once: by their LDS and by the waves per
// SIMD (x 4 SIMDs) the instantiation's VGPR budget allows
inline uint32_t workgroups_per_cu( size_t lds_bytes, uint32_t waves_per_simd, uint32_t workgroup_size )
{
    const uint32_t by_lds = lds_bytes ? (uint32_t)( kLdsPerCu / lds_bytes ) : 32u;
    const uint32_t by_waves = ( waves_per_simd ? waves_per_simd : 8u ) * 4u * 64u
			    / ( workgroup_size ? workgroup_size : 64u );
    return by_lds < by_waves ? by_lds : by_waves;
}

// rows lo .. lo + count - 1 of a batch (`sample_bytes`: 2 for MIFSK_IO_HOST_S16 rows)
inline mifsk_demod_io io_rows( const mifsk_demod_io &io, size_t lo, int count, size_t sample_bytes = sizeof(float) )
{
    mifsk_demod_io o = io;
    o.nstreams = count;
    o.d_samples = (const float *)( (const char *)io.d_samples + lo * io.stream_stride * sample_bytes );
    if ( o.d_nsamples )	    o.d_nsamples += lo;
    if ( o.d_bytes )	    o.d_bytes += lo * io.frames_cap;
    if ( o.d_nbytes )	    o.d_nbytes += lo;
    if ( o.d_bits )	    o.d_bits += lo * io.frames_cap;
    if ( o.d_frames )	    o.d_frames += lo * io.frames_cap;
    if ( o.d_nframes )	    o.d_nframes += lo;
    if ( o.d_episodes )	    o.d_episodes += lo * io.episodes_cap;
    if ( o.d_nepisodes )    o.d_nepisodes += lo;
    if ( o.d_status )	    o.d_status += lo;
    if ( o.d_counters )	    o.d_counters += lo * MIFSK_NCOUNTERS;
    if ( o.d_carrier_band ) o.d_carrier_band += lo;
    return o;
}

struct WaveChain;
// what the host glue hands either engine's launcher besides the plan and io: the loop state of streams
// that arrive in pieces (mifsk_demod_slab) and what a chained launch needs
struct HostArgs {
    uint32_t	samplebuf_size;
    mifsk_stream_state *d_state;	// mifsk_demod_slab: state in / out (nullptr: one call = whole streams)
    const uint64_t *d_origin;
    bool	final;
    // what a plan that chains runs on; the caller holds whatever serialises the chain's users
    const WaveChain *chain;
};

// ---- one wavefront per stream (mifsk_wave.hip) ---------------------------

enum { LAT_NONE = 0u, LAT_LINEAR = 1u, LAT_DIRECT = 2u };	// how a LATTICE block gets at the samples

// launch geometry and run-time options of demod_wave_kernel (by value: SGPRs)
struct WaveGeom {
    uint32_t	mags_cap;	// LDS: (mark, space) magnitude slots
    uint32_t	slab_floats;	// LDS: floats in the sample slab
    uint32_t	slab_cap;	// samples a skewed SCAN slab holds (0: SCAN streams from global memory)
    uint32_t	tiled;		// the slab is a TILE_FLOATS tile: long windows come from global memory through it
    uint32_t	lat_mode;	// LAT_*
    uint32_t	lat_fmax;	// frames per LATTICE block, at most (<= 64)
    uint32_t	lat_fmin;	// ... and at least (one pass of lanes)
    uint32_t	round_wins;	// LINEAR: bit windows per staging round
    uint32_t	bufsize;	// the reference's samplebuf_size (minimodem.c:1063-1070)
    uint32_t	ring_exact;	// RING addressing (stale-cell semantics)
    uint32_t	ring_stride;	// floats per stream in the device-resident samplebuf
    // --auto-carrier (minimodem.c:1179-1220)
    uint32_t	autodetect;
    float	auto_threshold;
    float	nps;		// nsamples_per_scan = min(nsamples_per_bit, fftsize)
    int32_t	b_shift;	// space band = mark band + b_shift
    uint32_t	fftsize, nbands;
    uint32_t	tw_entries;	// samples per per-stream twiddle table
};

// ---- the launch plan (mifsk_plan.cpp).  What decides a launch: a plan is a pure function of these (and of the experiment knobs above).
struct PlanInputs {
    const DevCfg *cfg;
    int		ncu, nstreams;	// compute units of the device (<= 0: 256); the batch
    uint32_t	nsamples;	// io.nsamples: the rows' common length (0: per-stream lengths only)
    uint32_t	samplebuf_size;
    uint32_t	engine_flags;	// MIFSK_IO_ENGINE_*
    bool	ring_exact, autodetect;		// MIFSK_IO_RING_EXACT, --auto-carrier
    bool	has_state, has_counters;	// mifsk_demod_slab's loop state in / out; io.d_counters
};

// the workgroup engine's geometry: its workers and demod_kernel's geometry arguments
struct WgGeom {
    uint32_t	nworkers, slab_cap, lat_frames, lat_rounds, region_floats, region_cap, lat_mode;
    bool	use_slab;
};

// Everything either engine's launcher needs to know before it touches the device.
struct LaunchPlan {
    uint32_t	engine;			// MIFSK_IO_ENGINE_WAVE or _WORKGROUP
    uint32_t	kernel;			// index into the engine's list (MIFSK_WAVE_KERNELS / MIFSK_WG_KERNELS)
    const char	*kernel_name;		// as mifsk_demod_plan reports it
    uint32_t	waves_per_simd;		// what the instantiation is compiled for (its VGPR budget)
    uint32_t	workgroup_size, lds_bytes;	// threads and dynamic LDS per workgroup
    uint32_t	lattice_mode;		// LAT_*
    uint32_t	frames_per_block;	// LATTICE frames scored at once, at most
    bool	resumable;		// an instantiation with the state code (mifsk_demod_slab, chains)
    uint32_t	chain_groups, chain_chunks;	// chained launches (WaveChain): groups of streams x time chunks; 0 = one launch
    // the wavefront engine: the planned fields of the kernel's geometry (mags_cap .. round_wins;
    // the launcher fills the run-time ones) and the staging width
    struct { WaveGeom g; int sv; } wave;
    WgGeom	wg;
};

// the engine a batch runs on, and its plan: 0, or -ENOMEM / -EINVAL where nothing fits
int plan_launch( const PlanInputs &in, LaunchPlan &plan );

// Streams that arrive in pieces (mifsk_demod_slab) and chained launches: what a resumable
// instantiation of either engine's kernel needs beyond the batch itself.
// The plain instantiations ignore all of it.
struct ResumeArgs {
    mifsk_stream_state	*d_state;	// [nstreams] the loop's state between calls (NULL: one call = whole streams)
    const uint64_t	*d_origin;	// [nstreams] stream index of each row's first sample (NULL: 0)
    uint32_t		final;		// the rows end where the streams end
    uint32_t		limit;		// chained launch: this call sees the first `limit` samples of every
					// row (a row that ends before is complete); 0 = all
    uint32_t		append;		// chained launch: outputs continue behind the chunk before (state: n*_total)
};
// ... filled here and nowhere else: by the launchers for one launch over the caller's rows, by
// chain_enqueue for a chunk of a chained launch
inline ResumeArgs resume_args( mifsk_stream_state *d_state, const uint64_t *d_origin, bool final,
	uint32_t limit = 0u, uint32_t append = 0u )
{
    return ResumeArgs{d_state, d_origin, final ? 1u : 0u, limit, append};
}

struct WaveAuto {
    const double	*d_cs;		// [fftsize][2]: cos, -sin of 2 pi k / fftsize
    double		*d_tw_scratch;	// [nstreams][tw_entries][4]
    float		*d_ring;	// [nstreams][ring_stride], zero-initialised
    ResumeArgs		rs;
    // shared segments: the rotation factor of segment i of window w of scan `kind`, laid out
    // [i][w] so that the lanes of the assembly (lane = window) read consecutive entries:
    // d_rot[kind][(i * rot_stride[kind] + w) * 4 .. + 3] = table entry of the segment's offset
    // inside the window (NULL: gathered from the stream's own table -- --auto-carrier)
    const double	*d_rot[5];
    uint32_t		rot_stride[5];
};

// Chained launches.  A batch of more streams than the chip holds runs in rounds of serial
// chains of unequal length: while a round's stragglers finish, the slots the others left stay
// empty.  Cut in time instead -- G groups of streams x K chunks of every stream, each (group,
// chunk) one launch of the resumable kernel, a group's chunks in order on the group's own HIP
// stream -- the dispatcher fills those slots with the other groups' next chunk, and the idle
// tail shrinks to that of one chunk.  The context owns what this needs (mifsk_ctx.cpp).
struct WaveChain {
    enum { kMaxGroups = 3 };
    void		*streams[kMaxGroups];	// hipStream_t, non-blocking
    void		*ev_fork;		// hipEvent_t: the caller's stream at the call
    void		*ev_done[kMaxGroups];	// ... and each group's last chunk
    mifsk_stream_state	*d_state;		// [state_cap] the loop's state between chunks
    size_t		state_cap;
};

// Enqueue a batch as `groups` x `chunks` launches.  `launch(gio, lo, rs, gs)` enqueues the
// resumable kernel over the rows `gio` (those from row `lo` of the batch) on the group's stream
// `gs` with the resume arguments `rs`: state in / out, the first `limit` samples of every row
// (0: all), outputs appended behind the chunk before.  The caller's stream waits for all of it,
// whatever fails on the way.
template <class Launch>
int chain_enqueue( const WaveChain &ch, const mifsk_demod_io &io, uint32_t groups, uint32_t chunks,
	hipStream_t st, Launch launch )
{
    if ( (size_t)io.nstreams > ch.state_cap )
	return -12;
    hipEvent_t fork = (hipEvent_t)ch.ev_fork;
    if ( hipEventRecord(fork, st) != hipSuccess )
	return -5;
    // (a limit of 0 means "all samples": rows with per-stream lengths only are not cut in time)
    if ( io.nsamples == 0u )
	chunks = 1u;
    mifsk_demod_io gio[WaveChain::kMaxGroups];
    uint32_t glo[WaveChain::kMaxGroups];
    bool prepared = true;
    for ( uint32_t gi = 0; gi < groups; gi++ ) {
	hipStream_t gs = (hipStream_t)ch.streams[gi];
	// behind the caller's stream, and behind whatever the call before left on ANY group's
	// stream (its groups were other ranges of the state array)
	(void)hipStreamWaitEvent(gs, fork, 0);
	for ( uint32_t h = 0; h < (uint32_t)WaveChain::kMaxGroups; h++ )
	    if ( h != gi )
		(void)hipStreamWaitEvent(gs, (hipEvent_t)ch.ev_done[h], 0);
	const uint32_t lo = (uint32_t)( (uint64_t)io.nstreams * gi / groups );
	const uint32_t hi = (uint32_t)( (uint64_t)io.nstreams * ( gi + 1u ) / groups );
	glo[gi] = lo;
	gio[gi] = io_rows(io, lo, (int)( hi - lo ));
	if ( hi > lo
		&& hipMemsetAsync(ch.d_state + lo, 0, (size_t)( hi - lo ) * sizeof(mifsk_stream_state), gs) != hipSuccess )
	    prepared = false;		// (no early return: the caller's stream is joined below either way)
    }
    const uint32_t chunk = ( io.nsamples + chunks - 1u ) / chunks;
    for ( uint32_t k = 0; k < chunks && prepared; k++ ) {
	const bool last = k + 1u == chunks;
	const uint64_t lim = (uint64_t)( k + 1u ) * chunk;
	for ( uint32_t gi = 0; gi < groups; gi++ )
	    if ( gio[gi].nstreams > 0 )
		launch(gio[gi], glo[gi], resume_args(ch.d_state + glo[gi], nullptr, last,
			last ? 0u : ( lim > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lim ), 1u), (hipStream_t)ch.streams[gi]);
    }
    const bool launched = hipGetLastError() == hipSuccess && prepared;
    for ( uint32_t gi = 0; gi < groups; gi++ ) {
	(void)hipEventRecord((hipEvent_t)ch.ev_done[gi], (hipStream_t)ch.streams[gi]);
	(void)hipStreamWaitEvent(st, (hipEvent_t)ch.ev_done[gi], 0);
    }
    return launched ? 0 : -5;
}

// One launch of the plan's kernel over the caller's rows, or -- where the plan cuts the batch -- its
// chained launches (ha.chain: made by the caller).  `launch(rows, lo, rs, on)` as for chain_enqueue.
template <class Launch>
int launch_planned( const LaunchPlan &plan, const HostArgs &ha, const mifsk_demod_io &io, hipStream_t st, Launch launch )
{
    if ( plan.chain_groups )
	return ha.chain ? chain_enqueue(*ha.chain, io, plan.chain_groups, plan.chain_chunks, st, launch) : -22;
    launch(io, 0u, resume_args(ha.d_state, ha.d_origin, ha.final), st);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// what the host glue hands the wavefront engine's launcher besides that
struct WaveHostArgs : HostArgs {
    bool	ring_exact;
    uint32_t	ring_stride;
    float	*d_ring;
    bool	autodetect;
    float	auto_threshold;
    float	nps;
    int32_t	b_shift;
    uint32_t	fftsize, nbands;
    uint32_t	tw_entries;
    const double *d_cs;
    double	*d_tw_scratch;
    const double *d_rot[5];
    uint32_t	rot_stride[5];
};

int launch_demod_wave( const LaunchPlan &plan, const DevCfg *d_cfg, const double *d_tw,
	const mifsk_demod_io &io, const WaveHostArgs &ha, void *stream );
int launch_demod_batch( const LaunchPlan &plan, const DevCfg *d_cfg, const double *d_tw,
	const mifsk_demod_io &io, const HostArgs &ha, void *stream );

int launch_detect_carrier( const float *d_samples, unsigned nsamples,
	const double *d_cs /* [fftsize][2] */, unsigned fftsize, unsigned nbands,
	float *d_mags /* [nbands] */, void *stream );

// self-test of the short square root of band_mag2() (mifsk_kernels.hip); d_out: four counters
int launch_selftest_sqrt( uint64_t seed, uint32_t blocks, uint32_t per_thread, unsigned long long *d_out, void *stream );

// the HIP device a context is bound to (mifsk_ctx.cpp)
int ctx_device( const mifsk_ctx *ctx );

// What --Xrxnoise really adds to every sample: (0 - 0.5f) * (factor * 2), in float as at
// simpleaudio-sndfile.c:67-69 (`rand()/RAND_MAX` is an integer division, i.e. 0).  Shared by the
// ingest kernels (mifsk_ingest.hip) and the time split's PCM16 gather (mifsk_timesplit.hip).
inline float rxnoise_term( float factor )
{
    if ( factor == 0.0f )
	return 0.0f;
    const float f = factor * 2;
    return ( 0 - 0.5f ) * f;
}

// A sample as the loop sees it, from what arrives.  THE expressions: every kernel that converts
// or offsets samples calls these (ingest_s16_kernel, offset_f32_kernel, session_append_kernel,
// the time split's gather), so that a stream gives the same floats whichever way it comes in.
//   PCM16: value / 32768 (libsndfile's normalisation, a power of two: exact) + dc
//   float: x + dc, applied only where --Xrxnoise is given (x + 0.0f would turn -0.0f into +0.0f)
__device__ inline float sample_from_s16( int v, float dc )
{
    return (float)v / 32768.0f + dc;
}

__device__ inline float sample_from_f32( float x, float dc )
{
    return x + dc;
}

// ---- the resident session's rows (mifsk_ingest.hip) --------

// one record per stream of the table a feed uploads
struct SessionRow {
    uint64_t	src_off;	// the new samples start at fresh[src_off] (elements)
    uint64_t	origin;		// stream index of the destination row's first sample
    uint32_t	drop;		// samples at the front of the old row that the loop has passed
    uint32_t	keep;		// samples behind them that stay
    uint32_t	k;		// new samples
    uint32_t	reserved;
};

// new_rows[i][0 .. width) = old_rows[i][drop .. drop + keep) | the k new samples | 0.0, and
// d_lens[i] = keep + k, d_origin[i] = origin.  `s16`: fresh holds PCM16, else floats.  width and
// both strides are multiples of 4, both row arrays 16-byte aligned; old_rows may be NULL when no
// row keeps anything.  `stream` is a hipStream_t.
int launch_session_append( const float *old_rows, size_t old_stride, float *new_rows, size_t new_stride,
	uint32_t width, const void *fresh, bool s16, const SessionRow *d_table, uint32_t *d_lens,
	uint64_t *d_origin, int nstreams, float dc, void *stream );

} // namespace mifsk
