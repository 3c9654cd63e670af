// mifsk_capi.cpp -- the batch entry points of libmifsk.so's C ABI (include/mifsk.h).
//
// Host-side glue only: argument checks and marshalling between the context's tables
// (mifsk_ctx.cpp), the launch planner (mifsk_plan.cpp) and the launchers.  There is no CPU
// implementation of the signal path in this library: every entry point that produces a result
// launches a HIP kernel, and context creation fails with -ENODEV when no gfx950 device is
// available.  (The reference's five-function API over the same kernels: mifsk_legacy.cpp.)
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "fsk.h"
#include "mifsk.h"
#include "mifsk_device.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"

using mifsk::DevCfg;
using mifsk::Prepared;

static_assert(sizeof(mifsk_stream_state) == 96, "mifsk_stream_state is part of the ABI");

extern "C" int mifsk_abi_version( void ) { return MIFSK_ABI_VERSION; }

extern "C" size_t mifsk_abi_sizeof( const char *name )
{
    if ( !name )
	return 0;
#define MIFSK_SIZEOF(T) if ( std::strcmp(name, #T) == 0 ) return sizeof(T)
    MIFSK_SIZEOF(mifsk_modem_args);
    MIFSK_SIZEOF(mifsk_rx_config);
    MIFSK_SIZEOF(mifsk_search);
    MIFSK_SIZEOF(mifsk_search_result);
    MIFSK_SIZEOF(mifsk_frame);
    MIFSK_SIZEOF(mifsk_episode);
    MIFSK_SIZEOF(mifsk_demod_io);
    MIFSK_SIZEOF(mifsk_launch_info);
    MIFSK_SIZEOF(mifsk_pipeline_info);
    MIFSK_SIZEOF(mifsk_gather_info);
    MIFSK_SIZEOF(mifsk_session_result);
    MIFSK_SIZEOF(mifsk_session_info);
    MIFSK_SIZEOF(mifsk_scan_plan);
    MIFSK_SIZEOF(mifsk_host_stats);
    MIFSK_SIZEOF(mifsk_stream_state);
    MIFSK_SIZEOF(mifsk_wav_info);
    MIFSK_SIZEOF(mifsk_file_result);
    MIFSK_SIZEOF(mifsk_time_split);
    MIFSK_SIZEOF(mifsk_time_split_stats);
    MIFSK_SIZEOF(mifsk_softbits_io);
    MIFSK_SIZEOF(mifsk_carrier_io);
    MIFSK_SIZEOF(mifsk_channel_params);
    MIFSK_SIZEOF(mifsk_channel_io);
    MIFSK_SIZEOF(mifsk_mux_params);
    MIFSK_SIZEOF(mifsk_mux_io);
    MIFSK_SIZEOF(mifsk_impair_io);
    MIFSK_SIZEOF(mifsk_fm_demod_io);
    MIFSK_SIZEOF(mifsk_fm_mod_io);
    MIFSK_SIZEOF(fsk_plan);
#undef MIFSK_SIZEOF
    return 0;
}

extern "C" int mifsk_selftest_sqrt( mifsk_ctx *ctx, uint64_t seed, uint64_t nvalues, uint64_t counts[4] )
{
    if ( !ctx || !counts )
	return -EINVAL;
    HIP_OK(hipSetDevice(ctx->device));
    mifsk::DevMem<unsigned long long> d;
    if ( d.alloc(4) )
	return -EIO;
    int rc = hipMemset(d.p, 0, 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -EIO;
    const uint32_t per_thread = 4096;
    uint64_t blocks = ( nvalues + 256ull * per_thread - 1 ) / ( 256ull * per_thread );
    if ( blocks < 1 ) blocks = 1;
    if ( blocks > 0x7FFFFFFFull ) blocks = 0x7FFFFFFFull;
    if ( rc == 0 )
	rc = mifsk::launch_selftest_sqrt(seed, (uint32_t)blocks, per_thread, d.p, nullptr);
    unsigned long long h[4] = { 0, 0, 0, 0 };
    if ( rc == 0 && hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess )
	rc = -EIO;
    for ( int i = 0; i < 4; i++ )
	counts[i] = h[i];
    return rc;
}

// ---------------------------------------------------------------------------
// batch entry points
// ---------------------------------------------------------------------------

// the batch of a demodulating entry point that accepts the flags `accepted`
static int check_io( const mifsk_rx_config *cfg, const mifsk_demod_io *io, unsigned accepted )
{
    if ( io->nstreams < 0 || ( io->nstreams > 0 && !io->d_samples ) )
	return -EINVAL;
    if ( io->stream_stride % 4 != 0 || ( (uintptr_t)io->d_samples & 15u ) )
	return -EINVAL;		// rows must be 16-byte aligned (coalesced float4 staging)
    if ( ( io->d_bytes || io->d_bits || io->d_frames ) && io->frames_cap == 0 )
	return -EINVAL;
    if ( io->flags & ~accepted )
	return -EINVAL;
    // the workgroup engine has neither RING addressing nor the in-loop --auto-carrier
    if ( ( io->flags & MIFSK_IO_ENGINE_WORKGROUP )
	    && ( ( io->flags & ( MIFSK_IO_ENGINE_WAVE | MIFSK_IO_RING_EXACT ) ) || cfg->auto_carrier_threshold > 0.0f ) )
	return -EINVAL;
    return 0;
}

extern "C" int mifsk_find_frame_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const float *d_samples, const mifsk_search *d_problems,
	mifsk_search_result *d_results, int nproblems, void *stream )
{
    if ( !ctx || mifsk_check_cfg(cfg) || ( nproblems > 0 && ( !d_samples || !d_problems || !d_results ) ) )
	return -EINVAL;
    Prepared p;
    if ( int rc = mifsk::prepare(ctx, cfg, p) )
	return rc;
    return mifsk::launch_find_frame_batch(p.d, p.tables.d_cfg, p.d_tw, d_samples, d_problems, d_results,
					  nproblems, stream);
}

// what decides a batch's launch plan (mifsk_plan.cpp): the same for a launch and for mifsk_demod_plan
static mifsk::PlanInputs plan_inputs( const mifsk_ctx *ctx, const mifsk_rx_config *cfg, const DevCfg &d,
	const mifsk_demod_io &io, const mifsk_stream_state *d_state )
{
    return mifsk::PlanInputs{&d, ctx->ncu, io.nstreams, io.nsamples, cfg->samplebuf_size,
			     io.flags & ( MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE ), ( io.flags & MIFSK_IO_RING_EXACT ) != 0,
			     cfg->auto_carrier_threshold > 0.0f, d_state != nullptr, io.d_counters != nullptr};
}

// One launch of the plan or -- where it cuts the batch -- the chained launches, one chain at a
// time on the context's streams.
template <class Args>
static int launch_engine( mifsk_ctx *ctx,
	int (*launch)( const mifsk::LaunchPlan &, const DevCfg *, const double *, const mifsk_demod_io &, const Args &, void * ),
	const mifsk::LaunchPlan &plan, const Prepared &p, const mifsk_demod_io &io, Args &ha, void *stream )
{
    if ( !plan.chain_groups )
	return launch(plan, p.tables.d_cfg, p.d_tw, io, ha, stream);
    std::lock_guard<std::mutex> one(ctx->chain_lock);
    if ( int rc = mifsk::chain_prepare(ctx, (size_t)io.nstreams) )
	return rc;
    ha.chain = &ctx->chain.view;
    return launch(plan, p.tables.d_cfg, p.d_tw, io, ha, stream);
}

// One wavefront per stream (mifsk_wave.hip): --auto-carrier and RING addressing
// need per-call device scratch; it is allocated and freed in stream order (behind a chain's
// groups too: the caller's stream has joined them when the launcher returns), so
// concurrent calls on different streams never share it.
static int demod_batch_wave( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const Prepared &p, const mifsk::LaunchPlan &plan,
	const mifsk_demod_io *io, void *stream, mifsk_stream_state *d_state, const uint64_t *d_origin, bool final,
	float *d_ring_persistent )
{
    hipStream_t st = (hipStream_t)stream;
    const size_t ns = (size_t)io->nstreams;
    mifsk::WaveHostArgs ha = {};
    static_cast<mifsk::HostArgs &>(ha) = mifsk::HostArgs{cfg->samplebuf_size, d_state, d_origin, final, nullptr};
    ha.fftsize = (uint32_t)cfg->fftsize;
    ha.nbands = cfg->nbands;
    ha.tw_entries = (uint32_t)mifsk::tw_entries(cfg->bit_nsamples);
    ha.ring_exact = ( io->flags & MIFSK_IO_RING_EXACT ) != 0;
    ha.autodetect = cfg->auto_carrier_threshold > 0.0f;
    // (--auto-carrier retunes per stream: its rotation factors come from the stream's own table)
    if ( !ha.autodetect )
	for ( int k = 0; k < 5; k++ ) {
	    ha.d_rot[k] = p.tables.d_rot[k];
	    ha.rot_stride[k] = p.tables.rot_stride[k];
	}
    mifsk::StreamMem scratch_tw(st), scratch_ring(st);
    if ( ha.autodetect ) {
	// default negative shift, in the reference's float arithmetic (minimodem.c:1203-1206)
	int b_shift = - (float)( cfg->autodetect_shift + cfg->band_width / 2.0f ) / cfg->band_width;
	if ( cfg->inverted_freqs )
	    b_shift *= -1;
	if ( b_shift == 0 )
	    return -EINVAL;			// assert in fsk_set_tones_by_bandshift (fsk.c:587)
	if ( (unsigned long long)cfg->nbands * cfg->bit_nsamples > 0xFFFFFFFFull )
	    return -EINVAL;			// (band * n is reduced in 32 bits on the device)
	int rc = mifsk::get_cs(ctx, (unsigned)cfg->fftsize, &ha.d_cs);
	if ( rc )
	    return rc;
	ha.auto_threshold = cfg->auto_carrier_threshold;
	ha.nps = cfg->nsamples_per_bit > (float)cfg->fftsize ? (float)cfg->fftsize
							      : cfg->nsamples_per_bit;
	ha.b_shift = b_shift;
	if ( scratch_tw.alloc(ns * ha.tw_entries * 4 * sizeof(double)) )
	    return -ENOMEM;
	ha.d_tw_scratch = (double *)scratch_tw.p;
    }
    if ( ha.ring_exact ) {
	ha.ring_stride = (uint32_t)mifsk::ring_row_floats(*cfg);
	// mifsk_demod_slab_ring: the caller's buffer IS the reference's samplebuf between calls
	ha.d_ring = d_ring_persistent;
	if ( !ha.d_ring ) {
	    if ( scratch_ring.alloc(ns * ha.ring_stride * sizeof(float))
		    || hipMemsetAsync(scratch_ring.p, 0, ns * ha.ring_stride * sizeof(float), st) != hipSuccess )
		return -ENOMEM;
	    ha.d_ring = (float *)scratch_ring.p;
	}
    }
    return launch_engine(ctx, mifsk::launch_demod_wave, plan, p, *io, ha, stream);
}

// Plan once; the plan names the engine (the same choice everywhere, the same state record).  Over
// whole streams or, with d_state, over streams that arrive in pieces (d_ring: mifsk_demod_slab_ring's).
static int demod_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const Prepared &p, const mifsk_demod_io *io,
	void *stream, mifsk_stream_state *d_state = nullptr, const uint64_t *d_origin = nullptr, bool final = true,
	float *d_ring = nullptr )
{
    if ( io->nstreams <= 0 )
	return 0;
    mifsk::LaunchPlan plan;
    if ( int rc = mifsk::plan_launch(plan_inputs(ctx, cfg, p.d, *io, d_state), plan) )
	return rc;
    if ( plan.engine == MIFSK_IO_ENGINE_WAVE )
	return demod_batch_wave(ctx, cfg, p, plan, io, stream, d_state, d_origin, final, d_ring);
    mifsk::HostArgs ha = {cfg->samplebuf_size, d_state, d_origin, final, nullptr};
    return launch_engine(ctx, mifsk::launch_demod_batch, plan, p, *io, ha, stream);
}

extern "C" int mifsk_demod_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io, void *stream )
{
    if ( !ctx || !io || mifsk_check_cfg(cfg)
	    || check_io(cfg, io, MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE) )
	return -EINVAL;
    Prepared p;
    if ( int rc = mifsk::prepare(ctx, cfg, p) )
	return rc;
    return demod_batch(ctx, cfg, p, io, stream);
}

static_assert(sizeof(mifsk_scan_plan) == sizeof(mifsk::SegPlan), "mifsk_scan_plan mirrors SegPlan");

extern "C" int mifsk_scan_plan_get( const mifsk_rx_config *cfg, int kind, mifsk_scan_plan *out )
{
    if ( mifsk_check_cfg(cfg) || !out || kind < 0 || kind > 4 )
	return -EINVAL;
    DevCfg d;
    mifsk::fill_devcfg(d, *cfg);
    std::memcpy(out, &d.seg[kind], sizeof(*out));
    return 0;
}

// the same loop for streams that arrive in pieces: state in, state out (either engine: the
// same choice as mifsk_demod_batch makes, the same state record)
extern "C" int mifsk_demod_slab( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const mifsk_demod_io *io,
	mifsk_stream_state *d_state, const uint64_t *d_origin, int final, void *stream )
{
    if ( !ctx || !io || !d_state || mifsk_check_cfg(cfg)
	    || cfg->samplebuf_size < 2u		// (the loop refills half a buffer at a time)
	    || check_io(cfg, io, MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP) )	// flat addressing
	return -EINVAL;
    Prepared p;
    if ( int rc = mifsk::prepare(ctx, cfg, p) )
	return rc;
    return demod_batch(ctx, cfg, p, io, stream, d_state, d_origin, final != 0);
}

// floats per stream of the buffer mifsk_demod_slab_ring keeps the reference's samplebuf in
extern "C" size_t mifsk_ring_floats( const mifsk_rx_config *cfg )
{
    return mifsk_check_cfg(cfg) ? 0 : mifsk::ring_row_floats(*cfg);
}

// mifsk_demod_slab with the reference's buffer semantics (MIFSK_IO_RING_EXACT) for streams fed
// in pieces: the samplebuf cells -- stale ones behind samples_nvalid included -- persist in
// d_ring between the calls (minimodem.c:1150-1156)
extern "C" int mifsk_demod_slab_ring( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const mifsk_demod_io *io,
	mifsk_stream_state *d_state, const uint64_t *d_origin, float *d_ring, int final, void *stream )
{
    if ( !ctx || !io || !d_state || !d_ring || mifsk_check_cfg(cfg) || cfg->samplebuf_size < 2u
	    || check_io(cfg, io, MIFSK_IO_ENGINE_WAVE | MIFSK_IO_RING_EXACT) )	// (RING addressing is the wavefront engine's)
	return -EINVAL;
    Prepared p;
    if ( int rc = mifsk::prepare(ctx, cfg, p) )
	return rc;
    mifsk_demod_io rio = *io;
    rio.flags |= MIFSK_IO_RING_EXACT;
    return demod_batch(ctx, cfg, p, &rio, stream, d_state, d_origin, final != 0, d_ring);
}

// what mifsk_demod_batch would launch for this configuration and batch size
extern "C" int mifsk_demod_plan( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int nstreams,
	unsigned flags, mifsk_launch_info *out )
{
    return mifsk_demod_plan_ex(ctx, cfg, nstreams, 0xFFFFFFFFu, flags, out);
}

extern "C" int mifsk_demod_plan_ex( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int nstreams,
	uint32_t nsamples, unsigned flags, mifsk_launch_info *out )
{
    if ( !ctx || !out || mifsk_check_cfg(cfg) || nstreams < 0 )
	return -EINVAL;
    DevCfg d;
    mifsk::derive_cfg(ctx, *cfg, d);
    mifsk_demod_io io;
    std::memset(&io, 0, sizeof(io));
    io.nstreams = nstreams;
    io.nsamples = nsamples;
    io.flags = flags;
    mifsk::LaunchPlan plan;
    if ( int rc = mifsk::plan_launch(plan_inputs(ctx, cfg, d, io, nullptr), plan) )
	return rc;
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", plan.kernel_name);
    out->engine = plan.engine;
    out->workgroup_size = plan.workgroup_size;
    out->lds_bytes_per_workgroup = plan.lds_bytes;
    out->workgroups_per_cu = mifsk::workgroups_per_cu(plan.lds_bytes, plan.waves_per_simd, plan.workgroup_size);
    out->lattice_mode = plan.lattice_mode;
    out->frames_per_block = plan.frames_per_block;
    out->compute_units = (uint32_t)ctx->ncu;
    out->chain_groups = plan.chain_groups;
    out->chain_chunks = plan.chain_chunks;
    return 0;
}

// ---------------------------------------------------------------------------
// several devices, one process: streams are independent, so context k (one per
// GPU) takes the contiguous range mifsk_shard_range(nstreams, k, nctx) and the
// "gather" is each device's copy back into the caller's arrays -- no collective.
// (One process per GPU with an RCCL gather of the decoded bytes is the other
// arrangement: minimodem_amd.ByteGatherer, bench.py --gpus N.)
// ---------------------------------------------------------------------------

extern "C" void mifsk_shard_range( int nstreams, int rank, int world, int *lo, int *hi )
{
    if ( world <= 0 ) world = 1;
    if ( nstreams < 0 ) nstreams = 0;
    const int q = nstreams / world, r = nstreams % world;
    const int a = rank * q + ( rank < r ? rank : r );
    if ( lo ) *lo = a;
    if ( hi ) *hi = a + q + ( rank < r ? 1 : 0 );
}

extern "C" int mifsk_demod_batch_host_multi( mifsk_ctx *const *ctxs, int nctx,
	const mifsk_rx_config *cfg, const mifsk_demod_io *hio )
{
    if ( !ctxs || nctx <= 0 || !hio || hio->nstreams < 0 )
	return -EINVAL;
    for ( int k = 0; k < nctx; k++ )
	if ( !ctxs[k] )
	    return -EINVAL;
    std::vector<int> rcs((size_t)nctx, 0);
    std::vector<std::thread> workers;
    for ( int k = 0; k < nctx; k++ ) {
	int lo = 0, hi = 0;
	mifsk_shard_range(hio->nstreams, k, nctx, &lo, &hi);
	if ( hi == lo )
	    continue;
	const mifsk_demod_io io = mifsk::io_rows(*hio, (size_t)lo, hi - lo,
						 ( hio->flags & MIFSK_IO_HOST_S16 ) ? 2u : 4u);
	mifsk_ctx *ctx = ctxs[k];
	int *rcp = &rcs[(size_t)k];
	// one host thread per device: the HIP "current device" is per thread, so
	// the per-device copies, launch and synchronisation proceed side by side
	workers.emplace_back([ctx, cfg, io, rcp]() { *rcp = mifsk_demod_batch_host(ctx, cfg, &io); });
    }
    for ( std::thread &t : workers )
	t.join();
    for ( int rc : rcs )
	if ( rc )
	    return rc;
    return 0;
}
