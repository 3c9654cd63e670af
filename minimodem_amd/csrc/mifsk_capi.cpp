// mifsk_capi.cpp -- the C ABI of libmifsk.so (include/fsk.h, include/mifsk.h).
//
// Host-side glue only: contexts, twiddle tables, argument marshalling, and the
// reference-compatible five-function API layered over the same kernels as the
// batch entry points.  There is no CPU implementation of the signal path in
// this library: every entry point that produces a result launches a HIP kernel,
// and context creation fails with -ENODEV when no gfx950 device is available.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "fsk.h"
#include "mifsk.h"
#include "mifsk_device.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif



using mifsk::DevCfg;

static_assert(sizeof(mifsk_stream_state) == 96, "mifsk_stream_state is part of the ABI");



// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------

int mifsk::ctx_device( const mifsk_ctx *ctx ) { return ctx->device; }

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

extern "C" int mifsk_ctx_create( mifsk_ctx **out, int device )
{
    if ( !out )
	return -EINVAL;
    *out = nullptr;
    int ndev = 0;
    if ( hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 ) {
	fprintf(stderr, "mifsk: no HIP device available (this library has no CPU path)\n");
	return -ENODEV;
    }
    if ( device >= 0 ) {
	if ( device >= ndev )
	    return -ENODEV;
	HIP_OK(hipSetDevice(device));
    } else {
	HIP_OK(hipGetDevice(&device));
    }
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    if ( std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 ) {
	fprintf(stderr, "mifsk: device %d is %s; the kernels are built for gfx950 only\n",
		device, prop.gcnArchName);
	return -ENODEV;
    }
    mifsk_ctx *ctx = new (std::nothrow) mifsk_ctx();
    if ( !ctx )
	return -ENOMEM;
    ctx->device = device;
    ctx->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    std::snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
    *out = ctx;
    return 0;
}

extern "C" void mifsk_ctx_destroy( mifsk_ctx *ctx )
{
    if ( !ctx )
	return;
    for ( TwEntry &e : ctx->tables )
	(void)hipFree(e.d_tw);
    for ( CfgEntry &e : ctx->configs ) {
	(void)hipFree(e.dev);
	for ( double *r : e.d_rot )
	    if ( r ) (void)hipFree(r);
    }
    if ( ctx->host )
	mifsk::host_work_destroy(ctx->host);
    {
	for ( void *st : ctx->chain.streams )
	    if ( st ) {
		(void)hipStreamSynchronize((hipStream_t)st);
		(void)hipStreamDestroy((hipStream_t)st);
	    }
	for ( void *e : ctx->chain.ev_done )
	    if ( e ) (void)hipEventDestroy((hipEvent_t)e);
	if ( ctx->chain.ev_fork ) (void)hipEventDestroy((hipEvent_t)ctx->chain.ev_fork);
	if ( ctx->chain.d_state ) (void)hipFree(ctx->chain.d_state);
    }
    delete ctx;
}

extern "C" const char *mifsk_ctx_device_name( const mifsk_ctx *ctx )
{
    return ctx ? ctx->name : "";
}

// cos, -sin of an angle as the oracle's tables hold them (ofsk_twiddle, and the spectrum table
// of ofsk_detect_carrier): its cos(ang) and -sin(ang) are compiled into ONE sincos() call, and the
// C library's sincos() is not its sin(): at 2 pi 198 / 240, for one, the two sines differ in the
// last place.  Separate calls made three entries of the Bell-202 table differ from the oracle's by
// an ulp -- invisible once a sum is rounded to float, but not "the oracle's sums"
// (tests/test_gpu_correlators.py compares the doubles).
static inline void cos_msin( double ang, double w[2] )
{
    double s, c;
    ::sincos(ang, &s, &c);
    w[0] = c;
    w[1] = -s;
}

// exp(-2 pi i b n / N): the angle is reduced exactly in integers first
static inline void twiddle( unsigned b, unsigned n, unsigned fftsize, double w[2] )
{
    const unsigned long long k = ( (unsigned long long)b * n ) % fftsize;
    cos_msin(2.0 * M_PI * (double)k / (double)fftsize, w);
}

// The caches are bounded: the legacy API makes a DevCfg per window shape and a twiddle
// table per tone pair it is re-tuned to (fsk_set_tones_by_bandshift).  Called at the top
// of every entry point that launches, BEFORE it takes the gate: when a cache has outgrown
// its bound, wait until no call is between lookup and launch (exclusive gate), let the
// device finish what is running, and drop everything -- the next lookups rebuild what is
// still in use.
static void cache_gc( mifsk_ctx *ctx )
{
    constexpr size_t kMaxConfigs = 64, kMaxTables = 64, kMaxTableBytes = 64u << 20;
    {
	std::lock_guard<std::mutex> g(ctx->lock);
	if ( ctx->configs.size() < kMaxConfigs && ctx->tables.size() < kMaxTables
		&& ctx->table_bytes < kMaxTableBytes )
	    return;
    }
    std::unique_lock<std::shared_mutex> x(ctx->gate);
    std::lock_guard<std::mutex> g(ctx->lock);
    // (another caller may have flushed while this one waited for the gate)
    if ( ctx->configs.size() < kMaxConfigs && ctx->tables.size() < kMaxTables
	    && ctx->table_bytes < kMaxTableBytes )
	return;
    (void)hipDeviceSynchronize();
    for ( CfgEntry &e : ctx->configs ) {
	(void)hipFree(e.dev);
	for ( double *r : e.d_rot )
	    if ( r ) (void)hipFree(r);
    }
    ctx->configs.clear();
    for ( TwEntry &e : ctx->tables )
	(void)hipFree(e.d_tw);
    ctx->tables.clear();
    ctx->table_bytes = 0;
}

static int get_twiddles( mifsk_ctx *ctx, const TwKey &key, const double **d_out )
{
    std::lock_guard<std::mutex> g(ctx->lock);
    for ( const TwEntry &e : ctx->tables )
	if ( e.key == key ) {
	    *d_out = e.d_tw;
	    return 0;
	}
    // zero-padded: the workgroup kernel consumes the table in chunks of 8 (and
    // fetches one half chunk ahead), the wavefront kernel in groups of 16 (one
    // group ahead, and keeps groups 0..2 resident): mifsk_tw_entries()
    const size_t n = mifsk::tw_entries(key.bit_nsamples);
    std::vector<double> h(4 * ( n ? n : 8 ), 0.0);
    for ( unsigned i = 0; i < key.bit_nsamples; i++ ) {
	twiddle(key.b_mark, i, key.fftsize, &h[4 * (size_t)i]);
	twiddle(key.b_space, i, key.fftsize, &h[4 * (size_t)i + 2]);
    }
    double *d = nullptr;
    HIP_OK(hipMalloc(&d, h.size() * sizeof(double)));
    if ( hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ) {
	(void)hipFree(d);
	return -EIO;
    }
    ctx->tables.push_back(TwEntry{key, d});
    ctx->table_bytes += h.size() * sizeof(double);
    *d_out = d;
    return 0;
}

static int get_devcfg( mifsk_ctx *ctx, const DevCfg &d, const DevCfg **d_out, CfgEntry *entry_out = nullptr )
{
    std::lock_guard<std::mutex> g(ctx->lock);
    for ( const CfgEntry &e : ctx->configs )
	if ( std::memcmp(&e.host, &d, sizeof(DevCfg)) == 0 ) {
	    *d_out = e.dev;
	    if ( entry_out ) *entry_out = e;		// (a copy: the vector may grow under another caller)
	    return 0;
	}
    DevCfg *dev = nullptr;
    HIP_OK(hipMalloc(&dev, sizeof(DevCfg)));
    if ( hipMemcpy(dev, &d, sizeof(DevCfg), hipMemcpyHostToDevice) != hipSuccess ) {
	(void)hipFree(dev);
	return -EIO;
    }
    CfgEntry ce;
    ce.host = d;
    ce.dev = dev;
    size_t rot_bytes = 0;
    for ( int k = 0; k < 5; k++ )
	ce.d_rot[k] = nullptr;
    // shared segments: every window's rotation factors, [segment of the window][window]
    for ( int k = 0; k < 5; k++ ) {
	ce.d_rot[k] = nullptr;
	ce.rot_stride[k] = 0;
	const mifsk::SegPlan &sp = d.seg[k];
	if ( !sp.valid )
	    continue;
	unsigned cmax = 0;
	for ( unsigned w = 0; w < sp.nwin; w++ )
	    cmax = sp.win_count[w] > cmax ? sp.win_count[w] : cmax;
	const unsigned stride = ( sp.nwin + 63u ) & ~63u;
	// (zero rows beyond the longest window's: Wave::seg_correlate walks the rows with a running
	// pointer, four segments a turn, and where two lanes share a window -- every other row each --
	// up to 2 x 3 + 1 rows beyond the last)
	std::vector<double> h((size_t)( ( cmax + 12u + 3u ) & ~3u ) * stride * 4, 0.0);
	for ( unsigned w = 0; w < sp.nwin; w++ )
	    for ( unsigned i = 0; i < sp.win_count[w]; i++ ) {
		const unsigned off = sp.seg_rel[sp.win_first[w] + i] - ( sp.p_win[w] >> 16 );
		double *t = &h[( (size_t)i * stride + w ) * 4];
		twiddle(d.b_mark, off, d.fftsize, t);
		twiddle(d.b_space, off, d.fftsize, t + 2);
	    }
	if ( hipMalloc(&ce.d_rot[k], h.size() * sizeof(double)) != hipSuccess
		|| hipMemcpy(ce.d_rot[k], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ) {
	    // nothing of a half-made entry stays behind
	    for ( int j = 0; j <= k; j++ )
		if ( ce.d_rot[j] ) (void)hipFree(ce.d_rot[j]);
	    (void)hipFree(dev);
	    return -ENOMEM;
	}
	ce.rot_stride[k] = stride;
	rot_bytes += h.size() * sizeof(double);
    }
    ctx->table_bytes += rot_bytes;
    ctx->configs.push_back(ce);
    *d_out = dev;
    if ( entry_out ) *entry_out = ce;
    return 0;
}

// cos / -sin of 2 pi k / N for k < N (the spectrum table of fsk_detect_carrier), one per
// FFT size seen; like the other tables it is only ever freed by cache_gc()
int mifsk::get_cs( mifsk_ctx *ctx, unsigned N, const double **d_out )
{
    std::lock_guard<std::mutex> g(ctx->lock);
    for ( const TwEntry &e : ctx->tables )
	if ( e.key == TwKey{N, 0u, 0u, 0u} ) {		// (bit_nsamples 0: never a bit table's key)
	    *d_out = e.d_tw;
	    return 0;
	}
    std::vector<double> h(2 * (size_t)N);
    for ( unsigned k = 0; k < N; k++ ) {
	cos_msin(2.0 * M_PI * (double)k / (double)N, &h[2 * (size_t)k]);
    }
    double *d = nullptr;
    if ( hipMalloc(&d, h.size() * sizeof(double)) != hipSuccess )
	return -ENOMEM;
    if ( hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ) {
	(void)hipFree(d);
	return -ENOMEM;
    }
    ctx->tables.push_back(TwEntry{TwKey{N, 0u, 0u, 0u}, d});
    ctx->table_bytes += h.size() * sizeof(double);
    *d_out = d;
    return 0;
}

// fill_devcfg through the context's small cache (keyed by the configuration's bytes: two equal
// byte strings are equal configurations; unequal padding only costs a miss)
static void derive_cfg( mifsk_ctx *ctx, const mifsk_rx_config &cfg, DevCfg &d )
{
    {
	std::lock_guard<std::mutex> g(ctx->lock);
	for ( const mifsk_ctx::DerivedCfg &e : ctx->derived )
	    if ( std::memcmp(&e.key, &cfg, sizeof(cfg)) == 0 ) {
		d = e.d;
		return;
	    }
    }
    mifsk::fill_devcfg(d, cfg);
    std::lock_guard<std::mutex> g(ctx->lock);
    // (another caller with the same configuration may have filled it in while this one derived:
    // keep one entry per key)
    for ( const mifsk_ctx::DerivedCfg &e : ctx->derived )
	if ( std::memcmp(&e.key, &cfg, sizeof(cfg)) == 0 )
	    return;
    constexpr size_t kKeep = 8;
    if ( ctx->derived.size() < kKeep ) {
	ctx->derived.push_back(mifsk_ctx::DerivedCfg{cfg, d});
    } else {
	ctx->derived[ctx->derived_next % kKeep] = mifsk_ctx::DerivedCfg{cfg, d};
	ctx->derived_next++;
    }
}

// ---------------------------------------------------------------------------
// batch entry points
// ---------------------------------------------------------------------------

// What every launching entry point does once its own arguments are checked: bind the device,
// collect the caches if they are due, take the gate, look the tables up.  The gate stays held
// (shared) as long as this object lives: from the lookup until the caller has enqueued.
struct Prepared {
    std::shared_lock<std::shared_mutex> gate;
    DevCfg		d;
    const DevCfg	*d_cfg = nullptr;
    const double	*d_tw = nullptr;
    CfgEntry		tables;
};

static int prepare( mifsk_ctx *ctx, const mifsk_rx_config *cfg, Prepared &p )
{
    HIP_OK(hipSetDevice(ctx->device));
    cache_gc(ctx);
    p.gate = std::shared_lock<std::shared_mutex>(ctx->gate);	// lookup .. enqueue
    int rc = get_twiddles(ctx, TwKey{(unsigned)cfg->fftsize, cfg->b_mark, cfg->b_space,
				     cfg->bit_nsamples}, &p.d_tw);
    if ( rc )
	return rc;
    derive_cfg(ctx, *cfg, p.d);
    return get_devcfg(ctx, p.d, &p.d_cfg, &p.tables);
}

int mifsk::lookup_tables( mifsk_ctx *ctx, const mifsk_rx_config *cfg, std::shared_lock<std::shared_mutex> &gate,
	DevCfg &d, const double **d_tw, const DevCfg **d_cfg )
{
    Prepared p;
    if ( int rc = prepare(ctx, cfg, p) )
	return rc;
    gate = std::move(p.gate);
    d = p.d;
    *d_tw = p.d_tw;
    if ( d_cfg )
	*d_cfg = p.d_cfg;
    return 0;
}

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
    if ( int rc = prepare(ctx, cfg, p) )
	return rc;
    return mifsk::launch_find_frame_batch(p.d, p.d_cfg, p.d_tw, d_samples, d_problems, d_results,
					  nproblems, stream);
}

// What a chained launch needs (mifsk_device.h WaveChain), with room for `ns` streams' states.
// Called with ctx->chain_lock held.
static int chain_prepare( mifsk_ctx *ctx, size_t ns )
{
    mifsk::WaveChain &ch = ctx->chain;
    if ( !ctx->chain_made ) {
	// (whatever an earlier, failed attempt made is kept and used: nothing is created twice)
	for ( void *&st : ch.streams )
	    if ( !st ) {
		hipStream_t h = nullptr;
		HIP_OK(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
		st = h;
	    }
	if ( !ch.ev_fork ) {
	    hipEvent_t e = nullptr;
	    HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
	    ch.ev_fork = e;
	}
	for ( void *&d : ch.ev_done )
	    if ( !d ) {
		hipEvent_t e = nullptr;
		HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		d = e;
	    }
	ctx->chain_made = true;
    }
    if ( ns > ch.state_cap ) {
	// (the chain before may still be running on the old array)
	for ( void *st : ch.streams )
	    HIP_OK(hipStreamSynchronize((hipStream_t)st));
	if ( ch.d_state )
	    (void)hipFree(ch.d_state);
	ch.d_state = nullptr;
	ch.state_cap = 0;
	const size_t cap = ( ns + 1023 ) & ~(size_t)1023;
	if ( hipMalloc((void **)&ch.d_state, cap * sizeof(mifsk_stream_state)) != hipSuccess )
	    return -ENOMEM;
	ch.state_cap = cap;
    }
    return 0;
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
	return launch(plan, p.d_cfg, p.d_tw, io, ha, stream);
    std::lock_guard<std::mutex> one(ctx->chain_lock);
    if ( int rc = chain_prepare(ctx, (size_t)io.nstreams) )
	return rc;
    ha.chain = &ctx->chain;
    return launch(plan, p.d_cfg, p.d_tw, io, ha, stream);
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
    if ( int rc = prepare(ctx, cfg, p) )
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
    if ( int rc = prepare(ctx, cfg, p) )
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
    if ( int rc = prepare(ctx, cfg, p) )
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
    derive_cfg(ctx, *cfg, d);
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

// ---------------------------------------------------------------------------
// the reference's five-function API (include/fsk.h) over the same kernels
// ---------------------------------------------------------------------------

namespace {

struct LegacyPlan {
    mifsk_ctx		*ctx;
    float		*d_samples;	size_t cap_samples;
    mifsk_search	*d_problem;
    mifsk_search_result	*d_result;
    float		*d_mags;	size_t cap_mags;
};

int legacy_reserve( LegacyPlan *lp, size_t nsamples )
{
    if ( nsamples <= lp->cap_samples )
	return 0;
    if ( lp->d_samples )
	(void)hipFree(lp->d_samples);
    lp->d_samples = nullptr;
    lp->cap_samples = 0;
    const size_t cap = ( nsamples + 4095 ) & ~(size_t)4095;
    if ( hipMalloc(&lp->d_samples, cap * sizeof(float)) != hipSuccess )
	return -ENOMEM;
    lp->cap_samples = cap;
    return 0;
}

} // namespace

extern "C" fsk_plan *fsk_plan_new( float sample_rate, float f_mark, float f_space,
	float filter_bw )
{
    fsk_plan *p = (fsk_plan *)std::calloc(1, sizeof(fsk_plan));
    if ( !p ) {
	errno = ENOMEM;
	return nullptr;
    }
    p->sample_rate = sample_rate;
    p->f_mark = f_mark;
    p->f_space = f_space;
    p->band_width = filter_bw;
    const float half = p->band_width / 2.0f;			// fsk.c:52-57
    p->fftsize = (int)( (sample_rate + half) / p->band_width );
    p->nbands = (unsigned)( p->fftsize / 2 + 1 );
    p->b_mark = (unsigned)( (f_mark + half) / p->band_width );
    p->b_space = (unsigned)( (f_space + half) / p->band_width );
    if ( p->b_mark >= p->nbands || p->b_space >= p->nbands ) {	// fsk.c:58-64
	fprintf(stderr, "b_mark=%u or b_space=%u is invalid (nbands=%u)\n",
		p->b_mark, p->b_space, p->nbands);
	std::free(p);
	errno = EINVAL;
	return nullptr;
    }
    LegacyPlan *lp = new (std::nothrow) LegacyPlan();
    if ( !lp ) {
	std::free(p);
	errno = ENOMEM;
	return nullptr;
    }
    std::memset(lp, 0, sizeof(*lp));
    int rc = mifsk_ctx_create(&lp->ctx, -1);
    if ( rc == 0 && ( hipMalloc(&lp->d_problem, sizeof(mifsk_search)) != hipSuccess
		   || hipMalloc(&lp->d_result, sizeof(mifsk_search_result)) != hipSuccess ) )
	rc = -ENOMEM;
    if ( rc ) {
	if ( lp->ctx ) mifsk_ctx_destroy(lp->ctx);
	delete lp;
	std::free(p);
	errno = -rc;
	return nullptr;
    }
    p->fftplan = lp;
    p->fftin = nullptr;
    p->fftout = nullptr;
    return p;
}

extern "C" void fsk_plan_destroy( fsk_plan *p )
{
    if ( !p )
	return;
    LegacyPlan *lp = (LegacyPlan *)p->fftplan;
    if ( lp ) {
	if ( lp->d_samples ) (void)hipFree(lp->d_samples);
	if ( lp->d_problem ) (void)hipFree(lp->d_problem);
	if ( lp->d_result ) (void)hipFree(lp->d_result);
	if ( lp->d_mags ) (void)hipFree(lp->d_mags);
	mifsk_ctx_destroy(lp->ctx);
	delete lp;
    }
    std::free(p);
}

extern "C" float fsk_find_frame( fsk_plan *p, float *samples, unsigned int frame_nsamples,
	unsigned int try_first_sample, unsigned int try_max_nsamples,
	unsigned int try_step_nsamples, float try_confidence_search_limit,
	const char *expect_bits_string, unsigned long long *bits_outp,
	float *ampl_outp, unsigned int *frame_start_outp )
{
    *bits_outp = 0;
    *ampl_outp = 0.0f;
    *frame_start_outp = 0;
    LegacyPlan *lp = p ? (LegacyPlan *)p->fftplan : nullptr;
    const size_t n_bits = expect_bits_string ? std::strlen(expect_bits_string) : 0;
    if ( !lp || n_bits == 0 || n_bits > MIFSK_MAX_FRAME_BITS	// assert in fsk.c:463
	    || (int)try_first_sample >= (int)try_max_nsamples || try_step_nsamples == 0 )
	return 0.0f;

    // the slice of the configuration that fsk_find_frame itself derives
    // (fsk.c:465,183,204); everything else in DevCfg is unused by this kernel
    mifsk_rx_config c;
    std::memset(&c, 0, sizeof(c));
    c.expect_n_bits = (unsigned)n_bits;
    const float spb = (float)frame_nsamples / (float)(int)n_bits;
    c.find_samples_per_bit = spb;
    c.bit_nsamples = (unsigned)( spb + 0.5f );
    if ( c.bit_nsamples == 0 )
	return 0.0f;
    for ( unsigned k = 0; k < n_bits; k++ ) {
	c.bit_offset[k] = (unsigned)( spb * (float)(int)k + 0.5f );
	c.expect_data[k] = expect_bits_string[k];
	c.expect_sync[k] = expect_bits_string[k];
    }
    c.fftsize = p->fftsize;
    c.b_mark = p->b_mark;
    c.b_space = p->b_space;

    // what the reference can touch (fsk.c:204-206,477-484): the highest candidate
    // it may try, first + k * step < try_max, plus the last bit window -- not
    // try_max - 1: a caller whose buffer ends at the reference's true extent
    // must not be over-read
    const unsigned up_steps = ( try_max_nsamples - try_first_sample - 1u ) / try_step_nsamples;
    const size_t t_last = (size_t)try_first_sample + (size_t)up_steps * try_step_nsamples;
    const size_t reach = t_last + c.bit_offset[n_bits - 1] + c.bit_nsamples;
    if ( hipSetDevice(lp->ctx->device) != hipSuccess || legacy_reserve(lp, reach) )
	return 0.0f;
    mifsk_search pr;
    pr.sample_offset = 0;
    pr.navail = (uint32_t)reach;
    pr.try_first = try_first_sample;
    pr.try_max = try_max_nsamples;
    pr.try_step = try_step_nsamples;
    pr.search_limit = try_confidence_search_limit;
    pr.use_sync_string = 0;
    mifsk_search_result res;
    if ( hipMemcpy(lp->d_samples, samples, reach * sizeof(float), hipMemcpyHostToDevice) != hipSuccess
	    || hipMemcpy(lp->d_problem, &pr, sizeof(pr), hipMemcpyHostToDevice) != hipSuccess )
	return 0.0f;
    if ( mifsk_find_frame_batch(lp->ctx, &c, lp->d_samples, lp->d_problem, lp->d_result, 1, nullptr) )
	return 0.0f;
    if ( hipMemcpy(&res, lp->d_result, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess )
	return 0.0f;
    *bits_outp = res.bits;
    *ampl_outp = res.amplitude;
    *frame_start_outp = res.frame_start;
    return res.confidence;
}

extern "C" int fsk_detect_carrier( fsk_plan *p, float *samples, unsigned int nsamples,
	float min_mag_threshold )
{
    LegacyPlan *lp = p ? (LegacyPlan *)p->fftplan : nullptr;
    if ( !lp || nsamples == 0 || nsamples > (unsigned)p->fftsize )	// assert in fsk.c:547
	return -1;
    mifsk_ctx *ctx = lp->ctx;
    if ( hipSetDevice(ctx->device) != hipSuccess )
	return -1;
    const unsigned N = (unsigned)p->fftsize;
    cache_gc(ctx);
    std::shared_lock<std::shared_mutex> gate(ctx->gate);	// lookup .. enqueue
    const double *d_cs = nullptr;
    if ( mifsk::get_cs(ctx, N, &d_cs) )
	return -1;
    if ( legacy_reserve(lp, nsamples) )
	return -1;
    if ( lp->cap_mags < p->nbands ) {
	if ( lp->d_mags ) (void)hipFree(lp->d_mags);
	lp->d_mags = nullptr;
	lp->cap_mags = 0;
	if ( hipMalloc(&lp->d_mags, p->nbands * sizeof(float)) != hipSuccess )
	    return -1;
	lp->cap_mags = p->nbands;
    }
    if ( hipMemcpy(lp->d_samples, samples, nsamples * sizeof(float), hipMemcpyHostToDevice) != hipSuccess )
	return -1;
    if ( mifsk::launch_detect_carrier(lp->d_samples, nsamples, d_cs, N, p->nbands,
				      lp->d_mags, nullptr) )
	return -1;
    std::vector<float> mags(p->nbands);
    if ( hipMemcpy(mags.data(), lp->d_mags, p->nbands * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess )
	return -1;
    // peak pick over the device-computed magnitudes (fsk.c:554-580)
    float max_mag = 0.0f;
    int max_band = -1;
    for ( unsigned i = 1; i < p->nbands; i++ ) {
	const float mag = mags[i];
	if ( mag < min_mag_threshold )
	    continue;
	if ( max_mag < mag ) {
	    max_mag = mag;
	    max_band = (int)i;
	}
    }
    return max_band;
}

extern "C" void fsk_set_tones_by_bandshift( fsk_plan *p, unsigned int b_mark, int b_shift )
{
    if ( !p || b_shift == 0 || b_mark >= p->nbands )		// asserts in fsk.c:587-592
	return;
    const int b_space = (int)b_mark + b_shift;
    if ( b_space < 0 || b_space >= (int)p->nbands )
	return;
    p->b_mark = b_mark;
    p->b_space = (unsigned)b_space;
    p->f_mark = b_mark * p->band_width;
    p->f_space = b_space * p->band_width;
}
