// mifsk_ctx.cpp -- the device context of libmifsk.so: create / destroy, its cache of device tables
// and the collector, what every launching entry point looks up (prepare), the chain's resources and
// the host pipeline's.  Everything the context keeps on the device is a member with an owner
// (mifsk_hostmem.h): there is no free in this file.
#include "mifsk_ctx.h"

#include <cerrno>
#include <cstring>
#include <new>

int mifsk::ctx_device( const mifsk_ctx *ctx ) { return ctx->device; }

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
    delete ctx;		// (the chain's streams are synchronised before its state array goes)
}

extern "C" const char *mifsk_ctx_device_name( const mifsk_ctx *ctx )
{
    return ctx ? ctx->name : "";
}

namespace mifsk {

// ---- the table cache ----

// n elements in device memory: -ENOMEM without the memory, -EIO without the copy, and then nothing is held
template <class T>
static int upload( const T *h, size_t n, DevMem<T> &d )
{
    if ( d.alloc(n) )
	return -ENOMEM;
    if ( hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess ) {
	d.reset();
	return -EIO;
    }
    return 0;
}

static int upload( const std::vector<double> &h, DevMem<double> &d ) { return upload(h.data(), h.size(), d); }

// Find or build, upload, keep: the entry of `entries` that `match` accepts, or a new one that
// `build` fills.  A build that fails leaves nothing: the half-made entry frees itself.
template <class Entry, class Match, class Build>
static int find_or_build( std::vector<Entry> &entries, Match match, Build build, const Entry **out )
{
    for ( const Entry &e : entries )
	if ( match(e) ) {
	    *out = &e;
	    return 0;
	}
    Entry e;
    if ( int rc = build(e) )
	return rc;
    entries.push_back(std::move(e));
    *out = &entries.back();
    return 0;
}

int TableCache::table( const TwKey &key, const double **d_out )
{
    const Table *t = nullptr;
    const int rc = find_or_build(tables,
	[&]( const Table &e ) { return e.key == key; },
	[&]( Table &e ) {
	    e.key = key;
	    return upload(key.bit_nsamples ? bit_table(key) : spectrum_table(key.fftsize), e.d);
	}, &t);
    if ( rc == 0 )
	*d_out = t->d.p;
    return rc;
}

int TableCache::config( const DevCfg &d, CfgTables &out )
{
    const Config *c = nullptr;
    const int rc = find_or_build(configs,
	[&]( const Config &e ) { return std::memcmp(&e.host, &d, sizeof(DevCfg)) == 0; },
	[&]( Config &e ) {
	    e.host = d;
	    if ( int rc = upload(&d, 1, e.dev) )
		return rc;
	    for ( int k = 0; k < 5; k++ ) {
		const std::vector<double> h = rotation_table(d, k, e.rot_stride[k]);
		if ( h.empty() )
		    continue;
		if ( int rc = upload(h, e.rot[k]) )
		    return rc;
	    }
	    return 0;
	}, &c);
    if ( rc )
	return rc;
    // (a view, not the entry: the vector may grow under another caller)
    out.d_cfg = c->dev.p;
    for ( int k = 0; k < 5; k++ ) {
	out.d_rot[k] = c->rot[k].p;
	out.rot_stride[k] = c->rot_stride[k];
    }
    return 0;
}

size_t TableCache::bytes() const
{
    size_t n = 0;
    for ( const Table &t : tables )
	n += t.d.cap;
    for ( const Config &c : configs )
	for ( const DevMem<double> &r : c.rot )
	    n += r.cap;
    return n * sizeof(double);
}

bool TableCache::full() const
{
    constexpr size_t kMaxConfigs = 64, kMaxTables = 64, kMaxTableBytes = 64u << 20;
    return configs.size() >= kMaxConfigs || tables.size() >= kMaxTables || bytes() >= kMaxTableBytes;
}

// The caches are bounded: the legacy API makes a DevCfg per window shape and a twiddle
// table per tone pair it is re-tuned to (fsk_set_tones_by_bandshift).  Called at the top
// of every entry point that launches, BEFORE it takes the gate: when a cache has outgrown
// its bound, wait until no call is between lookup and launch (exclusive gate), let the
// device finish what is running, and drop everything -- the next lookups rebuild what is
// still in use.
static void cache_gc( mifsk_ctx *ctx )
{
    {
	std::lock_guard<std::mutex> g(ctx->lock);
	if ( !ctx->cache.full() )
	    return;
    }
    std::unique_lock<std::shared_mutex> x(ctx->gate);
    std::lock_guard<std::mutex> g(ctx->lock);
    // (another caller may have flushed while this one waited for the gate)
    if ( !ctx->cache.full() )
	return;
    (void)hipDeviceSynchronize();
    ctx->cache.clear();
}

int get_cs( mifsk_ctx *ctx, unsigned N, const double **d_out )
{
    std::lock_guard<std::mutex> g(ctx->lock);
    return ctx->cache.table(TwKey{N, 0u, 0u, 0u}, d_out);
}

// (keyed by the configuration's bytes: two equal byte strings are equal configurations; unequal
// padding only costs a miss)
void derive_cfg( mifsk_ctx *ctx, const mifsk_rx_config &cfg, DevCfg &d )
{
    {
	std::lock_guard<std::mutex> g(ctx->lock);
	for ( const mifsk_ctx::DerivedCfg &e : ctx->derived )
	    if ( std::memcmp(&e.key, &cfg, sizeof(cfg)) == 0 ) {
		d = e.d;
		return;
	    }
    }
    fill_devcfg(d, cfg);
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

int enter( mifsk_ctx *ctx, std::shared_lock<std::shared_mutex> &gate )
{
    HIP_OK(hipSetDevice(ctx->device));
    cache_gc(ctx);
    gate = std::shared_lock<std::shared_mutex>(ctx->gate);	// lookup .. enqueue
    return 0;
}

int prepare( mifsk_ctx *ctx, const mifsk_rx_config *cfg, Prepared &p )
{
    if ( int rc = enter(ctx, p.gate) )
	return rc;
    {
	std::lock_guard<std::mutex> g(ctx->lock);
	if ( int rc = ctx->cache.table(TwKey{(unsigned)cfg->fftsize, cfg->b_mark, cfg->b_space, cfg->bit_nsamples},
				       &p.d_tw) )
	    return rc;
    }
    derive_cfg(ctx, *cfg, p.d);
    std::lock_guard<std::mutex> g(ctx->lock);
    return ctx->cache.config(p.d, p.tables);
}

int lookup_tables( mifsk_ctx *ctx, const mifsk_rx_config *cfg, std::shared_lock<std::shared_mutex> &gate,
	DevCfg &d, const double **d_tw, const DevCfg **d_cfg )
{
    Prepared p;
    if ( int rc = prepare(ctx, cfg, p) )
	return rc;
    gate = std::move(p.gate);
    d = p.d;
    *d_tw = p.d_tw;
    if ( d_cfg )
	*d_cfg = p.tables.d_cfg;
    return 0;
}

// ---- streams and events: the chain's, the host pipeline's ----

int chain_prepare( mifsk_ctx *ctx, size_t ns )
{
    ChainRes &ch = ctx->chain;
    if ( !ch.made ) {
	// (whatever an earlier, failed attempt made is kept and used: nothing is created twice)
	int rc = ch.ev_fork.make();
	for ( int g = 0; g < WaveChain::kMaxGroups && rc == 0; g++ )
	    if ( ( rc = ch.streams[g].make() ) == 0 )
		rc = ch.ev_done[g].make();
	if ( rc )
	    return rc;
	for ( int g = 0; g < WaveChain::kMaxGroups; g++ ) {
	    ch.view.streams[g] = ch.streams[g].h;
	    ch.view.ev_done[g] = ch.ev_done[g].h;
	}
	ch.view.ev_fork = ch.ev_fork.h;
	ch.made = true;
    }
    if ( ns > ch.state.cap ) {
	// (the chain before may still be running on the old array)
	for ( const HipStream &st : ch.streams )
	    HIP_OK(hipStreamSynchronize(st));
	const int rc = ch.state.alloc(( ns + 1023 ) & ~(size_t)1023);
	ch.view.d_state = ch.state.p;
	ch.view.state_cap = ch.state.cap;
	if ( rc )
	    return rc;
    }
    return 0;
}

// `overlapped`: the job has more than one chunk, i.e. something to overlap: the copy streams and
// the events that order the three are made then.  A job of one chunk -- a file, a few files: the
// reference's own use -- runs on the null stream alone (a stream costs ~10 ms to make: a third of
// what such a call spent inside the library).  Only what is missing is made: a
// call after one that failed half-way goes on where that one stopped.
int host_work_init( HostWork *w, bool overlapped )
{
    if ( w->ready || !overlapped )
	return 0;
    int rc = w->s_comp.make();
    if ( rc == 0 ) rc = w->s_in.make();
    if ( rc == 0 ) rc = w->s_out.make();
    for ( int i = 0; i < 2 && rc == 0; i++ )
	if ( ( rc = w->ev_in[i].make() ) == 0 && ( rc = w->ev_comp[i].make() ) == 0 )
	    rc = w->ev_out[i].make();
    w->ready = rc == 0;
    return rc;
}

} // namespace mifsk
