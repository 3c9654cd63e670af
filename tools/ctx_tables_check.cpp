// ctx_tables_check.cpp -- the context's device tables, its collector and its streams and events
// without a device: minimodem_amd/csrc/mifsk_ctx.cpp and mifsk_tables.cpp over a HIP made of malloc()
// (tools/fake_hip.h), whose N-th allocation, copy, stream or event can be made to fail, and every
// double of every table against the oracle's ofsk_twiddle (oracle/fsk_oracle.c, compiled in as the
// oracle's own library compiles it: its cos and -sin are ONE sincos call).
//
//   gcc -O2 -std=gnu11 -mfma -ffp-contract=off -c oracle/fsk_oracle.c -o fsk_oracle.o
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc -Itools
//       -fsanitize=address,undefined -o ctx_tables_check tools/ctx_tables_check.cpp
//       minimodem_amd/csrc/mifsk_ctx.cpp minimodem_amd/csrc/mifsk_tables.cpp
//       minimodem_amd/csrc/mifsk_plan.cpp minimodem_amd/csrc/mifsk_config.cpp fsk_oracle.o -lm
//
// Exit status 0 and "ctx_tables_check: N checks, 0 failed" when all is well; a leak, a double free
// or a read of freed memory is the sanitizer's to report.  (tests/test_ctx_tables.py)
#include <cerrno>
#include <string>
#include <utility>
#include <vector>

#include "fake_hip.h"
#include "mifsk_ctx.h"

extern "C" void ofsk_twiddle( unsigned int b, unsigned int n, unsigned int fftsize, double w[2] );

using namespace mifsk;

// ---- configurations

static mifsk_rx_config config_of( const std::string &mode )
{
    mifsk_modem_args a;
    mifsk_modem_args_default(&a);
    a.baudmode = mode.c_str();
    mifsk_rx_config cfg;
    CHECK(mifsk_rx_config_init(&cfg, &a) == 0);
    return cfg;
}

// B samples per bit at 48 kHz
static mifsk_rx_config config_of_bit_length( unsigned B )
{
    char mode[64];
    std::snprintf(mode, sizeof(mode), "%.17g", 48000.0 / (double)B);
    const mifsk_rx_config cfg = config_of(mode);
    CHECK(cfg.bit_nsamples == B);
    return cfg;
}

static TwKey key_of( const mifsk_rx_config &cfg )
{
    return TwKey{(unsigned)cfg.fftsize, cfg.b_mark, cfg.b_space, cfg.bit_nsamples};
}

static bool same_bits( const double *a, const double *b, size_t n )
{
    return std::memcmp(a, b, n * sizeof(double)) == 0;
}

// ---- table contents, bit for bit: the oracle's entries where the layout puts them, +0.0 elsewhere

static void check_bit_table( const mifsk_rx_config &cfg )
{
    const TwKey key = key_of(cfg);
    const std::vector<double> h = bit_table(key);
    const size_t entries = tw_entries(key.bit_nsamples) > 8 ? tw_entries(key.bit_nsamples) : 8;
    std::vector<double> want(4 * entries, 0.0);
    for ( unsigned n = 0; n < key.bit_nsamples; n++ ) {
	ofsk_twiddle(key.b_mark, n, key.fftsize, &want[4 * (size_t)n]);
	ofsk_twiddle(key.b_space, n, key.fftsize, &want[4 * (size_t)n + 2]);
    }
    CHECK(key.bit_nsamples <= entries && h.size() == want.size() && same_bits(h.data(), want.data(), want.size()));
}

static void check_spectrum_table( unsigned N )
{
    const std::vector<double> h = spectrum_table(N);
    std::vector<double> want(2 * (size_t)N);
    for ( unsigned k = 0; k < N; k++ )
	ofsk_twiddle(1u, k, N, &want[2 * (size_t)k]);		// (1 * k mod N = k: the oracle's 2 pi k / N)
    CHECK(h.size() == want.size() && same_bits(h.data(), want.data(), want.size()));
}

// -> how many of the configuration's five scans have a plan
static int check_rotation_tables( const mifsk_rx_config &cfg )
{
    DevCfg d;
    fill_devcfg(d, cfg);
    int valid = 0;
    for ( int kind = 0; kind < 5; kind++ ) {
	uint32_t stride = 12345;
	const std::vector<double> h = rotation_table(d, kind, stride);
	const SegPlan &sp = d.seg[kind];
	if ( !sp.valid ) {
	    CHECK(h.empty() && stride == 0);
	    continue;
	}
	valid++;
	unsigned cmax = 0;
	for ( unsigned w = 0; w < sp.nwin; w++ )
	    cmax = sp.win_count[w] > cmax ? sp.win_count[w] : cmax;
	const size_t rows = ( cmax + 12u + 3u ) & ~3u;
	CHECK(stride == ( ( sp.nwin + 63u ) & ~63u ) && stride >= sp.nwin && cmax > 0);
	std::vector<double> want(rows * stride * 4, 0.0);
	for ( unsigned w = 0; w < sp.nwin; w++ )
	    for ( unsigned i = 0; i < sp.win_count[w]; i++ ) {
		const unsigned off = sp.seg_rel[sp.win_first[w] + i] - ( sp.p_win[w] >> 16 );
		ofsk_twiddle(d.b_mark, off, d.fftsize, &want[( (size_t)i * stride + w ) * 4]);
		ofsk_twiddle(d.b_space, off, d.fftsize, &want[( (size_t)i * stride + w ) * 4 + 2]);
	    }
	CHECK(h.size() == want.size() && same_bits(h.data(), want.data(), want.size()));
    }
    return valid;
}

// ---- the cache

static mifsk_ctx *new_ctx()
{
    mifsk_ctx *ctx = nullptr;
    CHECK(mifsk_ctx_create(&ctx, 0) == 0 && ctx != nullptr);
    return ctx;
}

// allocations the cache's entries account for; a configuration entry is whole or not there
static long held( const mifsk_ctx *ctx )
{
    long n = (long)ctx->cache.tables.size();
    for ( const TableCache::Table &t : ctx->cache.tables )
	CHECK(t.d.p != nullptr);
    for ( const TableCache::Config &c : ctx->cache.configs ) {
	CHECK(c.dev.p != nullptr);
	n++;
	for ( int k = 0; k < 5; k++ ) {
	    CHECK(( c.rot[k].p != nullptr ) == ( c.host.seg[k].valid != 0 ) && ( c.rot_stride[k] != 0 ) == ( c.rot[k].p != nullptr ));
	    n += c.rot[k].p != nullptr;
	}
    }
    return n;
}

// the code of a call under the countdown that is set: the failure's, or 0
static int expected_rc()
{
    return g_alloc.fail_at ? -ENOMEM : g_copy.fail_at ? -EIO : 0;
}

static void all_succeed()
{
    g_alloc.fail_at = g_copy.fail_at = g_make.fail_at = 0;
}

// what a lookup hands back is what the builders make, in the fake's "device" memory
static void check_prepared( const mifsk_rx_config &cfg, const Prepared &p )
{
    const std::vector<double> tw = bit_table(key_of(cfg));
    CHECK(p.d_tw && same_bits(p.d_tw, tw.data(), tw.size()));
    CHECK(p.tables.d_cfg && std::memcmp(p.tables.d_cfg, &p.d, sizeof(DevCfg)) == 0);
    for ( int k = 0; k < 5; k++ ) {
	uint32_t stride = 0;
	const std::vector<double> rot = rotation_table(p.d, k, stride);
	CHECK(p.tables.rot_stride[k] == stride && ( p.tables.d_rot[k] != nullptr ) == !rot.empty());
	if ( p.tables.d_rot[k] && !rot.empty() )
	    CHECK(same_bits(p.tables.d_rot[k], rot.data(), rot.size()));
    }
}

// the first lookup of a configuration, something failing on the way (or not); the same lookup again;
// and once more: the same pointers, nothing allocated
static void lookup_scenario( const mifsk_rx_config &cfg )
{
    mifsk_ctx *ctx = new_ctx();
    {
	Prepared p;
	const int rc = prepare(ctx, &cfg, p);
	CHECK(rc == expected_rc());
	CHECK(g_live == held(ctx));			// nothing of a half-made entry stays behind
	if ( rc )
	    CHECK(ctx->cache.configs.empty());
    }
    all_succeed();
    Prepared first;
    CHECK(prepare(ctx, &cfg, first) == 0);
    check_prepared(cfg, first);
    first.gate = {};					// (the next call may want the gate exclusively)
    const long allocs = g_alloc.n, copies = g_copy.n;
    Prepared second;
    CHECK(prepare(ctx, &cfg, second) == 0 && g_alloc.n == allocs && g_copy.n == copies);
    CHECK(second.d_tw == first.d_tw && second.tables.d_cfg == first.tables.d_cfg);
    for ( int k = 0; k < 5; k++ )
	CHECK(second.tables.d_rot[k] == first.tables.d_rot[k] && second.tables.rot_stride[k] == first.tables.rot_stride[k]);
    CHECK(g_live == held(ctx) && ctx->cache.configs.size() == 1 && ctx->cache.tables.size() == 1);
    second.gate = {};
    mifsk_ctx_destroy(ctx);
}

static int spectrum( mifsk_ctx *ctx, unsigned N, const double **d_cs )
{
    std::shared_lock<std::shared_mutex> gate;
    CHECK(enter(ctx, gate) == 0);
    return get_cs(ctx, N, d_cs);
}

static void spectrum_scenario( unsigned N )
{
    mifsk_ctx *ctx = new_ctx();
    const double *d_cs = nullptr, *again = nullptr;
    const int rc = spectrum(ctx, N, &d_cs);
    CHECK(rc == expected_rc());
    if ( rc )
	CHECK(g_live == 0 && ctx->cache.tables.empty() && ctx->cache.bytes() == 0);
    all_succeed();
    CHECK(spectrum(ctx, N, &d_cs) == 0);
    const std::vector<double> cs = spectrum_table(N);
    CHECK(d_cs && same_bits(d_cs, cs.data(), cs.size()) && ctx->cache.bytes() == cs.size() * sizeof(double));
    const long allocs = g_alloc.n;
    CHECK(spectrum(ctx, N, &again) == 0 && again == d_cs && g_alloc.n == allocs && g_live == 1);
    mifsk_ctx_destroy(ctx);
}

// `n` configurations (bit lengths from `B0`) looked up once each
static void fill_configs( mifsk_ctx *ctx, unsigned B0, unsigned n )
{
    for ( unsigned B = B0; B < B0 + n; B++ ) {
	const mifsk_rx_config cfg = config_of_bit_length(B);
	Prepared p;
	CHECK(prepare(ctx, &cfg, p) == 0);
    }
}

// the collector runs when a call enters: one device synchronisation, nothing left
static void check_flush( mifsk_ctx *ctx, bool expected )
{
    const long syncs = g_device_syncs, live = g_live;
    std::shared_lock<std::shared_mutex> gate;
    CHECK(enter(ctx, gate) == 0);
    if ( expected )
	CHECK(g_device_syncs == syncs + 1 && g_live == 0 && ctx->cache.bytes() == 0
	      && ctx->cache.configs.empty() && ctx->cache.tables.empty());
    else
	CHECK(g_device_syncs == syncs && g_live == live && g_live == held(ctx));
}

static void collector_scenario()
{
    // 64 configurations
    mifsk_ctx *ctx = new_ctx();
    const mifsk_rx_config used = config_of_bit_length(8);
    std::vector<double> before;
    fill_configs(ctx, 8, 63);
    check_flush(ctx, false);
    CHECK(ctx->cache.configs.size() == 63 && g_device_syncs == 0);
    {
	Prepared p;
	CHECK(prepare(ctx, &used, p) == 0 && ctx->cache.configs.size() == 63);	// (one of the 63)
	before.assign(p.d_tw, p.d_tw + bit_table(key_of(used)).size());
    }
    fill_configs(ctx, 8 + 63, 1);
    CHECK(ctx->cache.configs.size() == 64 && ctx->cache.tables.size() == 64 && g_device_syncs == 0);
    {
	// the 64th makes the next prepare flush; a configuration used before is rebuilt with the same contents
	Prepared p;
	CHECK(prepare(ctx, &used, p) == 0 && g_device_syncs == 1);
	CHECK(ctx->cache.configs.size() == 1 && ctx->cache.tables.size() == 1 && g_live == held(ctx) && g_live == 2);
	CHECK(same_bits(p.d_tw, before.data(), before.size()));
	check_prepared(used, p);
    }
    check_flush(ctx, false);
    fill_configs(ctx, 100, 63);
    check_flush(ctx, true);
    mifsk_ctx_destroy(ctx);

    // 64 tables: one bit table and 63 spectrum tables
    ctx = new_ctx();
    fill_configs(ctx, 8, 1);
    const double *d_cs = nullptr;
    for ( unsigned N = 16; N < 16 + 62; N++ )
	CHECK(spectrum(ctx, N, &d_cs) == 0);
    check_flush(ctx, false);
    CHECK(ctx->cache.tables.size() == 63);
    CHECK(spectrum(ctx, 240, &d_cs) == 0);
    before.assign(d_cs, d_cs + 2 * 240);
    check_flush(ctx, true);
    CHECK(spectrum(ctx, 240, &d_cs) == 0 && same_bits(d_cs, before.data(), before.size()) && g_live == 1);
    mifsk_ctx_destroy(ctx);

    // 64 MB: two spectrum tables of 32 MB
    ctx = new_ctx();
    CHECK(spectrum(ctx, 1u << 21, &d_cs) == 0 && ctx->cache.bytes() == (size_t)32 << 20);
    check_flush(ctx, false);
    CHECK(spectrum(ctx, ( 1u << 21 ) - 1u, &d_cs) == 0);
    check_flush(ctx, false);				// (16 bytes short of the bound)
    CHECK(spectrum(ctx, 1u, &d_cs) == 0 && ctx->cache.bytes() == (size_t)64 << 20);
    check_flush(ctx, true);
    mifsk_ctx_destroy(ctx);
}

// ---- streams and events

template <class Owner>
static void handle_scenario()
{
    const long drops = g_drops;
    {
	Owner a;
	CHECK(a.h == nullptr);
	int rc = a.make();
	CHECK(rc == ( g_make.fail_at == 1 ? -EIO : 0 ) && ( a.h != nullptr ) == ( rc == 0 ));
	const auto was = a.h;
	const long makes = g_make.n;
	rc = a.make();					// holds one: nothing is made
	if ( was )
	    CHECK(rc == 0 && a.h == was && g_make.n == makes);
	const auto now = a.h;				// (made by the second call where the first failed)
	Owner b(std::move(a));
	CHECK(a.h == nullptr && b.h == now);
	Owner c;
	(void)c.make();
	c = std::move(b);				// over something held: that goes first
	CHECK(b.h == nullptr);
	Owner &self = c;
	c = std::move(self);
	c.reset();
	c.reset();
	CHECK(c.h == nullptr);
    }
    CHECK(g_handles == 0 && g_drops - drops == g_make.n - ( g_make.fail_at && g_make.fail_at <= g_make.n ? 1 : 0 ));
}

// host_work_init with a creation failing, then again: ready, three streams and six events, none made twice
static void host_work_scenario()
{
    HostWork *w = new HostWork();
    CHECK(host_work_init(w, false) == 0 && !w->ready && g_make.n == 0);	// one chunk: nothing to overlap
    int rc = host_work_init(w, true);
    CHECK(rc == ( g_make.fail_at ? -EIO : 0 ) && w->ready == ( rc == 0 ));
    const bool failed = rc != 0;
    all_succeed();
    CHECK(host_work_init(w, true) == 0 && w->ready);
    CHECK(g_handles == 9 && g_make.n == 9 + ( failed ? 1 : 0 ));
    CHECK(w->s_in.h && w->s_comp.h && w->s_out.h);
    for ( int i = 0; i < 2; i++ )
	CHECK(w->ev_in[i].h && w->ev_comp[i].h && w->ev_out[i].h);
    const long makes = g_make.n;
    CHECK(host_work_init(w, true) == 0 && g_make.n == makes);
    delete w;
}

// the chain: a creation or the state array's allocation failing, then again; a larger batch
static void chain_scenario()
{
    mifsk_ctx *ctx = new_ctx();
    {
	std::lock_guard<std::mutex> one(ctx->chain_lock);
	const long makes = g_make.n;
	const int rc = chain_prepare(ctx, 1000);
	CHECK(rc == ( g_make.fail_at ? -EIO : g_alloc.fail_at == 1 ? -ENOMEM : 0 ));
	const bool make_failed = g_make.fail_at != 0;
	const WaveChain &v = ctx->chain.view;
	if ( rc )
	    CHECK(v.d_state == nullptr && v.state_cap == 0 && g_live == 0);
	all_succeed();
	CHECK(chain_prepare(ctx, 1000) == 0 && ctx->chain.made);
	CHECK(g_handles == 7 && g_make.n - makes == 7 + ( make_failed ? 1 : 0 ));	// what the failed attempt made was kept
	CHECK(v.d_state == ctx->chain.state.p && v.d_state && v.state_cap == 1024 && v.ev_fork == ctx->chain.ev_fork.h);
	for ( int g = 0; g < WaveChain::kMaxGroups; g++ )
	    CHECK(v.streams[g] == ctx->chain.streams[g].h && v.streams[g] && v.ev_done[g] == ctx->chain.ev_done[g].h && v.ev_done[g]);
	const mifsk_stream_state *was = v.d_state;
	const long syncs = g_syncs;
	CHECK(chain_prepare(ctx, 1024) == 0 && v.d_state == was && g_syncs == syncs);
	CHECK(chain_prepare(ctx, 1025) == 0 && v.state_cap == 2048 && g_syncs == syncs + 3 && g_live == 1 && g_handles == 7);
	std::memset(v.d_state, 0, v.state_cap * sizeof(mifsk_stream_state));	// (the whole of it is there)
    }
    mifsk_ctx_destroy(ctx);
}

int main()
{
    const mifsk_rx_config bell202 = config_of("1200"), rtty = config_of("rtty"), same = config_of("same");
    CHECK(bell202.bit_nsamples == 40 && bell202.fftsize == 240);

    // the tables as values
    for ( const mifsk_rx_config &cfg : { bell202, config_of_bit_length(3), config_of_bit_length(320), same, rtty } ) {
	check_bit_table(cfg);
	const int valid = check_rotation_tables(cfg);
	CHECK(cfg.bit_nsamples >= 256 ? valid >= 2 : valid == 0);	// RTTY, B = 320: several scans with a plan
    }
    check_spectrum_table(240);
    check_spectrum_table((unsigned)rtty.fftsize);

    // the cache, every allocation and every copy failing in turn
    for ( Countdown *c : { &g_alloc, &g_copy } ) {
	every_failure(*c, [&] { lookup_scenario(bell202); });
	every_failure(*c, [&] { lookup_scenario(rtty); });
	every_failure(*c, [&] { spectrum_scenario(240); });
    }
    run(g_alloc, 0, collector_scenario);

    // streams and events
    every_failure(g_make, handle_scenario<HipStream>);
    every_failure(g_make, handle_scenario<HipEvent>);
    every_failure(g_make, host_work_scenario);
    every_failure(g_make, chain_scenario);
    every_failure(g_alloc, chain_scenario);

    // a context with a full cache, a made chain and the host pipeline's work goes whole, once, and
    // the chain's state array after its streams are synchronised
    run(g_alloc, 0, [] {
	mifsk_ctx *ctx = new_ctx();
	fill_configs(ctx, 8, 64);
	{
	    std::lock_guard<std::mutex> one(ctx->chain_lock);
	    CHECK(chain_prepare(ctx, 5000) == 0);
	}
	ctx->host.reset(new HostWork());
	CHECK(host_work_init(ctx->host.get(), true) == 0 && ctx->host->pin[0].fit(100) == 0);
	CHECK(g_live == held(ctx) + 2 && g_handles == 16);
	const long drops = g_drops, syncs = g_syncs;
	g_watch = ctx->chain.state.p;
	mifsk_ctx_destroy(ctx);
	CHECK(g_drops == drops + 16 && g_watch_syncs == syncs + 3);
	g_watch = nullptr;
    });

    CHECK(g_live == 0 && g_handles == 0);
    std::printf("ctx_tables_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
