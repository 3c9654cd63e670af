// timesplit_rounds.cpp -- the host logic of the time split without a device: the planner, the row
// table, settle_round and place_tails of minimodem_amd/csrc/mifsk_timesplit_plan.cpp, with a
// deterministic model in the place of the kernels (DESIGN.md "cutting a stream in time").
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc
//       -fsanitize=address,undefined -o timesplit_rounds tools/timesplit_rounds.cpp
//       minimodem_amd/csrc/mifsk_timesplit_plan.cpp minimodem_amd/csrc/mifsk_config.cpp && ./timesplit_rounds
//
// Prints "timesplit_rounds: N cases, F failed" (each failed check with a line of its own before
// it); exit status 1 when F > 0.  (tests/test_time_split_rounds.py)
#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mifsk_timesplit.h"

using namespace mifsk::timesplit;

static long g_cases = 0, g_failed = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;

#define CHECK(cond, ...) do { if ( !( cond ) ) { if ( g_failed++ < 50 ) { std::printf("FAILED %s: ", #cond); \
	std::printf(__VA_ARGS__); std::printf("\n"); } return; } } while (0)

static uint64_t rnd()		// splitmix64
{
    uint64_t z = ( g_rng += 0x9E3779B97F4A7C15ull );
    z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
    z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull;
    return z ^ ( z >> 31 );
}
static bool chance( double p ) { return (double)( rnd() >> 11 ) * ( 1.0 / 9007199254740992.0 ) < p; }

static mifsk_rx_config config( const char *mode )
{
    mifsk_modem_args a;
    mifsk_modem_args_default(&a);
    a.baudmode = mode;
    mifsk_rx_config c;
    if ( mifsk_rx_config_init(&c, &a) )
	std::abort();
    return c;
}

// ---- rounds: states are labels.  Row r's correct entry state is label r + 1; run from it the row
// pauses in the next row's (kFin: the row finishes its stream); run from any other state it pauses
// there too with probability p, else in a label nothing else has.
static const int64_t kFin = -1;
struct Model {
    double			p;
    int				fin;		// the row that finishes its stream, or -1
    int64_t			fresh = 1 << 20;
    std::vector<int64_t>	start, pause;
    int64_t run( int r, int64_t from )
    {
	const int64_t right = r == fin ? kFin : r + 2;
	return from == r + 1 || chance(p) ? right : fresh++;
    }
};

static void rounds_case( const mifsk_rx_config &cfg, double q, double p )
{
    g_cases++;
    const uint64_t lat = cfg.samplebuf_size / 2u / gcd64(cfg.samplebuf_size / 2u, 4) * 4, W = 2ull * cfg.samplebuf_size;
    const int M = 1 + (int)( rnd() % 5 );
    std::vector<uint64_t> n(M);
    std::vector<mifsk_time_split_stats> ps(M);
    for ( int m = 0; m < M; m++ ) {
	std::memset(&ps[m], 0, sizeof(ps[m]));
	ps[m].nchunks = 1 + (uint32_t)( rnd() % 12 );
	ps[m].chunk = lat;
	ps[m].warmup = W;
	ps[m].nsamples = n[m] = ( ps[m].nchunks - 1 ) * lat + W + rnd() % lat;
    }
    RowLayout lay(&cfg, n.data(), ps);
    RowFlags f(lay);
    const int R = lay.R;
    Model d;
    d.p = p;
    d.fin = rnd() % 2 ? (int)( rnd() % R ) : -1;
    d.start.resize(R);
    d.pause.resize(R);
    for ( int r = 0; r < R; r++ ) {		// pass A's guesses (a stream's row 0 needs none), pass B
	d.start[r] = lay.hrow[r].k == 0 || chance(q) ? r + 1 : d.fresh++;
	d.pause[r] = d.run(r, d.start[r]);
    }
    std::vector<uint32_t> code(lay.nrows, 0);
    std::vector<int> reruns(R, 0);
    uint64_t passes = 0;
    for ( ;; passes++ ) {
	CHECK(passes <= 12, "the rounds do not end (q %g p %g)", q, p);
	for ( int r = 0; r < R; r++ )		// ts_verify
	    if ( lay.hrow[r].k )
		code[r] = d.pause[r - 1] == kFin ? 2u : d.start[r] == d.pause[r - 1] ? 1u : 0u;
	const RowSpan span = settle_round(code, lay, f, ps);
	for ( int r = 0; r < lay.nrows; r++ )		// (a row behind a finished one waits: it is not marked)
	    CHECK(!f.mark[r] || ( r >= span.lo && r <= span.hi && r < R && code[r] == 0 ), "row %d marked outside [%d, %d]",
		  r, span.lo, span.hi);
	if ( span.lo < 0 )
	    break;
	CHECK(f.mark[span.lo] && f.mark[span.hi], "[%d, %d] does not end on marked rows", span.lo, span.hi);
	std::vector<int64_t> seed(d.pause);		// ts_seed reads every pause before a row runs again
	for ( int r = span.lo; r <= span.hi; r++ )
	    if ( f.mark[r] ) {
		d.start[r] = seed[r - 1];
		d.pause[r] = d.run(r, d.start[r]);
		reruns[r]++;
	    }
    }
    uint32_t most = 0;
    for ( int m = 0; m < M; m++ ) {
	const StreamRef &s = lay.hs[m];
	uint32_t ever = 0, dropped_unrun = 0, total = 0;
	uint64_t samples = 0;
	bool finished = false;		// a row before this one finished the stream
	for ( uint32_t k = 0; k < s.K; k++ ) {
	    const int r = (int)( s.rowbase + k );
	    CHECK(f.settled[r], "row %d is not settled", r);
	    CHECK(!!f.drop[r] == finished, "row %d of stream %d: drop %d, finished before it %d", r, m, f.drop[r], finished);
	    CHECK(f.drop[r] || d.start[r] == r + 1, "kept row %d started from the wrong state", r);
	    CHECK(!!f.ran[r] == ( reruns[r] > 0 ), "row %d: ran %d after %d re-runs", r, f.ran[r], reruns[r]);
	    ever += reruns[r] > 0;
	    dropped_unrun += f.drop[r] && !reruns[r];
	    total += (uint32_t)reruns[r];
	    samples += (uint64_t)reruns[r] * lay.hns[r];
	    finished = finished || r == d.fin;
	}
	CHECK(ps[m].rounds <= s.K - 1, "stream %d: %u rounds for %u chunks", m, ps[m].rounds, s.K);
	CHECK(ps[m].accepted + ever + dropped_unrun == s.K - 1, "stream %d: accepted %u + re-run %u + dropped %u != %u",
	      m, ps[m].accepted, ever, dropped_unrun, s.K - 1);
	CHECK(ps[m].rerun == total && ps[m].samples_rerun == samples, "stream %d: rerun %u (%u), samples_rerun %" PRIu64
	      " (%" PRIu64 ")", m, ps[m].rerun, total, ps[m].samples_rerun, samples);
	most = std::max(most, ps[m].rounds);
    }
    CHECK(passes == most, "%" PRIu64 " passes, the largest per-stream rounds %u", passes, most);
}

// ---- the row table of a plan, and the tails over made-up last states
static void layout_case( const mifsk_rx_config &cfg, const std::vector<uint64_t> &n, const mifsk_time_split *params )
{
    g_cases++;
    const int M = (int)n.size();
    std::vector<mifsk_time_split_stats> ps(M);
    const int rc = plan(&cfg, n.data(), M, params, 0, ps.data());
    CHECK(rc == 0, "plan: %d", rc);
    uint64_t sumK = 0;
    for ( int m = 0; m < M; m++ )
	sumK += ps[m].nchunks;
    if ( sumK == (uint64_t)M )
	return;			// (no stream is cut: no row table)
    RowLayout lay(&cfg, n.data(), ps);
    const uint64_t L = ps[0].chunk, W = ps[0].warmup;
    CHECK(lay.M == M && lay.R == (int)sumK && lay.nrows == lay.R + M && lay.L == L && lay.W == W
	  && lay.rstride == ( ( L + W + 3 ) & ~3ull ), "the layout's sizes");
    for ( int m = 0, r = 0; m < M; m++ ) {
	const StreamRef &s = lay.hs[m];
	CHECK(s.n == n[m] && (int)s.rowbase == r && s.K == ps[m].nchunks, "stream %d's rows", m);
	for ( uint32_t k = 0; k < s.K; k++, r++ )
	    CHECK(lay.hrow[r].m == (uint32_t)m && lay.hrow[r].k == k
		  && lay.hns[r] == ( k + 1 < s.K ? L + W : n[m] - k * L ) && lay.hns[r] <= L + W, "row %d", r);
	CHECK(lay.hrow[lay.R + m].m == (uint32_t)m && lay.hrow[lay.R + m].k == s.K && lay.hns[lay.R + m] == 0, "tail %d", m);
    }
    std::vector<mifsk_stream_state> last(M), was;
    std::vector<uint8_t> drop(lay.nrows, 0);
    for ( int m = 0; m < M; m++ ) {
	const int end = (int)( lay.hs[m].rowbase + lay.hs[m].K - 1 );
	std::memset(&last[m], 0, sizeof(last[m]));
	last[m].base = rnd() % ( (uint64_t)lay.hns[end] + 1 );
	last[m].rp = last[m].base + rnd() % 1000;
	last[m].flags = MIFSK_STATE_STARTED | ( rnd() % 2 ? MIFSK_STATE_CARRIER : 0 ) | ( rnd() % 4 ? 0 : MIFSK_STATE_FINISHED );
	last[m].nframes_total = last[m].nbytes_total = (uint32_t)rnd();
	last[m].carrier_nsamples = rnd();
	last[m].b_mark = 7;
	drop[end] = rnd() % 4 == 0;
    }
    was = last;
    const std::vector<uint8_t> dropped(drop);
    const Tails t = place_tails(lay, last, drop);
    uint64_t longest = 0;
    bool live = false;
    for ( int m = 0; m < M; m++ ) {
	const StreamRef &s = lay.hs[m];
	const uint32_t len = lay.hns[lay.R + m];
	mifsk_stream_state want;
	if ( dropped[s.rowbase + s.K - 1] || ( was[m].flags & MIFSK_STATE_FINISHED ) ) {
	    std::memset(&want, 0, sizeof(want));
	    want.flags = MIFSK_STATE_STARTED | MIFSK_STATE_FINISHED;
	    CHECK(s.tail_off == n[m] && len == 0 && drop[lay.R + m] == 1, "stream %d's dropped tail", m);
	} else {
	    const uint64_t rel = was[m].base & ~3ull;
	    want = reset_book(was[m], rel);
	    CHECK(s.tail_off == ( s.K - 1 ) * L + rel && len == n[m] - s.tail_off && drop[lay.R + m] == 0, "stream %d's tail", m);
	    live = true;
	}
	CHECK(std::memcmp(&last[m], &want, sizeof(want)) == 0, "the state stream %d's tail starts from", m);
	longest = std::max<uint64_t>(longest, len);
    }
    CHECK(t.longest == longest && t.live == live, "longest tail %" PRIu64 " (%" PRIu64 "), live %d (%d)", t.longest, longest,
	  t.live, live);
    CHECK(std::equal(dropped.begin(), dropped.begin() + lay.R, drop.begin()), "a chunk row's drop flag changed");
}

// ---- the planner at the edges of its arithmetic: 0 or the documented refusals, and a cut that covers
static void edge_case( const mifsk_rx_config &cfg, uint64_t n, uint64_t warmup, uint32_t chunks, uint64_t chunk )
{
    g_cases++;
    const mifsk_time_split p = { chunk, warmup, chunks, 0 };
    const uint64_t two[2] = { n, n / 3 };
    mifsk_time_split_stats ps[2];
    for ( int M = 1; M <= 2; M++ ) {
	const int rc = plan(&cfg, two, M, &p, 0, ps);
	CHECK(rc == 0 || rc == -EINVAL || rc == -ENOTSUP, "plan(%" PRIu64 "): %d", n, rc);
	for ( int m = 0; rc == 0 && m < M; m++ ) {
	    const uint64_t K = ps[m].nchunks, L = ps[m].chunk, W = ps[m].warmup;
	    CHECK(K >= 1 && ps[m].nsamples == two[m], "K %" PRIu64, K);
	    if ( ps[0].nchunks + ( M > 1 ? ps[1].nchunks : 1 ) > 2 )		// a split
		CHECK(L % ps[m].lattice == 0 && L + W < 0x7FFFFFF0ull
		      && ( two[m] > W ? ( K - 1 ) * L + W <= two[m] && two[m] < K * L + W : K == 1 ),
		      "n %" PRIu64 " K %" PRIu64 " L %" PRIu64 " W %" PRIu64, two[m], K, L, W);
	}
    }
}

int main()
{
    static const char *const kModes[] = { "1200", "300", "rtty", "tdd", "same", "12000", "uic-train", "callerid" };
    static const double kProb[] = { 0.0, 0.25, 0.5, 0.75, 1.0 };
    const mifsk_rx_config bell = config("1200");
    for ( double q : kProb )		// (q = 0: MIFSK_TIME_SPLIT_REJECT_ALL; p = 0: the longest chains)
	for ( double p : kProb )
	    for ( int i = 0; i < 1000; i++ )
		rounds_case(bell, q, p);
    for ( const char *mode : kModes ) {
	const mifsk_rx_config cfg = config(mode);
	const uint64_t half = cfg.samplebuf_size / 2u, lat = half / gcd64(half, 4) * 4, wmin = 2ull * cfg.samplebuf_size;
	const uint64_t W = std::max<uint64_t>((uint64_t)( kDefaultWarmupSeconds * cfg.sample_rate ), wmin);
	const mifsk_time_split least = { lat, wmin, 0, 0 };
	const uint64_t hours2 = 7200ull * cfg.sample_rate;
	const uint64_t lens[] = { 0, 1, wmin - 1, wmin, wmin + 1, wmin + lat, W, W + 1, 4 * W, hours2 / 24, hours2 };
	for ( int i = 0; i < 40; i++ ) {
	    std::vector<uint64_t> n(1 + rnd() % 4);
	    for ( uint64_t &v : n )
		v = rnd() % 3 ? lens[rnd() % ( sizeof(lens) / sizeof(lens[0]) )] : rnd() % ( hours2 + 1 );
	    layout_case(cfg, n, nullptr);
	    for ( uint64_t &v : n )		// (a lattice step per chunk: keep the forced plan's table small)
		v %= hours2 / 24 + 1;
	    layout_case(cfg, n, &least);
	}
	const uint64_t around[] = { W, 4 * W, 1ull << 31, 1ull << 32, 1ull << 62, UINT64_MAX };
	const uint64_t warm[] = { 0, wmin - 1, wmin, 0x7FFFFFEFull, 0x7FFFFFF0ull, UINT64_MAX };
	const uint32_t chunks[] = { 0, 1, 0xFFFFFFFFu };
	const uint64_t chunk_of[] = { 0, lat, lat * ( 0x7FFFFFEFull / lat ) };
	const uint64_t deltas[] = { UINT64_MAX, 0, 1 };		// (-1, 0, +1)
	for ( uint64_t a : around )
	    for ( uint64_t delta : deltas )
		for ( uint64_t w : warm )
		    for ( uint32_t c : chunks )
			for ( uint64_t chunk : chunk_of )
			    edge_case(cfg, a + delta, w, c, chunk);
    }
    std::printf("timesplit_rounds: %ld cases, %ld failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
