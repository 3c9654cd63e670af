// mifsk_timesplit_plan.cpp -- the host logic of the time split (DESIGN.md "cutting a stream in
// time"): the parameter check, the planner, the row table of a planned call, the host half of a
// verify / re-run round and the tail placement.  Plain C++: nothing here touches the device, so
// tools/timesplit_rounds.cpp runs all of it on a CPU; mifsk_timesplit.hip is the driver.
#include <algorithm>
#include <cerrno>
#include <cstring>

#include "mifsk_timesplit.h"

namespace {

const unsigned kKnownFlags = MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE
			   | MIFSK_TIME_SPLIT_REJECT_ALL;

} // namespace

int mifsk::time_split_check_params( const mifsk_rx_config *cfg, const mifsk_time_split *params )
{
    if ( mifsk_check_cfg(cfg) )
	return -EINVAL;
    mifsk_time_split p;
    std::memset(&p, 0, sizeof(p));
    if ( params )
	p = *params;
    if ( p.flags & ~kKnownFlags )
	return -EINVAL;
    if ( ( p.flags & MIFSK_IO_ENGINE_WORKGROUP ) && ( p.flags & MIFSK_IO_ENGINE_WAVE ) )
	return -EINVAL;
    if ( p.flags & MIFSK_IO_RING_EXACT )
	return -ENOTSUP;
    if ( cfg->samplebuf_size < 2u )
	return -EINVAL;
    const uint64_t half = cfg->samplebuf_size / 2u;
    const uint64_t lattice = half / timesplit::gcd64(half, 4) * 4;		// lcm(samplebuf_size / 2, 4)
    if ( p.warmup && p.warmup < 2ull * cfg->samplebuf_size )
	return -EINVAL;
    if ( p.chunk && ( p.chunk % lattice || p.chunk >= 0x7FFFFFF0ull ) )
	return -EINVAL;
    if ( p.warmup >= 0x7FFFFFF0ull )
	return -EINVAL;		// (rows are uint32 lengths; keeps the planner's arithmetic exact)
    return 0;
}

namespace mifsk {
namespace timesplit {

uint64_t gcd64( uint64_t a, uint64_t b )
{
    while ( b ) {
	const uint64_t t = a % b;
	a = b;
	b = t;
    }
    return a;
}

int plan( const mifsk_rx_config *cfg, const uint64_t *n, int nstreams, const mifsk_time_split *params,
	uint32_t chunks_hint, mifsk_time_split_stats *out )
{
    if ( !cfg || !out || !n || nstreams <= 0 )
	return -EINVAL;
    if ( const int rc = time_split_check_params(cfg, params) )
	return rc;
    mifsk_time_split p;
    std::memset(&p, 0, sizeof(p));
    if ( params )
	p = *params;
    const uint64_t half = cfg->samplebuf_size / 2u;
    const uint64_t lattice = half / gcd64(half, 4) * 4;		// lcm(samplebuf_size / 2, 4)
    const uint64_t wmin = 2ull * cfg->samplebuf_size;
    uint64_t W = p.warmup;
    if ( !W ) {
	W = (uint64_t)( kDefaultWarmupSeconds * cfg->sample_rate );
	W = std::max(W, wmin);
    }
    // what the chunks have to cover, and the longest stream
    uint64_t cover = 0, longest = 0;
    for ( int m = 0; m < nstreams; m++ ) {
	if ( n[m] >= ( 1ull << 62 ) )
	    return -EINVAL;
	longest = std::max(longest, n[m]);
	if ( n[m] > W )
	    cover += n[m] - W;
	if ( cover >= ( 1ull << 62 ) )
	    return -EINVAL;
    }
    uint64_t L = p.chunk;
    uint64_t rows = (uint64_t)nstreams;
    bool split = false;
    if ( cover ) {
	if ( !L ) {
	    // (sum of K_m - 1 <= cover / L <= target: the cap bounds the rows' warm-up overlap)
	    uint64_t target = p.chunks ? p.chunks : ( chunks_hint ? chunks_hint : 1024u );
	    target = std::min(target, std::max<uint64_t>(2, kOverlapBudget / ( W * sizeof(float) )));
	    L = ( cover + target - 1 ) / target;
	    L = std::max(lattice, ( L + lattice - 1 ) / lattice * lattice);
	}
	rows = 0;
	for ( int m = 0; m < nstreams; m++ )
	    rows += n[m] > W ? ( n[m] - W ) / L + 1 : 1;
	split = rows > (uint64_t)nstreams;
	// the library's choice: a split pays when a row (about L + 2 W) is well short of the whole
	if ( !p.chunk && !p.warmup && 4 * W > longest )
	    split = false;
    }
    if ( split && ( L + W >= 0x7FFFFFF0ull || rows > 0x7FFFFFFull ) )
	return -EINVAL;
    if ( !split && longest > 0xFFFFFFF0ull )
	return -EINVAL;
    for ( int m = 0; m < nstreams; m++ ) {
	const uint64_t K = split && n[m] > W ? ( n[m] - W ) / L + 1 : 1;
	mifsk_time_split_stats &o = out[m];
	std::memset(&o, 0, sizeof(o));
	o.nsamples = n[m];
	o.warmup = W;
	o.lattice = lattice;
	o.nchunks = (uint32_t)K;
	o.chunk = split ? L : n[m];		// (one chunk everywhere: the single call, no cut)
	o.samples_speculative = 2 * ( K - 1 ) * W;
    }
    return 0;
}

RowLayout::RowLayout( const mifsk_rx_config *cfg, const uint64_t *nsamples,
	const std::vector<mifsk_time_split_stats> &ps )
    : M((int)ps.size()), R(0), L(ps[0].chunk), W(ps[0].warmup), rstride(( L + W + 3u ) & ~3ull),
      fcap(mifsk_max_frames(cfg, L + W)), ecap(mifsk_max_episodes(cfg, L + W) + 1), hs(ps.size())
{
    for ( int m = 0; m < M; m++ )
	R += (int)ps[m].nchunks;
    nrows = R + M;
    hrow.resize(nrows);
    hns.assign(nrows, 0);
    for ( int m = 0, r = 0; m < M; m++ ) {
	hs[m].n = nsamples[m];
	hs[m].tail_off = 0;
	hs[m].rowbase = (uint32_t)r;
	hs[m].K = ps[m].nchunks;
	for ( uint32_t k = 0; k < hs[m].K; k++, r++ ) {
	    hrow[r].m = (uint32_t)m;
	    hrow[r].k = k;
	    hns[r] = (uint32_t)( k + 1 < hs[m].K ? L + W : nsamples[m] - k * L );
	}
	hrow[R + m].m = (uint32_t)m;
	hrow[R + m].k = hs[m].K;
    }
}

RowFlags::RowFlags( const RowLayout &lay )
    : settled(lay.nrows, 0), drop(lay.nrows, 0), ran(lay.nrows, 0), mark(lay.nrows, 0)
{
    for ( const StreamRef &s : lay.hs )
	settled[s.rowbase] = 1;
}

RowSpan settle_round( const std::vector<uint32_t> &hcode, const RowLayout &lay, RowFlags &f,
	std::vector<mifsk_time_split_stats> &ps )
{
    RowSpan span = { -1, -1 };
    std::fill(f.mark.begin(), f.mark.end(), 0);
    for ( size_t m = 0; m < lay.hs.size(); m++ ) {
	const int r0 = (int)lay.hs[m].rowbase, r1 = r0 + (int)lay.hs[m].K;
	for ( int r = r0 + 1; r < r1; r++ ) {
	    if ( f.settled[r] )
		continue;
	    if ( !f.settled[r - 1] )
		break;
	    if ( f.drop[r - 1] || ( hcode[r] & 2u ) ) {
		f.drop[r] = f.settled[r] = 1;
	    } else if ( hcode[r] & 1u ) {
		f.settled[r] = 1;
		ps[m].accepted += !f.ran[r];
	    } else {
		break;
	    }
	}
	bool any = false;
	for ( int r = r0 + 1; r < r1; r++ )
	    if ( !f.settled[r] && hcode[r] == 0u ) {	// (behind a finished row: wait for it to settle)
		f.mark[r] = 1;
		any = true;
		if ( span.lo < 0 )
		    span.lo = r;
		span.hi = r;
		f.ran[r] = 1;
		ps[m].rerun++;
		ps[m].samples_rerun += lay.hns[r];
	    }
	ps[m].rounds += any;
    }
    return span;
}

Tails place_tails( RowLayout &lay, std::vector<mifsk_stream_state> &last, std::vector<uint8_t> &drop )
{
    Tails t = { 0, false };
    for ( int m = 0; m < lay.M; m++ ) {
	StreamRef &s = lay.hs[m];
	if ( drop[s.rowbase + s.K - 1] || ( last[m].flags & MIFSK_STATE_FINISHED ) ) {
	    drop[lay.R + m] = 1;
	    s.tail_off = s.n;
	    std::memset(&last[m], 0, sizeof(last[m]));
	    last[m].flags = MIFSK_STATE_STARTED | MIFSK_STATE_FINISHED;
	    continue;
	}
	const uint64_t rel = last[m].base & ~3ull;	// (rows start 16-byte aligned)
	s.tail_off = ( s.K - 1 ) * lay.L + rel;
	last[m] = reset_book(last[m], rel);
	lay.hns[lay.R + m] = (uint32_t)( s.n - s.tail_off );
	t.longest = std::max<uint64_t>(t.longest, lay.hns[lay.R + m]);
	t.live = true;
    }
    return t;
}

} // namespace timesplit
} // namespace mifsk

extern "C" int mifsk_time_split_plan_get( const mifsk_rx_config *cfg, uint64_t nsamples,
	const mifsk_time_split *params, mifsk_time_split_stats *out )
{
    return mifsk::timesplit::plan(cfg, &nsamples, 1, params, 0, out);
}

extern "C" int mifsk_time_split_plan_batch_get( const mifsk_rx_config *cfg, const uint64_t *nsamples,
	int nstreams, const mifsk_time_split *params, mifsk_time_split_stats *out )
{
    return mifsk::timesplit::plan(cfg, nsamples, nstreams, params, 0, out);
}
