// mifsk_plan.cpp -- the host-side planner: what the kernels read of a receive configuration (DevCfg,
// mifsk_device.h; cached by the context) and the launch plan of a batch (LaunchPlan: engine, kernel,
// LDS geometry, chain cut).  Plain C++: nothing here touches the device; every experiment knob is read here.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mifsk.h"
#include "mifsk_device.h"

namespace mifsk {

// The closed form of one zig-zag scan (fsk.c:477-484: first, first + step, first - step, ...
// until a candidate reaches `mx`, candidates below 0 skipped): `up` candidates at or above
// `first`, `down` below it.  The scan ends with the first candidate at or beyond mx, so it
// never goes further down than it went up.
struct ZigZagCounts { unsigned up, down; };
static ZigZagCounts zigzag_counts( unsigned first, unsigned mx, unsigned step )
{
    if ( (int)first >= (int)mx || step == 0 )
	return ZigZagCounts{0u, 0u};
    const unsigned up = ( mx - first - 1 ) / step + 1;
    return ZigZagCounts{up, up - 1 < first / step ? up - 1 : first / step};
}

// candidates of one zig-zag scan in scan order, appended to `out`
static void zigzag_candidates( std::vector<unsigned> &out, unsigned first, unsigned mx, unsigned step )
{
    const ZigZagCounts z = zigzag_counts(first, mx, step);
    const unsigned U = z.up, D = z.down;
    for ( unsigned i = 0; i < U + D; i++ ) {
	if ( i == 0 ) out.push_back(first);
	else if ( i <= 2 * D ) out.push_back(( i & 1u ) ? first + ( ( i + 1 ) / 2 ) * step : first - ( ( i + 1 ) / 2 ) * step);
	else out.push_back(first + ( i - D ) * step);
    }
}

// The shared-segment plan of one zig-zag scan (SegPlan in mifsk_device.h): cut the span
// the scan's windows cover at every window edge, drop pieces no window covers (bit
// offsets are rounded, consecutive windows may leave a sample between them), split the
// longest pieces until the lanes of ceil(n / 64) passes are full, hand the pieces to
// the passes longest first.
// `cand`: the candidates whose windows the plan covers, window w = candidate w / n_bits, bit w % n_bits
static void plan_segments( SegPlan &sp, const mifsk_rx_config &c, const std::vector<unsigned> &cand )
{
    std::memset(&sp, 0, sizeof(sp));
    const unsigned nb = c.expect_n_bits, B = c.bit_nsamples;
    const unsigned J = (unsigned)cand.size();
    if ( J == 0 || nb == 0 || J * nb > (unsigned)SEGW_MAX )
	return;
    auto at = [&]( unsigned i ) -> unsigned { return cand[i]; };
    std::vector<unsigned> wstart(J * nb);
    std::vector<unsigned> cuts;
    for ( unsigned j = 0; j < J; j++ )
	for ( unsigned k = 0; k < nb; k++ ) {
	    const unsigned a = at(j) + c.bit_offset[k];
	    wstart[j * nb + k] = a;
	    cuts.push_back(a);
	    cuts.push_back(a + B);
	}
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    struct Seg { unsigned rel, len; };
    std::vector<Seg> segs;
    for ( size_t i = 0; i + 1 < cuts.size(); i++ ) {
	const unsigned lo = cuts[i], hi = cuts[i + 1];
	bool covered = false;
	for ( unsigned a : wstart )
	    covered = covered || ( a <= lo && hi <= a + B );
	if ( covered )
	    segs.push_back(Seg{lo, hi - lo});
    }
    if ( segs.empty() || segs.size() > (size_t)SEG_MAX )
	return;
    // Balance.  Every piece may be cut further; the parts go to (at most two) passes of 64 lanes,
    // longest first.  What a pass costs is decided by its longest part: whole groups of 16 samples
    // (a group of the sums: ~86 instructions, ~118 where some lane's part ends inside it and the
    // samples are masked) in whole tile steps of 32 (stage, read back, fetch: ~60).  Two ways of
    // cutting are tried and the cheapest plan is taken:
    //  * equal parts: with a target length T piece i gets ceil(len_i / T) parts (all T);
    //  * caps (round 6): pass 0 takes parts of at most A0 samples, pass 1 of at most A1 <= A0, and
    //    a piece is cut UNEQUALLY into n0 parts for the one and n1 for the other -- which (n0, n1)
    //    per piece is a small dynamic program over the 64 lanes of each pass.  RTTY's carrier-held
    //    plan (pieces of 165, 110, 66, 55, 44 samples) went from 83 + 82 | 110 whole -- 7 + 6 groups
    //    in 4 + 3 steps -- to 101 + 64 | 110 whole: 7 + 4 groups in 4 + 2 steps.
    {
	const std::vector<Seg> pieces = segs;
	// (the assembly: ~16 instructions per segment of the longest window, once per 64 windows --
	// per 32 where two lanes share a window, Wave::seg_correlate)
	const unsigned asm_units = J * nb <= 32u ? 1u : 2u * ( ( J * nb + 63u ) / 64u );
	auto cost_of = [&]( const std::vector<std::vector<unsigned>> &parts ) -> unsigned {
	    std::vector<unsigned> lens, at;
	    for ( size_t i = 0; i < parts.size(); i++ ) {
		unsigned a = pieces[i].rel;
		for ( unsigned l : parts[i] ) {
		    lens.push_back(l);
		    at.push_back(a);
		    a += l;
		}
	    }
	    if ( lens.empty() || lens.size() > (size_t)SEG_MAX )
		return 0xFFFFFFFFu;
	    unsigned cmax = 0;
	    for ( unsigned a : wstart ) {
		unsigned n = 0;
		for ( size_t i = 0; i < lens.size(); i++ )
		    n += ( at[i] >= a && at[i] + lens[i] <= a + B ) ? 1u : 0u;
		cmax = std::max(cmax, n);
	    }
	    std::sort(lens.begin(), lens.end(), [](unsigned x, unsigned y) { return x > y; });
	    unsigned cost = 8u * cmax * asm_units;
	    for ( size_t p0 = 0; p0 < lens.size(); p0 += 64 ) {
		const size_t p1 = std::min(lens.size(), p0 + 64);
		const unsigned lmax = lens[p0], lmin = lens[p1 - 1];
		const unsigned g = ( lmax + 15 ) / 16, st = ( g + 1 ) / 2, full = lmin / 16;
		cost += 86u * g + 60u * st + 32u * ( g - std::min(g, full) );
	    }
	    return cost;
	};
	unsigned best_cost = 0xFFFFFFFFu;
	std::vector<std::vector<unsigned>> best;		// the parts of every piece, in position order
	// equal parts
	{
	    std::vector<unsigned> cand;
	    for ( const Seg &s : pieces )
		for ( unsigned k = 1; k <= 16u && s.len / k >= 16u; k++ )
		    cand.push_back(( s.len + k - 1 ) / k);
	    std::sort(cand.begin(), cand.end());
	    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
	    for ( unsigned T : cand ) {
		std::vector<std::vector<unsigned>> parts;
		size_t nparts = 0;
		for ( const Seg &s : pieces ) {
		    const unsigned k = ( s.len + T - 1 ) / T;
		    parts.emplace_back();
		    for ( unsigned q = 0; q < k; q++ )
			parts.back().push_back(s.len / k + ( q < s.len % k ? 1u : 0u ));
		    nparts += k;
		}
		if ( nparts > (size_t)SEG_MAX )
		    continue;
		const unsigned c = cost_of(parts);
		if ( c < best_cost ) {
		    best_cost = c;
		    best = parts;
		}
	    }
	}
	// caps
	{
	    unsigned lnat = 0, ltot = 0;
	    for ( const Seg &s : pieces ) {
		lnat = std::max(lnat, s.len);
		ltot += s.len;
	    }
	    const unsigned amax = ( lnat + 15u ) & ~15u;
	    constexpr unsigned INF = 0xFFFFu;
	    std::vector<uint16_t> choice(pieces.size() * 65u);
	    std::vector<unsigned> dp(65), nx(65);
	    std::vector<std::vector<unsigned>> parts(pieces.size());
	    // (caps in whole groups; for very long windows in coarser steps: at most 32 values)
	    const unsigned astep = std::max(16u, ( amax / 32u + 15u ) & ~15u);
	    for ( unsigned A0 = astep; A0 <= amax + astep - 1u; A0 += astep )
		for ( unsigned A1 = astep; A1 <= A0; A1 += astep ) {
		    if ( 64u * ( A0 + A1 ) < ltot )
			continue;			// (the lanes of two passes cannot hold the span)
		    // (a plan whose longest parts are a whole group below its caps is found under the
		    // smaller caps: these caps cost at least their own groups and steps)
		    if ( 86u * ( A0 / 16u + A1 / 16u ) + 60u * ( ( A0 + 16u ) / 32u + ( A1 + 16u ) / 32u ) >= best_cost )
			continue;
		    // dp[j]: fewest pass-1 parts with j pass-0 parts over the pieces so far
		    std::fill(dp.begin(), dp.end(), INF);
		    dp[0] = 0;
		    for ( size_t i = 0; i < pieces.size(); i++ ) {
			const unsigned L = pieces[i].len;
			std::fill(nx.begin(), nx.end(), INF);
			for ( unsigned j = 0; j <= 64; j++ ) {
			    if ( dp[j] == INF )
				continue;
			    for ( unsigned n0 = 0; n0 <= ( L + A0 - 1 ) / A0 && j + n0 <= 64; n0++ ) {
				const unsigned rest = L > n0 * A0 ? L - n0 * A0 : 0u;
				const unsigned n1 = ( rest + A1 - 1 ) / A1;
				if ( n0 + n1 == 0 || n0 + n1 > L )
				    continue;
				if ( dp[j] + n1 < nx[j + n0] ) {
				    nx[j + n0] = dp[j] + n1;
				    choice[i * 65u + j + n0] = (uint16_t)n0;
				}
			    }
			}
			dp.swap(nx);
		    }
		    unsigned jbest = 65;
		    for ( unsigned j = 0; j <= 64; j++ )
			if ( dp[j] <= 64 && ( jbest == 65 || dp[j] + j < dp[jbest] + jbest ) )
			    jbest = j;
		    if ( jbest == 65 )
			continue;
		    // walk back: n0 of every piece; its n1 follows
		    unsigned j = jbest;
		    for ( size_t i = pieces.size(); i-- > 0; ) {
			const unsigned L = pieces[i].len, n0 = choice[i * 65u + j];
			const unsigned rest = L > n0 * A0 ? L - n0 * A0 : 0u;
			const unsigned n1 = ( rest + A1 - 1 ) / A1;
			// pass 1's parts as long as they may be, pass 0's share the rest equally
			unsigned t1 = n1 ? std::min(n1 * A1, L - n0) : 0u;
			if ( n0 == 0 )
			    t1 = L;
			const unsigned t0 = L - t1;
			parts[i].clear();
			for ( unsigned q = 0; q < n0; q++ )
			    parts[i].push_back(t0 / n0 + ( q < t0 % n0 ? 1u : 0u ));
			for ( unsigned q = 0; q < n1; q++ )
			    parts[i].push_back(t1 / n1 + ( q < t1 % n1 ? 1u : 0u ));
			j -= n0;
		    }
		    bool sound = true;
		    for ( const std::vector<unsigned> &pp : parts )
			for ( unsigned l : pp )
			    sound = sound && l >= 1u;
		    const unsigned c = sound ? cost_of(parts) : 0xFFFFFFFFu;
		    if ( c < best_cost ) {
			best_cost = c;
			best = parts;
		    }
		}
	}
	if ( best.empty() )
	    return;
	segs.clear();
	for ( size_t i = 0; i < pieces.size(); i++ ) {
	    unsigned at = pieces[i].rel, total = 0;
	    for ( unsigned l : best[i] ) {
		segs.push_back(Seg{at, l});
		at += l;
		total += l;
	    }
	    if ( total != pieces[i].len )
		return;				// (cannot happen; leaves valid = 0)
	}
	if ( segs.size() > (size_t)SEG_MAX )
	    return;
    }
    const unsigned npass = (unsigned)( ( segs.size() + 63 ) / 64 );
    // passes: longest pieces first, position order inside a pass
    std::vector<unsigned> order(segs.size());
    for ( size_t i = 0; i < order.size(); i++ ) order[i] = (unsigned)i;
    std::stable_sort(order.begin(), order.end(), [&]( unsigned a, unsigned b ) { return segs[a].len > segs[b].len; });
    sp.nseg = (unsigned)segs.size();
    sp.npass = npass;
    sp.nwin = J * nb;
    for ( unsigned i = 0; i < (unsigned)SEG_MAX; i++ )
	sp.slot_seg[i] = 0xFFFFu;
    unsigned lmax = 0;
    for ( unsigned pss = 0; pss < npass; pss++ ) {
	std::vector<unsigned> mine(order.begin() + 64 * pss,
				   order.begin() + (long)std::min<size_t>(order.size(), 64 * ( pss + 1 )));
	std::sort(mine.begin(), mine.end());
	sp.pass_len[pss] = 0;
	sp.pass_min[pss] = 0xFFFFFFFFu;
	for ( size_t l = 0; l < mine.size(); l++ ) {
	    sp.slot_seg[64 * pss + l] = (uint16_t)mine[l];
	    sp.pass_len[pss] = std::max(sp.pass_len[pss], segs[mine[l]].len);
	    sp.pass_min[pss] = std::min(sp.pass_min[pss], segs[mine[l]].len);
	}
	lmax = std::max(lmax, sp.pass_len[pss]);
    }
    for ( size_t i = 0; i < segs.size(); i++ ) {
	sp.seg_rel[i] = segs[i].rel;
	sp.seg_len[i] = (uint16_t)segs[i].len;
	sp.span_hi = std::max(sp.span_hi, segs[i].rel + segs[i].len);
    }
    unsigned cmax = 0;
    for ( unsigned w = 0; w < sp.nwin; w++ ) {
	unsigned f = 0, n = 0;
	bool in = false;
	for ( unsigned i = 0; i < sp.nseg; i++ ) {
	    const bool inside = segs[i].rel >= wstart[w] && segs[i].rel + segs[i].len <= wstart[w] + B;
	    if ( inside && !in ) { f = i; in = true; }
	    if ( inside ) n++;
	}
	sp.win_first[w] = (uint16_t)f;
	sp.win_count[w] = (uint16_t)n;
	cmax = std::max(cmax, n);
	// (its pieces are consecutive and tile it but for the uncovered samples, which no
	// window contains: those lie between windows, never inside one)
	unsigned total = 0;
	for ( unsigned i = f; i < f + n; i++ ) total += segs[i].len;
	if ( total != B )
	    return;				// (cannot happen; leaves valid = 0)
    }
    // DESIGN.md "shared segments": index-order rounding (B - 1) + segment sums
    // sqrt(2) (L - 1) + assembly 2 n + table entries' own rounding 85, in units of
    // 2^-53 * sum |x|; rounded up generously
    // (+ 2: a short scan's windows are assembled as two half sums and one more addition)
    sp.bound_c = (float)( B + 1.5 * lmax + 2.0 * cmax + 2.0 + 128.0 );
    // (a pass loads table group ceil(L / 16) + 3 at most; the table has ceil(B / 16) + 1)
    if ( ( lmax + 15 ) / 16 + 3 > ( B + 15 ) / 16 )
	return;
    // packed copies; a plan whose numbers do not fit the fields is not used
    if ( lmax >= 4096u || sp.span_hi >= ( 1u << 20 ) || sp.nseg > 255u )
	return;
    for ( unsigned i = 0; i < (unsigned)SEG_MAX; i++ ) {
	const unsigned s = sp.slot_seg[i];
	sp.p_slot_seg[i] = s == 0xFFFFu ? 0xFFu : (uint8_t)s;
	sp.p_slot[i] = s == 0xFFFFu ? 0u : ( sp.seg_rel[s] | ( (uint32_t)sp.seg_len[s] << 20 ) );
    }
    for ( unsigned w = 0; w < sp.nwin; w++ ) {
	if ( wstart[w] >= 65536u || sp.win_count[w] > 255u )
	    return;
	sp.p_win[w] = sp.win_first[w] | ( (uint32_t)sp.win_count[w] << 8 ) | ( wstart[w] << 16 );
    }
    sp.valid = 1;
}

// the last sample a frame's bit windows touch, relative to the frame's start
static uint32_t last_reach( const mifsk_rx_config &c )
{
    return c.bit_offset[c.expect_n_bits - 1] + c.bit_nsamples;
}

size_t ring_row_floats( const mifsk_rx_config &c )
{
    // samplebuf plus what a search at the top of it may touch beyond
    const size_t reach = (size_t)( c.try_max[0] > c.try_max[1] ? c.try_max[0] : c.try_max[1] )
		       + last_reach(c) + 64;
    return ( (size_t)c.samplebuf_size + reach + 3 ) & ~(size_t)3;
}

void fill_devcfg( DevCfg &d, const mifsk_rx_config &c )
{
    std::memset(&d, 0, sizeof(d));
    d.n_bits = c.expect_n_bits;
    d.bit_nsamples = c.bit_nsamples;
    d.last_reach = last_reach(c);
    d.magscalar = 2.0f / (float)c.bit_nsamples;		// fsk.c:132
    d.frame_nsamples = c.frame_nsamples;
    d.expect_nsamples = c.expect_nsamples;
    d.overscan = c.nsamples_overscan;
    for ( int i = 0; i < 2; i++ ) {
	d.try_first[i] = c.try_first[i];
	d.try_max[i] = c.try_max[i];
	d.try_step[i] = c.try_step[i];
	d.try_step_fine[i] = c.try_step_fine[i];
    }
    d.conf_threshold = c.confidence_threshold;
    d.search_limit = c.search_limit;
    d.n_data_bits = c.n_data_bits;
    d.nstartbits = (uint32_t)c.nstartbits;
    d.has_stopbits = c.nstopbits != 0.0f ? 1u : 0u;
    d.msb_first = c.msb_first ? 1u : 0u;
    d.do_rx_sync = c.do_rx_sync ? 1u : 0u;
    d.rx_one = c.rx_one ? 1u : 0u;
    d.sync_byte = c.sync_byte;
    d.b_mark = c.b_mark;
    d.b_space = c.b_space;
    d.fftsize = (uint32_t)c.fftsize;

    // One pad word per bit row of a SCAN slab where that spreads the lanes of a
    // search over more LDS banks: the first 64 windows of the carrier-held fine
    // search (lane = candidate * n_bits + bit, ds_read_b32, 32 lanes per LDS
    // cycle, bank = word mod 32) are laid out both ways and the cheaper pitch
    // wins; unpadded rows on a tie (no per-sample row test in the correlator).
    {
	std::vector<unsigned> fine;
	zigzag_candidates(fine, c.try_first[1], c.try_max[1], c.try_step_fine[1]);
	auto cost = [&]( unsigned skew ) -> unsigned {
	    const unsigned nb = c.expect_n_bits ? c.expect_n_bits : 1u, B = c.bit_nsamples ? c.bit_nsamples : 1u;
	    unsigned word[64], n = 0;
	    for ( size_t i = 0; i < fine.size() && n < 64; i++ ) {
		for ( unsigned k = 0; k < nb && n < 64; k++ ) {
		    const unsigned rel = fine[i] + c.bit_offset[k];
		    word[n++] = rel + ( rel / B ) * skew;
		}
	    }
	    unsigned total = 0;
	    for ( unsigned h = 0; h < n; h += 32 ) {
		unsigned worst = 0;
		for ( unsigned bank = 0; bank < 32; bank++ ) {
		    unsigned distinct = 0;
		    for ( unsigned i = h; i < n && i < h + 32; i++ ) {
			if ( word[i] % 32 != bank )
			    continue;
			bool seen = false;
			for ( unsigned j = h; j < i; j++ )
			    seen = seen || word[j] == word[i];
			distinct += seen ? 0u : 1u;
		    }
		    worst = distinct > worst ? distinct : worst;
		}
		total += worst;
	    }
	    return total;
	};
	d.skew = cost(1) < cost(0) ? 1u : 0u;
    }
    for ( int i = 0; i < 4; i++ ) {
	const ZigZagCounts z = zigzag_counts(c.try_first[i & 1], c.try_max[i & 1],
					     ( i & 2 ) ? c.try_step_fine[i & 1] : c.try_step[i & 1]);
	d.zz_up[i] = z.up;
	d.zz_down[i] = z.down;
    }
    // long windows (what the wavefront engine reads through its LDS tile): the scans share
    // their segments' partial sums
    if ( c.bit_nsamples >= 256u && c.bit_nsamples <= 65535u )
	for ( int i = 0; i < 4; i++ ) {
	    std::vector<unsigned> cand;
	    zigzag_candidates(cand, c.try_first[i & 1], c.try_max[i & 1],
			      ( i & 2 ) ? c.try_step_fine[i & 1] : c.try_step[i & 1]);
	    plan_segments(d.seg[i], c, cand);
	}
    if ( d.seg[1].valid && d.seg[3].valid ) {
	std::vector<unsigned> cand;
	zigzag_candidates(cand, c.try_first[1], c.try_max[1], c.try_step[1]);
	d.seg_union_first_fine = (uint32_t)cand.size() * c.expect_n_bits;
	zigzag_candidates(cand, c.try_first[1], c.try_max[1], c.try_step_fine[1]);
	plan_segments(d.seg[4], c, cand);
    }
    d.div_magic = c.bit_nsamples > 1 ? (uint32_t)( 0x100000000ULL / c.bit_nsamples ) : 0xFFFFFFFFu;
    // minimodem.c:1407 with frame_start == try_first (carrier)
    d.lock_advance = c.try_first[1] + c.frame_nsamples - c.nsamples_overscan;
    d.la_magic = d.lock_advance > 1 ? (uint32_t)( 0x100000000ULL / d.lock_advance ) : 0xFFFFFFFFu;
    d.nbits_magic = c.expect_n_bits > 1 ? (uint32_t)( 0x100000000ULL / c.expect_n_bits ) : 0xFFFFFFFFu;
    {
	// lowest candidate of the carrier coarse scan relative to its first try, rounded up to
	// whole bit lengths
	const unsigned down = zigzag_counts(c.try_first[1], c.try_max[1], c.try_step[1]).down * c.try_step[1];
	d.lock_back = ( down + c.bit_nsamples - 1 ) / c.bit_nsamples * c.bit_nsamples;
    }
    // every lattice window starts a multiple of 4 samples after the first one
    // when the bit length, all bit offsets and the frame step are multiples of
    // 4: then an unskewed region read with 16-byte LDS loads is conflict-light
    d.lat_linear = ( c.bit_nsamples % 4 == 0 && d.lock_advance % 4 == 0 ) ? 1u : 0u;
    for ( unsigned k = 0; k < c.expect_n_bits; k++ )
	if ( c.bit_offset[k] % 4 != 0 )
	    d.lat_linear = 0;
    d.lat_grid = ( d.lat_linear && c.expect_n_bits >= 2
		   && d.lock_advance == ( c.expect_n_bits - 1 ) * c.bit_nsamples ) ? 1u : 0u;
    for ( unsigned k = 0; k < c.expect_n_bits; k++ )
	if ( c.bit_offset[k] != k * c.bit_nsamples )
	    d.lat_grid = 0;
    for ( unsigned k = 0; k < c.expect_n_bits; k++ ) {
	d.bit_offset[k] = c.bit_offset[k];
	for ( int s = 0; s < 2; s++ ) {
	    const char ch = ( s ? c.expect_sync : c.expect_data )[k];
	    if ( ch != 'd' ) {
		d.req_mask[s] |= 1ULL << k;
		if ( ch == '1' )
		    d.req_val[s] |= 1ULL << k;
	    }
	}
    }
}

// ---- the launch plan of a batch: a pure function of PlanInputs and the experiment knobs ----

// Engine.  One wavefront per stream is the general engine (every option,
// every mode).  Where bit windows are staged through LDS and long enough
// that correlation, not the per-frame decisions, is the work (linear
// LATTICE, >= 16 samples per bit: Bell-202, 2400 baud, ...), the workgroup
// engine's master / worker pipeline overlaps the two and wins at every
// batch size measured (0.32 vs 0.52 ms at 512 streams, 0.50 vs 0.59 at
// 1024, 1.64 vs 2.19 at 4096); at 12000 baud (4 samples per bit) the
// wavefront engine is 4 x faster.  With longer windows and a clean signal it
// still wins (tools/gpu/eng50.py, 2048 streams: 50 baud 3.0 vs 4.4 ms, 150 baud
// 1.3 vs 4.1 ms).  Identical results either way.  (The workgroup engine has neither RING
// addressing nor the in-loop --auto-carrier, and accepts lattice frames without the reference's
// `advance <= samples_nvalid`: not where the lattice's own step exceeds half the reference's buffer,
// 4 and more stop bits.)
static bool use_workgroup_engine( const PlanInputs &in )
{
    const DevCfg &d = *in.cfg;
    const bool plain = !in.ring_exact && !in.autodetect
		    && ( in.samplebuf_size == 0u || d.lock_advance <= in.samplebuf_size / 2u );
    bool workgroup = plain && !( in.engine_flags & MIFSK_IO_ENGINE_WAVE )
		  && ( ( in.engine_flags & MIFSK_IO_ENGINE_WORKGROUP )
		       || ( d.lat_linear && d.bit_nsamples >= 16u ) );
    if ( const char *e = experiment_env("MIFSK_ENGINE") )	// diagnostic override: "workgroup" / "wave"
	if ( !( in.engine_flags & ( MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE ) ) )
	    workgroup = plain && e[0] == 'w' && e[1] == 'o';
    return workgroup;
}

namespace {

// ---- what the two engines' plans share -------------------------------------

// samples one search must see at once (+ slack for the chunked correlator)
uint32_t search_reach( const DevCfg &cfg )
{
    return ( cfg.try_max[0] > cfg.try_max[1] ? cfg.try_max[0] : cfg.try_max[1] ) + cfg.last_reach + 8u;
}

// floats of a skewed slab of `nsamp` samples (DevCfg::skew: a pad word per bit row)
size_t skewed_floats( const DevCfg &cfg, uint32_t nsamp )
{
    return ( (size_t)nsamp + (size_t)( nsamp / cfg.bit_nsamples + 2 ) * cfg.skew + 8 + 3 ) & ~(size_t)3;
}

// samples a skewed slab of `floats` floats holds in SCAN mode
uint32_t skewed_samples( const DevCfg &cfg, size_t floats )
{
    size_t ns = floats * cfg.bit_nsamples / ( cfg.bit_nsamples + cfg.skew );
    ns = ns > 16 ? ns - 16 : 0;
    return (uint32_t)( ns & ~(size_t)3 );
}

// distinct bit windows of the first F frames of a LATTICE block (on the grid the last window of
// a frame is the first of the next)
uint32_t block_wins( const DevCfg &cfg, uint32_t F )
{
    return cfg.lat_grid ? F * ( cfg.n_bits - 1u ) + 1u : F * cfg.n_bits;
}

// where window w of a block starts, relative to the block's first: windows numbered frame by
// frame, or -- `grid` -- along the one grid of bit lengths the frames share
uint32_t win_rel( const DevCfg &cfg, uint32_t w, bool grid )
{
    return grid ? w * cfg.bit_nsamples
		: ( w / cfg.n_bits ) * cfg.lock_advance + cfg.bit_offset[w % cfg.n_bits];
}

// window starts do not decrease in window order (a wave takes its span from its first and last lane)
bool starts_ordered( const DevCfg &cfg, uint32_t nwin, bool grid )
{
    bool ordered = true;
    for ( uint32_t w = 1; w < nwin; w++ )
	ordered = ordered && win_rel(cfg, w, grid) >= win_rel(cfg, w - 1, grid);
    return ordered;
}

// MIFSK_CHAIN = "G,K" (experiments and tests only) cuts any batch that may be chained; then the
// bounds of a cut: at most kMaxGroups groups, none empty, at least two chunks -- else (0, 0)
void chain_shape( bool allowed, int nstreams, uint32_t &groups, uint32_t &chunks )
{
    if ( const char *e = experiment_env("MIFSK_CHAIN") ) {
	int a = 0, b = 0;
	if ( allowed && std::sscanf(e, "%d,%d", &a, &b) == 2 ) {
	    groups = (uint32_t)( a < 0 ? 0 : a );
	    chunks = (uint32_t)( b < 0 ? 0 : b );
	}
    }
    if ( groups > (uint32_t)WaveChain::kMaxGroups ) groups = (uint32_t)WaveChain::kMaxGroups;
    if ( groups > (uint32_t)nstreams ) groups = (uint32_t)nstreams;
    if ( groups < 1u || chunks < 2u )
	groups = chunks = 0u;
}

// ---- one wavefront per stream: occupancy and LDS geometry per configuration ----

// Geometry for a staging width `sv` within `budget` bytes of LDS per wave (plan.wave, plan.lds_bytes);
// false when it does not fit.
bool wave_fit( const PlanInputs &in, int sv, size_t budget, LaunchPlan &plan, bool want_tile = false )
{
    const DevCfg &cfg = *in.cfg;
    const uint32_t B = cfg.bit_nsamples, nb = cfg.n_bits;
    WaveGeom g;
    std::memset(&g, 0, sizeof(g));
    const uint32_t round_floats = 64u * (uint32_t)sv * 4u;

    // The bulk path accepts a frame without looking at samples_nvalid: sound
    // when half the reference's buffer (what is always valid away from the end
    // of the stream) covers everything a carrier-held search reads and the
    // largest advance.
    const uint32_t half = in.samplebuf_size / 2u;
    const bool lattice_sound = !in.ring_exact
	&& half >= cfg.try_max[1] + cfg.last_reach
	&& half >= cfg.expect_nsamples + cfg.try_max[1]
	&& half > cfg.try_max[1] + cfg.frame_nsamples;
    g.lat_mode = lattice_sound ? LAT_DIRECT : LAT_NONE;
    g.lat_fmax = 64u;
    {
	uint32_t fmin = cfg.lat_grid ? 63u / ( nb - 1u ) : 64u / nb;	// one pass of lanes
	if ( fmin < 2u ) fmin = 2u;
	g.lat_fmin = fmin;
    }
    // LINEAR: window starts non-decreasing in window order and a round's span
    // within one staging pass
    if ( g.lat_mode != LAT_NONE && cfg.lat_linear ) {
	const uint32_t wtot = block_wins(cfg, 64u);
	const bool ordered = starts_ordered(cfg, wtot, cfg.lat_grid != 0u);
	uint32_t rw = 0;
	for ( uint32_t cand = 64u; ordered && cand <= 1024u; cand += 64u ) {
	    bool fits = true;
	    for ( uint32_t w0 = 0; w0 < wtot && fits; w0 += cand ) {
		const uint32_t w1 = w0 + cand < wtot ? w0 + cand : wtot;
		fits = win_rel(cfg, w1 - 1, cfg.lat_grid != 0u) + B - win_rel(cfg, w0, cfg.lat_grid != 0u) <= round_floats;
	    }
	    if ( !fits )
		break;
	    rw = cand;
	}
	if ( rw ) {
	    g.lat_mode = LAT_LINEAR;
	    g.round_wins = rw;
	}
    }

    const uint32_t slab_cap = ( search_reach(cfg) + 4u + 3u ) & ~3u;
    size_t scan_floats = skewed_floats(cfg, slab_cap);
    const size_t region_floats = g.lat_mode == LAT_LINEAR ? round_floats + 16u : 0u;
    if ( want_tile )
	scan_floats = 0;		// the tile instead of a slab

    for (;;) {
	// a SCAN chunk scores mags_cap / n_bits candidates at once: room for a
	// whole fine scan (<= 2 * 8 candidates) where it fits
	uint32_t mcap = g.lat_mode != LAT_NONE ? block_wins(cfg, g.lat_fmax) : 0u;
	if ( mcap < 16u * nb ) mcap = 16u * nb;
	g.mags_cap = ( mcap + 1u ) & ~1u;
	size_t sf = scan_floats > region_floats ? scan_floats : region_floats;
	// no SCAN slab: long windows go through a tile instead (corr_global_tiled)
	g.tiled = ( scan_floats == 0 && want_tile && !in.ring_exact && B >= TILE_K ) ? 1u : 0u;
	if ( g.tiled ) {
	    if ( g.lat_mode == LAT_LINEAR )
		g.lat_mode = LAT_DIRECT;	// (that instantiation has no staged rounds)
	    sf = TILE_FLOATS;
	    bool any = false;
	    for ( int i = 0; i < 4; i++ )
		any = any || cfg.seg[i].valid;
	    if ( any )			// shared segments: the carrier-held scans' plan words, the list of
		sf += 2u * ( 2u * SEG_MAX + SEG_MAX / 4u ) + 64u;	// windows to sum again (the partial sums lie on the tile)
	}
	const size_t total = kCntBytes + (size_t)g.mags_cap * 2u * sizeof(float) + sf * 4u + 16u;
	if ( total <= budget ) {
	    g.slab_floats = (uint32_t)sf;
	    g.slab_cap = 0;
	    if ( scan_floats ) {
		// the skewed slab may use the whole region
		g.slab_cap = skewed_samples(cfg, sf);
		if ( g.slab_cap < slab_cap )
		    g.slab_cap = slab_cap;
	    }
	    // DIRECT blocks of short windows (SAME) stream every lane's window from global memory,
	    // and the frames behind a refinement are read AGAIN by the block after it -- on a signal
	    // that is refined every fifth frame (SAME's 8-bit frames without start / stop bits) a
	    // block of a full pass of lanes (8 frames) throws three of them away: 2.3 x the
	    // algorithmic bytes moved, at 4.6 TB/s of fabric traffic.  A pass of lanes costs the
	    // same half full, so after a break the next block is as long as the lattice held last
	    // time, down to four frames (same-box: 7.46 -> 7.07 ms; 3, 5, 6: 7.23, 7.27, 7.21).
	    if ( g.lat_mode == LAT_DIRECT && !g.tiled && g.lat_fmin > 4u )
		g.lat_fmin = 4u;
	    if ( const char *e = experiment_env("MIFSK_LAT_FMIN") )	// experiments only
		if ( std::atoi(e) >= 1 )
		    g.lat_fmin = (uint32_t)std::atoi(e);
	    plan.wave.g = g;
	    plan.wave.sv = sv;
	    plan.lds_bytes = (uint32_t)total;
	    return true;
	}
	if ( g.lat_mode != LAT_NONE && g.lat_fmax / 2u >= g.lat_fmin && g.lat_fmax > 8u ) {
	    g.lat_fmax /= 2u;			// shorter blocks: fewer magnitude slots
	    continue;
	}
	if ( scan_floats > region_floats ) {
	    scan_floats = 0;			// SCAN streams its windows from global memory
	    continue;
	}
	return false;
    }
}

struct WaveKernelRow {
    int		sv, nq;
    bool	st, ra;
    const char	*name;
    uint32_t	waves_per_simd;
};
#define MIFSK_ROW(SV_, NQ_, ST_, RA_)										\
    { SV_, NQ_, ST_, RA_,											\
      ST_ ? "mifsk::demod_wave_kernel<" #SV_ ", " #NQ_ ", true>" : "mifsk::demod_wave_kernel<" #SV_ ", " #NQ_ ">",	\
      NQ_ == kTiled || SV_ >= 10 ? 2u : 4u },
const WaveKernelRow kWaveKernels[] = { MIFSK_WAVE_KERNELS(MIFSK_ROW) };
#undef MIFSK_ROW

// The instantiation a fit runs (its index in the list; -1: a staging width no instantiation
// has).  `nq`: the resident-table correlator of the bit length, where there is one (0: the
// generic correlators); `st`: resumable; `ra`: with RING addressing and --auto-carrier.
int wave_kernel( const LaunchPlan &plan, uint32_t nq, bool st, bool ra )
{
    const WaveGeom &g = plan.wave.g;
    const int sv = g.tiled ? 10 : plan.wave.sv;
    int want = g.tiled ? kTiled : g.lat_mode == LAT_LINEAR ? 0 : kDirect;
    if ( !st && !g.tiled && ( sv == 10 ? nq == 10u || nq == 5u : nq == 1u ) )
	want = (int)nq;
    for ( int i = 0; i < (int)( sizeof(kWaveKernels) / sizeof(kWaveKernels[0]) ); i++ )
	if ( kWaveKernels[i].sv == sv && kWaveKernels[i].nq == want && kWaveKernels[i].st == st && kWaveKernels[i].ra == ra )
	    return i;
    return -1;
}

int plan_wave( const PlanInputs &in, LaunchPlan &plan )
{
    const DevCfg &cfg = *in.cfg;
    const int ncu = in.ncu > 0 ? in.ncu : 256;
    // Waves per CU the batch can use (a wave is a workgroup): at least one per
    // SIMD, at most 16 (4 per SIMD at <= 128 VGPRs).  Each gets that share of
    // the CU's LDS; prefer the widest staging that fits, then fewer waves.
    uint32_t want = ( (uint32_t)in.nstreams + (uint32_t)ncu - 1u ) / (uint32_t)ncu;
    if ( want < 4u ) want = 4u;
    if ( want > 16u ) want = 16u;
    int force_sv = 0;
    if ( const char *e = experiment_env("MIFSK_WAVES_PER_CU") )	// experiments only
	want = (uint32_t)std::atoi(e) < 1u ? 1u : (uint32_t)std::atoi(e);
    if ( const char *e = experiment_env("MIFSK_SV") )
	force_sv = std::atoi(e);
    const WaveGeom &g = plan.wave.g;
    bool ok = false;
    // Long windows are better read through the tile at two waves per SIMD than
    // from a slab that leaves one wave per SIMD (tools/ubench/longwin.hip: 17 ms
    // against 45): a slab only while it fits 8 waves per CU then
    const bool tile_ok = !in.ring_exact && cfg.bit_nsamples >= kTileMinBit && force_sv != 4;
    const uint32_t wmin = tile_ok ? 8u : 4u;
    for ( uint32_t wpc = want; wpc >= wmin && !ok; wpc -= ( wpc > 8u ? 4u : ( wpc > 4u ? 2u : 1u ) ) ) {
	const size_t budget = ( kLdsPerCu / wpc ) & ~(size_t)255;
	// The wide-staging instantiation is compiled for two waves per SIMD (256
	// VGPRs): worth it where rounds are staged through LDS (linear LATTICE) or
	// where no more than 8 waves per CU are wanted anyway
	const bool wide = force_sv ? force_sv == 10 : ( wpc <= 8u || cfg.lat_linear );
	ok = wide && wave_fit(in, 10, budget, plan) && g.slab_cap != 0u
		  && ( g.lat_mode == LAT_LINEAR || wpc <= 8u || force_sv == 10 );
	if ( !ok )
	    ok = wave_fit(in, 4, budget, plan) && g.slab_cap != 0u;
	if ( wpc == 4u )
	    break;
    }
    if ( !ok && force_sv != 4 ) {
	// nothing keeps the SCAN slab in LDS (RTTY: 1056-sample windows, a 40 kB
	// span; 0.5 baud: 96000-sample windows): the windows come from global
	// memory through the tile (with the shared segments' plan words 12.9 kB), two waves per
	// SIMD: compiled for three (168 VGPRs) the instantiation spilled 44 VGPRs to scratch and
	// ran 4096 RTTY streams in 10.8 ms at 8 waves per CU; with 191 VGPRs and nothing spilled
	// the same 8 waves per CU take 9.3 ms (profiles/r03_history.md)
	for ( uint32_t wpc = want < 8u ? want : 8u; wpc >= 4u && !ok; wpc-- ) {
	    const size_t budget = ( kLdsPerCu / wpc ) & ~(size_t)255;
	    ok = wave_fit(in, 10, budget, plan, true) && g.tiled;
	}
    }
    if ( !ok ) {
	// ... or straight into registers, a window per lane
	const size_t budget = ( kLdsPerCu / want ) & ~(size_t)255;
	ok = wave_fit(in, 4, budget, plan);
	if ( !ok )
	    return -12;
    }
    const bool lin = g.lat_mode == LAT_LINEAR;
    // the resident-table correlator of the bit lengths that have one (linear LATTICE only)
    const uint32_t nq = ( lin && cfg.bit_nsamples % 4u == 0u ) ? cfg.bit_nsamples / 4u : 0u;
    // (RING addressing and --auto-carrier have their own instantiations: the plain ones carry
    // neither that code nor the registers it keeps alive; mifsk_demod_slab's all do)
    const bool ra = in.has_state || in.ring_exact || in.autodetect;
    // Chained launches (WaveChain, mifsk_device.h): where the plain instantiation is one of the
    // resumable ones, the batch is more than the chip holds at once and the streams are long
    // enough to cut (a chunk's last samplebuf waits for the next chunk: at least 8 per chunk).
    uint32_t &chain_g = plan.chain_groups, &chain_k = plan.chain_chunks;
    {
	const int plain = wave_kernel(plan, nq, false, ra);
	if ( plain < 0 )
	    return -22;
	const bool st_kernel = plain == wave_kernel(plan, 0u, false, ra);
	const uint64_t slots = (uint64_t)workgroups_per_cu(plan.lds_bytes, kWaveKernels[plain].waves_per_simd, 64u) * (uint64_t)ncu;
	const bool allowed = st_kernel && !in.has_state && !in.ring_exact && !in.has_counters && in.nstreams > 0;
	if ( allowed && (uint64_t)in.nstreams > slots && in.samplebuf_size > 0u ) {
	    chain_g = 2u;
	    chain_k = in.nsamples / ( 8u * in.samplebuf_size );
	    if ( chain_k > 8u ) chain_k = 8u;
	}
	chain_shape(allowed, in.nstreams, chain_g, chain_k);
    }
    // (mifsk_demod_slab and the chained launches: the instantiations with the state code)
    plan.resumable = in.has_state || chain_g;
    const int index = wave_kernel(plan, nq, plan.resumable, ra);
    if ( index < 0 )
	return -22;
    plan.engine = MIFSK_IO_ENGINE_WAVE;
    plan.kernel = (uint32_t)index;
    plan.kernel_name = kWaveKernels[index].name;
    plan.waves_per_simd = kWaveKernels[index].waves_per_simd;
    // Whole rounds.  A batch of more streams than waves fit runs in rounds, and a last round
    // that is a fraction of one leaves the chip mostly idle while its chains finish (4096 RTTY
    // streams at 12 waves per CU are 1.33 rounds: measured 13.8 ms against 13.3 at 8-10).  Among
    // the occupancies this plan allows (down to two thirds of the most) take the one that wastes
    // the fewest wave slots over the whole batch, the higher one on a tie; the kernel is limited
    // to it by its LDS allocation.  (Not for chained launches: their slots are refilled as they
    // come free.)
    {
	const uint32_t most = workgroups_per_cu(plan.lds_bytes, plan.waves_per_simd, 64u);
	const uint32_t per_cu = ( (uint32_t)( in.nstreams > 0 ? in.nstreams : 0 ) + (uint32_t)ncu - 1u ) / (uint32_t)ncu;
	if ( most >= 3u && per_cu > most && !chain_g ) {
	    uint32_t best = most, best_waste = 0xFFFFFFFFu;
	    for ( uint32_t w = most; 3u * w >= 2u * most; w-- ) {
		const uint32_t waste = ( per_cu + w - 1u ) / w * w - per_cu;
		if ( waste < best_waste ) {
		    best_waste = waste;
		    best = w;
		}
	    }
	    if ( best < most ) {
		const size_t pad = ( kLdsPerCu / best ) & ~(size_t)255;	// exactly `best` of these fit a CU
		if ( pad > plan.lds_bytes && kLdsPerCu / pad == best )
		    plan.lds_bytes = (uint32_t)pad;
	    }
	}
    }
    if ( const char *e = experiment_env("MIFSK_LDS_PAD") )	// experiments only: limit occupancy
	if ( (size_t)std::atoi(e) > plan.lds_bytes )
	    plan.lds_bytes = (uint32_t)std::atoi(e);
    plan.workgroup_size = 64u;
    plan.lattice_mode = g.lat_mode;
    plan.frames_per_block = g.lat_mode != LAT_NONE ? g.lat_fmax : 0u;
    return 0;
}

// ---- one workgroup per stream: a master wave and its workers ----------------

struct WgKernelRow {
    bool	use_slab, bell202, st;
    const char	*name;
    uint32_t	waves_per_simd;
};
#define MIFSK_ROW(WAVES_, SLAB_, BELL_, ST_, ...)	{ SLAB_, BELL_, ST_, "mifsk::demod_kernel<" #__VA_ARGS__ ">", WAVES_ },
const WgKernelRow kWgKernels[] = { MIFSK_WG_KERNELS(MIFSK_ROW) };
#undef MIFSK_ROW

// LDS geometry with `nworkers` workers: the kernel's arguments and its dynamic LDS
size_t wg_fit( const DevCfg &cfg, uint32_t nworkers, WgGeom &g )
{
    const uint32_t B = cfg.bit_nsamples;
    const uint32_t lat_lanes = nworkers * 64u;	// bit windows per lattice round
    const uint32_t reach = search_reach(cfg);
    // LDS budget: 4 workgroups per CU when the stream count can use them
    const size_t budget_small = kLdsPerCu / 4 - 64;

    // LATTICE geometry.  A round is as many frames as fill the worker lanes (64 per worker)
    // with distinct bit windows.  LINEAR workers stage their 64 windows' span in
    // a private LDS region (fastest; needs bit length, offsets and frame step
    // in multiples of 4 samples and the span to fit ten 16-byte loads per
    // lane); otherwise DIRECT workers stream each window from global memory.
    const uint32_t frames_max = cfg.lat_grid ? ( lat_lanes - 1u ) / ( cfg.n_bits - 1u )
					     : lat_lanes / cfg.n_bits;
    g.nworkers = nworkers;
    g.lat_frames = frames_max > P_CAP ? P_CAP : frames_max;
    g.lat_mode = g.lat_frames ? LAT_DIRECT : LAT_NONE;
    g.region_cap = g.region_floats = 0;
    if ( g.lat_frames && cfg.lat_linear && starts_ordered(cfg, g.lat_frames * cfg.n_bits, false) ) {
	// span of the widest wave: 64 windows (or all of them), plus what the
	// group-wise correlator (corr_lds_stream: whole groups of 16 samples) loads
	// beyond the last window -- nothing in the Bell-202 instantiation, whose
	// resident-table correlator reads the window and no more
	const uint32_t over = ( nworkers == 2u && B == 40u ) ? 0u : ( 16u - B % 16u ) % 16u;
	uint32_t span = 0;
	if ( cfg.lat_grid ) {
	    const uint32_t nwin = block_wins(cfg, g.lat_frames);
	    span = ( nwin < 64u ? nwin : 64u ) * B + over;
	} else {
	    const uint32_t nwin = g.lat_frames * cfg.n_bits;
	    for ( uint32_t w0 = 0; w0 < nwin; w0 += 64 ) {
		const uint32_t wl = w0 + 63 < nwin ? w0 + 63 : nwin - 1;
		const uint32_t len = win_rel(cfg, wl, false) + B - win_rel(cfg, w0, false);
		span = len > span ? len : span;
	    }
	    span += over;
	}
	g.region_cap = ( span + 3 ) & ~3u;
	g.region_floats = (uint32_t)skewed_floats(cfg, g.region_cap);
	if ( g.region_cap <= 64u * STAGE_VEC * 4u
		&& kWgLdsHeader + (size_t)nworkers * g.region_floats * 4 <= budget_small
		&& (size_t)nworkers * g.region_floats >= skewed_floats(cfg, reach + 4) )
	    g.lat_mode = LAT_LINEAR;
    }

    // the master scores `g.lat_rounds` rounds at once: halves the per-frame cost
    // of everything that is paid per batch -- the confidence pass, the barrier,
    // the command hand-off
    g.lat_rounds = 1;
    if ( g.lat_frames ) {
	g.lat_rounds = 2;
	if ( const char *e = experiment_env("MIFSK_LAT_ROUNDS") )	// experiments only
	    g.lat_rounds = (uint32_t)std::atoi(e) < 1u ? 1u : (uint32_t)std::atoi(e);
	while ( g.lat_rounds > 1 && ( g.lat_frames * g.lat_rounds > P_CAP
				    || block_wins(cfg, g.lat_frames) * g.lat_rounds > W_CAP ) )
	    g.lat_rounds--;
    }

    g.slab_cap = 0;
    size_t slab_floats = 0;
    g.use_slab = true;
    if ( g.lat_mode == LAT_LINEAR ) {
	slab_floats = (size_t)nworkers * g.region_floats;
	g.slab_cap = skewed_samples(cfg, slab_floats);
    } else {
	// no regions: the slab serves SCAN only; take what one search needs
	g.region_cap = 0;
	g.region_floats = 0;
	if ( kWgLdsHeader + skewed_floats(cfg, reach + 4) * 4 <= kLdsPerCu - 1024 ) {
	    g.slab_cap = ( reach + 4 + 3 ) & ~3u;
	    slab_floats = skewed_floats(cfg, g.slab_cap);
	} else {
	    g.use_slab = false;	// e.g. 0.5 baud: windows of 96000 samples; no lattice either
	    g.lat_mode = LAT_NONE;
	    g.lat_frames = 0;
	    g.lat_rounds = 1;
	}
    }
    return g.use_slab ? kWgLdsHeader + slab_floats * 4 : kWgLdsHeader + 16;
}

int plan_workgroup( const PlanInputs &in, LaunchPlan &plan )
{
    const DevCfg &cfg = *in.cfg;
    // Bell-202 (40 samples per bit, linear): two workers and the resident table, where that
    // geometry keeps the linear lattice; three workers otherwise
    WgGeom &g = plan.wg;
    size_t lds_all = 0;
    bool bell202 = false;
    if ( cfg.lat_linear && cfg.bit_nsamples == 40u ) {
	lds_all = wg_fit(cfg, 2u, g);
	bell202 = g.use_slab && g.lat_mode == LAT_LINEAR;
    }
    if ( !bell202 )
	lds_all = wg_fit(cfg, 3u, g);
    // Chained launches (as in plan_wave): the batch cut into G groups of
    // streams x K time chunks, each (group, chunk) its own grid of the RESUMABLE instantiation on
    // the group's stream.  The mechanism is the wavefront engine's and gives the single launch's
    // results bit for bit (tests/test_gpu_chain.py) -- but this engine's library default is ONE
    // launch at every batch size: its streams are short chains (0.45 ms for 10 s of Bell-202), the
    // dispatcher refills a finished workgroup's slot with the next stream anyway, and every chunk
    // restarts with a search and a pipeline fill.  Measured (tools/gpu/wg_chain_sizes.py,
    // profiles/r04_history.md): 1536 / 3000 / 5000 streams 0.825 / 1.43 / 2.16 ms in one launch,
    // 0.84-0.90 / 1.43-1.52 / 2.24-2.38 chained (2x2 ... 3x3).  MIFSK_CHAIN forces a cut
    // (experiments and tests).
    uint32_t &chain_g = plan.chain_groups, &chain_k = plan.chain_chunks;
    chain_shape(!in.has_state && !in.has_counters && in.nstreams > 0, in.nstreams, chain_g, chain_k);
    // (the cut is made by io.nsamples: with per-stream lengths only -- io.nsamples == 0 -- a
    // limit of 0 would mean "all samples" to every chunk but the last; such a batch is not cut)
    if ( in.nsamples == 0u )
	chain_g = chain_k = 0u;
    // The plain instantiations take `advance <= N - base` for the reference's `advance <= samples_nvalid`
    // (minimodem.c:1150-1152, where its loop ENDS otherwise): the same thing while no advance exceeds half
    // the reference's buffer, which is what is valid of it away from the end of the stream.  The buffer is
    // sized without the stop bits (minimodem.c:1056-1060): with 3 of them a frame is as long as that half,
    // and the advance behind a frame found late in its search longer -- the reference stops decoding there,
    // in mid stream.  Such configurations run the resumable instantiation, which carries the file position
    // and does the reference's buffer arithmetic statement for statement, here without a state record.
    const uint32_t reach = cfg.try_max[0] > cfg.try_max[1] ? cfg.try_max[0] : cfg.try_max[1];
    const bool flat_sound = in.samplebuf_size == 0u
			 || reach + cfg.frame_nsamples - cfg.overscan <= in.samplebuf_size / 2u;
    plan.resumable = in.has_state || chain_g || !flat_sound;
    int index = 0;		// (always found: Bell-202 has a slab)
    while ( index + 1 < (int)( sizeof(kWgKernels) / sizeof(kWgKernels[0]) )
	    && !( kWgKernels[index].use_slab == g.use_slab && kWgKernels[index].bell202 == bell202 && kWgKernels[index].st == plan.resumable ) )
	index++;
    plan.engine = MIFSK_IO_ENGINE_WORKGROUP;
    plan.kernel = (uint32_t)index;
    plan.kernel_name = kWgKernels[index].name;
    plan.waves_per_simd = kWgKernels[index].waves_per_simd;
    plan.workgroup_size = 64u * ( g.nworkers + 1u );
    plan.lds_bytes = (uint32_t)lds_all;
    plan.lattice_mode = g.lat_mode;
    plan.frames_per_block = g.lat_frames * g.lat_rounds;
    return 0;
}

} // namespace

int plan_launch( const PlanInputs &in, LaunchPlan &plan )
{
    std::memset(&plan, 0, sizeof(plan));
    return use_workgroup_engine(in) ? plan_workgroup(in, plan) : plan_wave(in, plan);
}

} // namespace mifsk
