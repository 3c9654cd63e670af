// mifsk_plan.cpp -- the host-side planner: what the kernels read of a receive configuration
// (DevCfg, mifsk_device.h), derived once per configuration and cached by the context.  Plain
// C++: nothing here touches the device.
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

} // namespace mifsk
