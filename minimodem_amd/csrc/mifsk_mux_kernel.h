// mifsk_mux_kernel.h -- the multiplexer's kernel and its launcher, for both of its sources:
// mifsk_mux.hip (the batch entries, STREAM = false) and mifsk_mux_stream.hip (rows fed in pieces,
// include/mifsk/mux_stream.h, STREAM = true).  One body, so that the pieces stay the whole bit for bit.
// Not part of the ABI.
//
// One output n = m L + phi of one channel is a polyphase sum: the taps phi, phi + L, ... against the
// samples x[m], x[m - 1], ...  The kernel is laid out around what feeds the FP64 pipe:
//   * a lane owns kMxO outputs of ONE phase, n, n + L, ..., n + 7 L.  They share every G entry,
//     and their samples are a sliding window x[m - j + u]: one 16-byte table read and ONE new
//     sample per tap step feed 2 * kMxO FMAs.  The window lives in registers; the tap loop is
//     unrolled by kMxO so that the shift is a renaming.
//   * slot E = 256 * block + thread is group g = E div L, phase phi = E mod L; the slot's outputs
//     are (8 g + u) L + phi.  Lanes of a wave are consecutive slots: consecutive phases read
//     consecutive table entries and store consecutive outputs, lanes of one group read the same
//     sample (a broadcast), and with L < 64 a wave spans several groups, whose windows lie 8
//     samples apart -- the staged samples are padded by one double per 8 so that those reads fall
//     on different banks.
//   * channels run in the lane's loop in order, (o, oi) of each owned output in registers: the sum
//     over the channels is the definition's chain.  The block's span of each channel's row is
//     staged in LDS, widened to double once, for as many channels at a time as fit beside G
//     (which is staged whole: 16 B * T <= 64 KiB); a wave stages a channel, so the row and its
//     length are the wave's.  A tap step's table entry and sample are read a step ahead.
//   * a block whose span lies wholly inside a channel's row takes the window path; one that
//     overlaps an end of the row takes a path that tests every term (a term outside the row is
//     skipped, not multiplied by zero: the taps may be anything); one beyond the row has re = im =
//     0.0 without a look at the taps.
//   * W is read from memory (L2) once per output and channel; the phase index walks from n to
//     n + L by an addition mod P, and starts from a product reduced mod P in exact double
//     arithmetic (both factors are below 2^20).
// The kernel reads nothing it wrote, so it needs no fences; the outputs are plain vector stores.
// Blocks beyond the stream's outputs store zeros only; block 0 stores the count.
//
// A stream keeps a record (seen, first: the samples it has taken and the absolute index in front of
// which there are none; mifsk_mux_stream_check.h) and per row a tail, the row's last H = jmax - 1
// samples as they came.  A feed runs the kernel over the piece with LOCAL indices: output n of the feed
// is output seen L + n of the stream, sample i >= 0 is the piece's, sample i in [-H, 0) is tail element
// H + i.  What STREAM = true changes, all of it outside the tap loops:
//   1. the stager takes sample i from the piece (0 <= i < the row's length), +0.0 beyond the row's
//      length, or the tail (i < 0).  It goes to the same xs cell, so the padding, the spans and the bank
//      behaviour of the tap loops are the batch rows'.
//   2. every row's length is k_s = the stream's Nmax for the choice of the path (a shorter row has been
//      continued with +0.0), the lower existence test i >= 0 is i >= -back, back = min(seen - first, H)
//      from the record, and the count is k_s L.  The upper test i < k_s is not made for the choice of
//      the path: an output m < k_s reads no sample beyond k_s - 1, an output m >= k_s lies behind the
//      count and is stored as zero whatever its lane computed from the +0.0 staged there.  So the window
//      path runs everywhere but at a stream's start.
//   3. the phase start gets ((seen mod P) (L mod P)) mod P added mod P, in 64-bit integers.
//   4. the new record and the new tails, the last H elements of [old tail | piece continued to k_s],
//      go to the other side, ahead of the tap loops (so that nothing of it is live across them); the rows
//      of a stream are spread over all its workgroups, those that store only zeros included.  With k_s = 0 that is the record and the tails as they were.
//   5. the arguments have five more fields (MuxStreamArgs).
// No launch reads what it writes (records and tails exist twice, mifsk_stream_check.h).  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "mifsk_mux_plan.h"
#include "mifsk_mux_stream_check.h"

namespace mifsk {

// MuxArgs first, so a feed's rows and outputs lie where the batch kernel takes them; then the stream's
// five fields (mifsk_stream_check.h), the tails [nstreams * K][tail_cap] elements
struct MuxStreamArgs : MuxArgs, StreamSides<MuxStreamRecord> {};

static_assert(sizeof(MuxArgs) == 136 && sizeof(MuxStreamArgs) == 136 + sizeof(StreamSides<MuxStreamRecord>),
	      "rec_in at 136, tail_cap at 168, 176 bytes: the kernel's code reads them there");

// where sample e of a staged span lies: one double of padding per 8
__device__ __forceinline__ uint32_t mux_pad( uint32_t e ) { return e + ( e >> 3 ); }

// (a * b) mod P for a, b < P <= 2^20: the product is exact in double, the quotient off by one at most
__device__ __forceinline__ uint32_t mux_mulmod( uint32_t a, uint32_t b, uint32_t P, double inv_p )
{
    const double prod = (double)a * (double)b, dp = (double)P;
    double r = fma(-floor(prod * inv_p), dp, prod);
    if ( r < 0.0 )
	r += dp;
    if ( r >= dp )
	r -= dp;
    return (uint32_t)r;
}

// CX: complex rows.  S16: PCM16 scalars.  IQIN: the input rows of mifsk_multiplex_iq_batch
// (include/mifsk/mux_iq.h), (I, Q) pairs of floats.  A sample is staged as it is read, one 8-byte cell
// of two floats where a real row's sample is one double, so that the padding, the spans and the LDS
// sizing are the same and one ds_read_b64 per tap step still brings the new sample; both halves are
// widened at the read (exact, so where it happens does not matter) and the window holds 8 (I, Q) pairs
// of doubles: a tap step is 4 * kMxO FMAs.  A parameter of this kernel, not a body shared by two
// kernels (mifsk_channel_kernel.h says why): what the IQIN = false instantiations execute is the text it
// was.  STREAM: rows fed in pieces; its branches are plain `if constexpr` statements on purpose (a source
// chosen by a lambda called on the spot made the channelizer's staging loops 7 to 11 instructions longer).
template <bool CX, bool S16, bool IQIN, bool STREAM>
__global__ __launch_bounds__(256)
void multiplex_kernel( const std::conditional_t<STREAM, MuxStreamArgs, MuxArgs> S )
{
    using ET = std::conditional_t<IQIN, float2, float>;		// a raw input element
    extern __shared__ double2 mx_lds[];
    __shared__ uint32_t nmax_sh;
    const MuxArgs &A = S;
    const uint32_t tid = threadIdx.x;
    const uint32_t T = A.T, L = A.L, K = A.K, P = A.P, jmax = A.jmax;
    double2 *gl = mx_lds;					// T table entries | cb spans of samples
    double *xs = reinterpret_cast<double *>(mx_lds + T);

    const uint32_t s = A.s0 + blockIdx.y;
    const size_t row0 = (size_t)s * K;
    auto row_len = [&]( uint32_t k ) { return (uint32_t)A.in.len(row0 + k); };
    if ( tid == 0 )
	nmax_sh = 0u;
    __syncthreads();
    {
	uint32_t mine = 0u;
	for ( uint32_t k = tid; k < K; k += kMxThreads ) {
	    const uint32_t n = row_len(k);
	    mine = n > mine ? n : mine;
	}
	if ( mine )
	    atomicMax(&nmax_sh, mine);
    }
    for ( uint32_t t = tid; t < T; t += kMxThreads )
	gl[t] = A.g[t];
    __syncthreads();
    const uint32_t nmax = nmax_sh;				// of a stream: k_s
    const uint64_t total = STREAM ? (uint64_t)nmax * L : nmax ? (uint64_t)( nmax - 1u ) * L + T : 0ull;
    const uint32_t cnt = total < A.nout_cap ? (uint32_t)total : A.nout_cap;
    if ( blockIdx.x == 0u && tid == 0u )
	A.nout[s] = cnt;

    // of a stream: its record, the first sample that exists (local index, -back) and the phase of
    // its output seen * L
    int32_t low = 0;
    uint32_t pbase = 0u;
    if constexpr ( STREAM ) {
	const MuxStreamRecord rec = S.rec_in[s];
	low = -(int32_t)mux_stream_back(jmax - 1u, rec);
	pbase = (uint32_t)( ( ( rec.seen % P ) * (uint64_t)( L % P ) ) % P );
	// the stream's other side: the record moved on by k_s = nmax, and per row the last H elements of
	// [old tail | piece continued with +0.0 to k_s], local samples k_s - H .. k_s - 1, as they came.
	// The stream's workgroups take the rows in turns.
	const uint32_t H = jmax - 1u;
	for ( uint32_t k = blockIdx.x; k < K; k += gridDim.x ) {
	    const int64_t nk = row_len(k);
	    const ET *xr = reinterpret_cast<const ET *>(A.in.x) + ( row0 + k ) * A.in.stride;
	    const ET *tl = reinterpret_cast<const ET *>(S.tail_in) + ( row0 + k ) * S.tail_cap;
	    ET *to = reinterpret_cast<ET *>(S.tail_out) + ( row0 + k ) * S.tail_cap;
	    for ( uint32_t t = tid; t < H; t += kMxThreads ) {
		const int64_t i = (int64_t)nmax - (int64_t)H + t;
		ET v = {};
		if ( i < 0 )
		    v = tl[(int64_t)H + i];
		else if ( i < nk )
		    v = xr[i];
		to[t] = v;
	    }
	}
	// (ahead of the tap loops, so that nothing of this is kept in registers across them)
	if ( blockIdx.x == 0u && tid == 0u )
	    S.rec_out[s] = MuxStreamRecord{rec.seen + nmax, rec.first};
    }

    // this lane's slot, and the groups of the block
    const uint64_t e0 = (uint64_t)blockIdx.x * kMxThreads;
    const uint64_t g_first = e0 / L, g_last = ( e0 + kMxThreads - 1u ) / L;
    const uint64_t g = ( e0 + tid ) / L;
    const uint32_t phi = (uint32_t)( ( e0 + tid ) - g * L );
    const int64_t m0 = (int64_t)( g * kMxO );			// the lane's first m
    const uint64_t n0 = (uint64_t)m0 * L + phi;			// ... and first output
    const int64_t lo = (int64_t)( g_first * kMxO ) - (int64_t)( jmax - 1u );	// the block's span of samples
    const int64_t hi = (int64_t)( g_last * kMxO ) + ( kMxO - 1 );
    const uint32_t span = (uint32_t)( hi - lo + 1 );		// <= A.span
    const uint32_t xb = (uint32_t)( m0 - lo );			// >= jmax - 1

    double o[kMxO], oi[kMxO];
#pragma unroll
    for ( int u = 0; u < kMxO; u++ ) {
	o[u] = 0.0;
	oi[u] = 0.0;
    }
    if ( g_first * kMxO * L < cnt ) {				// (the whole workgroup)
	const double inv_p = 1.0 / (double)P;
	uint32_t nm0 = (uint32_t)( n0 % P );
	if constexpr ( STREAM ) {
	    nm0 += pbase;
	    if ( nm0 >= P )
		nm0 -= P;
	}
	for ( uint32_t k0 = 0; k0 < K; k0 += A.cb ) {
	    const uint32_t cbn = K - k0 < A.cb ? K - k0 : A.cb;
	    __syncthreads();					// the spans before have been read
	    // a wave per channel: the row and its length are the wave's, the lanes read along the row
	    for ( uint32_t c = tid >> 6; c < cbn; c += kMxThreads / 64u ) {
		const int64_t nk = row_len(k0 + c);
		if constexpr ( STREAM ) {
		    // lo >= -(jmax - 1): tail element jmax - 1 + i exists in the tail's room for every i < 0
		    const ET *xr = reinterpret_cast<const ET *>(A.in.x) + ( row0 + k0 + c ) * A.in.stride;
		    const ET *tl = reinterpret_cast<const ET *>(S.tail_in) + ( row0 + k0 + c ) * S.tail_cap;
		    for ( uint32_t e = tid & 63u; e < span; e += 64u ) {
			const int64_t i = lo + e;
			ET v = {};
			if ( i < 0 )
			    v = tl[(int64_t)( jmax - 1u ) + i];
			else if ( i < nk )
			    v = xr[i];
			if constexpr ( IQIN )
			    ( reinterpret_cast<float2 *>(xs) + (size_t)c * A.spanp )[mux_pad(e)] = v;
			else
			    ( xs + (size_t)c * A.spanp )[mux_pad(e)] = (double)v;
		    }
		} else
		if constexpr ( IQIN ) {
		    const float2 *xr = reinterpret_cast<const float2 *>(A.in.x) + ( row0 + k0 + c ) * A.in.stride;
		    float2 *xc = reinterpret_cast<float2 *>(xs) + (size_t)c * A.spanp;
		    for ( uint32_t e = tid & 63u; e < span; e += 64u ) {
			const int64_t i = lo + e;
			xc[mux_pad(e)] = i >= 0 && i < nk ? xr[i] : float2{0.0f, 0.0f};
		    }
		} else {
		const float *xr = reinterpret_cast<const float *>(A.in.x) + ( row0 + k0 + c ) * A.in.stride;
		double *xc = xs + (size_t)c * A.spanp;
		for ( uint32_t e = tid & 63u; e < span; e += 64u ) {
		    const int64_t i = lo + e;
		    xc[mux_pad(e)] = i >= 0 && i < nk ? (double)xr[i] : 0.0;
		}
		}
	    }
	    __syncthreads();
	    for ( uint32_t c = 0; c < cbn; c++ ) {
		const uint32_t k = k0 + c;
		const int64_t nk = STREAM ? (int64_t)nmax : (int64_t)row_len(k);
		const double *xc = xs + (size_t)c * A.spanp;
		double re[kMxO], im[kMxO];
		double2 w[kMxO];
		// p = (dq * (n mod P)) mod P; from n to n + L it grows by ps = (dq * (L mod P)) mod P.
		// W is asked for here, ahead of the taps, and used behind them.
		{
		    uint32_t p = mux_mulmod(A.dq[k], nm0, P, inv_p);
		    const uint32_t ps = A.ps[k];
#pragma unroll
		    for ( int u = 0; u < kMxO; u++ ) {
			w[u] = A.w[p];
			p += ps;
			if ( p >= P )
			    p -= P;
		    }
		}
#pragma unroll
		for ( int u = 0; u < kMxO; u++ ) {
		    re[u] = 0.0;
		    im[u] = 0.0;
		}
		if constexpr ( IQIN ) {
		    const float2 *xq = reinterpret_cast<const float2 *>(xs) + (size_t)c * A.spanp;
		    if ( lo >= low && ( STREAM || hi < nk ) ) {
			// the window path of real rows below, a slot (I, Q) as two doubles
			double wa[kMxO], wb[kMxO];
#pragma unroll
			for ( int u = 0; u < kMxO; u++ ) {
			    const float2 v = xq[mux_pad(xb + (uint32_t)u)];
			    wa[u] = (double)v.x;
			    wb[u] = (double)v.y;
			}
			uint32_t t = phi;
			double2 gn = gl[t < T ? t : T - 1u];
			float2 xn = float2{0.0f, 0.0f};
			for ( uint32_t j0 = 0; j0 < jmax; j0 += (uint32_t)kMxO ) {
#pragma unroll
			    for ( int r = 0; r < kMxO; r++ ) {
				const uint32_t j = j0 + (uint32_t)r, tn = t + L;
				const double2 gt = gn;
				if ( r > 0 || j0 > 0u ) {
				    wa[( kMxO - r ) & 7] = (double)xn.x;		// x[m0 - j]
				    wb[( kMxO - r ) & 7] = (double)xn.y;
				}
				gn = gl[tn < T ? tn : T - 1u];
				xn = xq[mux_pad(xb - ( j + 1u < jmax ? j + 1u : jmax - 1u ))];
				if ( t < T ) {
#pragma unroll
				    for ( int u = 0; u < kMxO; u++ ) {
					const double a = wa[( u - r ) & 7], b = wb[( u - r ) & 7];
					re[u] = fma(a, gt.x, re[u]);
					re[u] = fma(-b, gt.y, re[u]);
					im[u] = fma(a, gt.y, im[u]);
					im[u] = fma(b, gt.x, im[u]);
				    }
				}
				t = tn;
			    }
			}
		    } else if ( lo < nk ) {
			uint32_t t = phi;
			for ( uint32_t j = 0; j < jmax && t < T; j++, t += L ) {
			    const double2 gt = gl[t];
#pragma unroll
			    for ( int u = 0; u < kMxO; u++ ) {
				const int64_t i = m0 + u - (int64_t)j;
				if ( i >= low && i < nk ) {
				    const float2 v = xq[mux_pad(xb + (uint32_t)u - j)];
				    const double a = (double)v.x, b = (double)v.y;
				    re[u] = fma(a, gt.x, re[u]);
				    re[u] = fma(-b, gt.y, re[u]);
				    im[u] = fma(a, gt.y, im[u]);
				    im[u] = fma(b, gt.x, im[u]);
				}
			    }
			}
		    }
		} else
		if ( lo >= low && ( STREAM || hi < nk ) ) {
		    // every term of every lane exists: the window in registers, slot (v & 7) holds
		    // x[m0 + v] for the 8 values of v in use
		    double win[kMxO];
#pragma unroll
		    for ( int u = 0; u < kMxO; u++ )
			win[u] = xc[mux_pad(xb + (uint32_t)u)];
		    // The table entry and the sample of a step are fetched a step ahead, outside any
		    // test (their indices are clamped into the table and the span), so that the reads
		    // are in flight during the FMAs before them; what a lane past its last tap fetches
		    // or puts into the window is never used.
		    uint32_t t = phi;
		    double2 gn = gl[t < T ? t : T - 1u];
		    double xn = 0.0;
		    for ( uint32_t j0 = 0; j0 < jmax; j0 += (uint32_t)kMxO ) {
#pragma unroll
			for ( int r = 0; r < kMxO; r++ ) {
			    const uint32_t j = j0 + (uint32_t)r, tn = t + L;
			    const double2 gt = gn;
			    if ( r > 0 || j0 > 0u )
				win[( kMxO - r ) & 7] = xn;		// x[m0 - j]
			    gn = gl[tn < T ? tn : T - 1u];
			    xn = xc[mux_pad(xb - ( j + 1u < jmax ? j + 1u : jmax - 1u ))];
			    if ( t < T ) {
#pragma unroll
				for ( int u = 0; u < kMxO; u++ ) {
				    re[u] = fma(win[( u - r ) & 7], gt.x, re[u]);
				    im[u] = fma(win[( u - r ) & 7], gt.y, im[u]);
				}
			    }
			    t = tn;
			}
		    }
		} else if ( lo < nk ) {
		    // an end of the row inside the span: term by term
		    uint32_t t = phi;
		    for ( uint32_t j = 0; j < jmax && t < T; j++, t += L ) {
			const double2 gt = gl[t];
#pragma unroll
			for ( int u = 0; u < kMxO; u++ ) {
			    const int64_t i = m0 + u - (int64_t)j;
			    if ( i >= low && i < nk ) {
				const double x = xc[mux_pad(xb + (uint32_t)u - j)];
				re[u] = fma(x, gt.x, re[u]);
				im[u] = fma(x, gt.y, im[u]);
			    }
			}
		    }
		}
		if ( A.gains ) {
		    const double gain = (double)A.gains[k];
#pragma unroll
		    for ( int u = 0; u < kMxO; u++ ) {
			re[u] = re[u] * gain;
			im[u] = im[u] * gain;
		    }
		}
#pragma unroll
		for ( int u = 0; u < kMxO; u++ ) {
		    o[u] = fma(re[u], w[u].x, o[u]);
		    o[u] = fma(-im[u], w[u].y, o[u]);
		    if constexpr ( CX ) {
			oi[u] = fma(re[u], w[u].y, oi[u]);
			oi[u] = fma(im[u], w[u].x, oi[u]);
		    }
		}
	    }
	}
    }
    char *out = reinterpret_cast<char *>(A.out) + (size_t)s * A.out_stride * ( ( S16 ? 2u : 4u ) * ( CX ? 2u : 1u ) );
#pragma unroll
    for ( int u = 0; u < kMxO; u++ ) {
	const uint64_t n = n0 + (uint64_t)u * L;
	if ( n >= A.out_stride )
	    continue;
	const float vr = n < cnt ? (float)o[u] : 0.0f, vi = n < cnt ? (float)oi[u] : 0.0f;
	if constexpr ( CX ) {
	    if constexpr ( S16 )
		reinterpret_cast<short2 *>(out)[n] = short2{n < cnt ? rows_s16(vr) : (int16_t)0, n < cnt ? rows_s16(vi) : (int16_t)0};
	    else
		reinterpret_cast<float2 *>(out)[n] = float2{vr, vi};
	} else {
	    if constexpr ( S16 )
		reinterpret_cast<int16_t *>(out)[n] = n < cnt ? rows_s16(vr) : (int16_t)0;
	    else
		reinterpret_cast<float *>(out)[n] = vr;
	}
    }
}

// The launches of `plan`'s kernel over nstreams streams, A.s0 set for each: batch rows (Args: MuxArgs)
// or the pieces of a multiplexer stream (MuxStreamArgs).  `iq`: the input rows are (I, Q) pairs of
// floats and the kernel is the IQIN one.  0 when all went out.
template <class Args>
inline int mux_launch( const mifsk_mux_plan &plan, const MuxGeometry &geo, int nstreams, Args &A, bool iq, hipStream_t st )
{
    constexpr bool STREAM = std::is_same_v<Args, MuxStreamArgs>;
    if ( hipSetDevice(plan.device) != hipSuccess )
	return -EIO;
    return for_row_blocks((uint32_t)nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	return dispatch_kind(plan.cx, plan.s16, [&]( auto cx, auto s16 ) {
	    constexpr bool CX = decltype(cx)::value, S16 = decltype(s16)::value;
	    return launch_lds(iq ? multiplex_kernel<CX, S16, true, STREAM> : multiplex_kernel<CX, S16, false, STREAM>,
			      dim3(geo.nblocks, rows, 1), dim3(kMxThreads), geo.lds, st, A);
	});
    });
}

} // namespace mifsk
