// mifsk_channel_kernel.h -- the channelizer's kernel and its launcher, for both of its sources:
// mifsk_channel.hip (the batch entries, STREAM = false) and mifsk_channel_stream.hip (rows fed in pieces,
// include/mifsk/channel_stream.h, STREAM = true).  One body, so that the pieces stay the whole bit for
// bit.  Not part of the ABI.
//
// One output sample is a window sum of carrier_survey_kernel's kind -- the complex sum kept, the
// rectangle replaced by a filter's taps, then rotated to the output tone -- so the kernel is laid
// out the same way around what feeds the FP64 pipe:
//   * a lane owns NC channels (c, c + cw) and kChO outputs: 2 * NC * kChO independent accumulator
//     chains.  G[k][t] does not depend on the output: ONE table read per channel and tap feeds
//     2 * kChO FMAs (4 * kChO with complex rows); a sample is the same for every channel: ONE
//     read per output and tap feeds 2 * NC (4 * NC) FMAs.
//   * the 64 lanes of a wave are cw channel lanes x 64 / cw groups of outputs, cw the power of two
//     that holds the channels (at most 64): three channels keep 64 lanes busy.  The four waves of
//     a workgroup take further groups of outputs of the same channels, channel blocks beyond
//     64 * NC are workgroups of their own (grid z).  A lane's outputs are NOG apart (NOG: the
//     workgroup's groups of outputs), so lanes of neighbouring groups read neighbouring samples
//     and, with few channel lanes, write neighbouring outputs; with 64 channel lanes every lane
//     of a wave stores to a row of its own (one store per T taps of work).
//   * G is uploaded transposed ([t][k]) and staged into LDS in tiles of tt taps as [t][NC][cw]:
//     the lanes of a wave read consecutive 16-byte entries, lanes of one channel the same one.
//   * the outputs of a chunk overlap whenever D < T: the chunk's span of samples for a tile of
//     taps, (outputs - 1) * D + tt, is staged once, widened to double (PCM16 converted on the way,
//     in float).  With D >= tt the tiles of the outputs do not overlap, and each output's tt
//     samples are staged at a stride of tt + 1 (odd: the lanes' reads fall on different banks).
//     Either way output ml of the chunk reads xs[ml * ss + e].
//   * W is read once per output and channel from memory (L2); the phase index walks from output to
//     output by additions mod P.
// The sums are the definition's in its order (re, im from 0.0, t ascending, one fma each).  No f64
// MFMA: its internal summation is not that chain.
//
// A stream keeps a record (seen, next: the elements it has seen and the next output it delivers;
// mifsk_channel_stream_check.h) and a tail: elements [next D, seen) of the capture as they came, T - 1 at
// most.  A feed runs the kernel over the VIRTUAL row that starts at element next D of the capture: the
// tail, then the piece (less its first next D - seen elements when the tail is empty and D > T has left
// a gap).  Output ml of the feed is output next + ml of the capture and reads virtual elements
// ml D + t.  What STREAM = true changes:
//   1. a row's length is 64 bits and comes from the record plus the piece: L + k_s passes 2^32 - 1
//      when a piece of 2^32 - 1 elements follows a tail.
//   2. the stager takes virtual element `at` from the tail (at < L) or from the piece (at - L + skip).
//      It goes to the same xs[i], so the LDS layout, its strides and the bank behaviour of the inner
//      loop are the batch rows'; the seam costs a compare and a select per staged sample, outside the
//      FMA loop.
//   3. the epilogue's phase walk starts at the absolute output index, ((next + m0 + ol) D) mod P, each
//      factor reduced mod P first, in 64 bits.
//   4. the workgroup of chunk 0 and channel block 0 of a stream writes the stream's new record and its
//      new tail, virtual elements [fit D, nv), the raw elements copied.
//   5. the arguments have five more fields (ChannelStreamArgs).
// No launch reads what it writes (records and tails exist twice, mifsk_stream_check.h).  So the
// kernel needs no fences, and any workgroup may write the new state while others still read the
// old.  The outputs are plain vector stores.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <type_traits>

#include "mifsk_channel_plan.h"
#include "mifsk_channel_stream_check.h"

namespace mifsk {

// ChannelArgs first, so a feed's rows and outputs lie where the batch kernel takes them; then the
// stream's five fields (mifsk_stream_check.h), the tails [nstreams][tail_cap] elements
struct ChannelStreamArgs : ChannelArgs, StreamSides<StreamRecord> {};

static_assert(sizeof(ChannelArgs) == 120 && sizeof(ChannelStreamArgs) == 120 + sizeof(StreamSides<StreamRecord>),
	      "rec_in at 120, tail_cap at 152, 160 bytes: the kernels' code reads them there");

// virtual element `at` of a stream, widened: tail [0, L), then the piece from its element `skip` on
template <bool CX, bool S16>
__device__ __forceinline__ auto stream_sample( const void *tail, const void *row, uint32_t L, uint64_t skip, uint64_t at )
{
    const bool old = at < L;
    return channel_sample<CX, S16>(old ? tail : row, old ? at : at - L + skip);
}

// NC: channels per lane.  CX: complex rows.  S16: PCM16 scalars.  IQ: the epilogue of
// mifsk_channelize_iq_batch (include/mifsk/channel_iq.h): rows are [out_stride] (I, Q) pairs, I the
// real entry's output, Q the other half of the same rotation, one 8-byte store for both.  (A
// parameter of this kernel, not a body shared by two kernels: inlined into a wrapper the IQ = false
// code comes out nine instructions longer, and it is to stay as it is.)  STREAM: rows fed in pieces.
// (Its branches are plain `if constexpr` statements on purpose: with the sample's source, or A,
// chosen by a lambda called on the spot, the staging loop of every instantiation comes out 7 to 11
// instructions longer.)
template <int NC, bool CX, bool S16, bool IQ, bool STREAM>
__global__ __launch_bounds__(256)
void channelize_kernel( const std::conditional_t<STREAM, ChannelStreamArgs, ChannelArgs> S )
{
    using OT = std::conditional_t<IQ, float2, float>;
    using XT = std::conditional_t<CX, double2, double>;
    // a raw element: 2, 4 or 8 bytes
    using ET = std::conditional_t<CX, std::conditional_t<S16, uint32_t, uint64_t>, std::conditional_t<S16, uint16_t, uint32_t>>;
    using NT = std::conditional_t<STREAM, uint64_t, uint32_t>;	// a row's length
    extern __shared__ double2 ch_lds[];
    const ChannelArgs &A = S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t T = A.T, D = A.D, K = A.K, P = A.P, tt = A.tt, ss = A.ss;
    const uint32_t cw = 1u << A.cwshift, cshift = A.cwshift + ( NC == 2 ? 1u : 0u ), C = 1u << cshift;
    const uint32_t ogw = 64u >> A.cwshift;			// groups of outputs in a wave
    const uint32_t NOG = kChWaves * ogw, OB = NOG * (uint32_t)kChO;	// ... and outputs in a chunk
    const uint32_t cl = lane & ( cw - 1u ), ol = wave * ogw + ( lane >> A.cwshift );
    // LDS: tt * C table entries [t][NC][cw] | (OB - 1) * ss + tt samples
    double2 *gl = ch_lds;
    XT *xs = reinterpret_cast<XT *>(ch_lds + (size_t)tt * C);
    const uint32_t R = ( OB - 1u ) * ss + tt;

    const uint32_t s = A.s0 + blockIdx.y, k0 = blockIdx.z * C;
    // (RowsIn::len(s), written out: with the member this kernel's code comes out three instructions
    // shorter, and it is to stay as it is)
    const uint32_t n_row = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    const uint32_t ks = n_row < A.in.stride ? n_row : (uint32_t)A.in.stride;	// elements the row holds: new ones
    const char *row = reinterpret_cast<const char *>(A.in.x) + (size_t)s * A.in.stride * sizeof(ET);
    const char *tail = nullptr;
    StreamRecord rec = {};
    uint32_t L = 0u;						// the tail's elements, T - 1 at most
    uint64_t skip = 0u;						// of the piece, read by nobody
    NT nv = ks;							// elements the (virtual) row holds
    if constexpr ( STREAM ) {
	// the virtual row: element 0 is element next * D of the capture
	tail = S.tail_in + (size_t)s * S.tail_cap * sizeof(ET);
	rec = S.rec_in[s];
	const uint64_t first = rec.next * D;
	L = rec.seen > first ? (uint32_t)( rec.seen - first ) : 0u;
	if ( L > S.tail_cap )					// (never: the tail's room is not left)
	    L = S.tail_cap;
	skip = first > rec.seen ? first - rec.seen : 0u;
	nv = ks > skip ? L + ( ks - skip ) : L;
    }
    // outputs that exist, of those the rows have room for: output m < cnt reads x[m D + t], t < T,
    // all below nv.  Of a stream every one is delivered (the host has seen to the room): `fit` of
    // them move the record, `cnt` are written
    const NT fit = nv >= T ? ( nv - T ) / D + 1u : 0u;
    const uint32_t cnt = fit < A.nout_cap ? (uint32_t)fit : A.nout_cap;
    const uint64_t m0 = (uint64_t)blockIdx.x * OB;
    if ( blockIdx.x == 0u )
	for ( uint32_t c = tid; c < C; c += blockDim.x )
	    if ( k0 + c < K )
		A.nout[(size_t)s * K + k0 + c] = cnt;

    uint32_t k[NC];
    double re[kChO][NC], im[kChO][NC];
#pragma unroll
    for ( int j = 0; j < NC; j++ ) {
	k[j] = k0 + (uint32_t)j * cw + cl;
#pragma unroll
	for ( int o = 0; o < kChO; o++ ) {
	    re[o][j] = 0.0;
	    im[o][j] = 0.0;
	}
    }
    if ( m0 < cnt ) {						// (the whole workgroup)
	const XT *xp = xs + ol * ss;
	const uint32_t os = NOG * ss;				// from one of the lane's outputs to the next
	for ( uint32_t t0 = 0; t0 < T; t0 += tt ) {
	    const uint32_t tl = T - t0 < tt ? T - t0 : tt;
	    __syncthreads();					// the tile before has been read
	    for ( uint32_t i = tid; i < tt * C; i += blockDim.x ) {
		const uint32_t e = i >> cshift, kk = k0 + ( i & ( C - 1u ) );
		double2 g = {0.0, 0.0};
		if ( e < tl && kk < K )
		    g = A.gt[(size_t)( t0 + e ) * K + kk];
		gl[i] = g;
	    }
	    for ( uint32_t i = tid; i < R; i += blockDim.x ) {
		uint64_t at;
		bool in = true;
		if ( D < tt )					// one span: output ml's tile starts at ml * D
		    at = m0 * D + t0 + i;
		else {						// a tile per output, ss = tt + 1 apart
		    const uint32_t ml = i / ss, e = i - ml * ss;
		    at = ( m0 + ml ) * D + t0 + e;
		    in = e < tt;
		}
		XT v = {};
		if ( in && at < nv ) {
		    if constexpr ( STREAM )
			v = stream_sample<CX, S16>(tail, row, L, skip, at);
		    else
			v = channel_sample<CX, S16>(row, at);
		}
		xs[i] = v;
	    }
	    __syncthreads();
#pragma unroll 2
	    for ( uint32_t e = 0; e < tl; e++ ) {
		double2 g[NC];
#pragma unroll
		for ( int j = 0; j < NC; j++ )
		    g[j] = gl[( e * (uint32_t)NC + (uint32_t)j ) * cw + cl];
#pragma unroll
		for ( int o = 0; o < kChO; o++ ) {
		    const XT x = xp[(uint32_t)o * os + e];
#pragma unroll
		    for ( int j = 0; j < NC; j++ ) {
			if constexpr ( CX ) {
			    re[o][j] = fma(x.x, g[j].x, re[o][j]);
			    re[o][j] = fma(-x.y, g[j].y, re[o][j]);
			    im[o][j] = fma(x.x, g[j].y, im[o][j]);
			    im[o][j] = fma(x.y, g[j].x, im[o][j]);
			} else {
			    re[o][j] = fma(x, g[j].x, re[o][j]);
			    im[o][j] = fma(x, g[j].y, im[o][j]);
			}
		    }
		}
	    }
	}
    }
    // p = (dq * ((m D) mod P)) mod P for m = m0 + ol + o NOG, of a stream the absolute m = next + m0 +
    // ol + o NOG: there every factor is reduced first, so no product passes 2^41.  From o to o + 1 it
    // grows by (dq * ((NOG D) mod P)) mod P
    uint32_t md0;
    if constexpr ( STREAM ) {
	const uint64_t mabs = ( rec.next % P + ( m0 + ol ) % P ) % P;
	md0 = (uint32_t)( ( mabs * ( D % P ) ) % P );
    } else
	md0 = (uint32_t)( ( ( m0 + ol ) * D ) % P );
    const uint32_t mdstep = (uint32_t)( ( (uint64_t)NOG * D ) % P );
#pragma unroll
    for ( int j = 0; j < NC; j++ ) {
	if ( k[j] >= K )
	    continue;
	const uint32_t dq = A.dq[k[j]];
	uint32_t p = (uint32_t)( ( (uint64_t)dq * md0 ) % P );
	const uint32_t pstep = (uint32_t)( ( (uint64_t)dq * mdstep ) % P );
	OT *out = reinterpret_cast<OT *>(A.rows) + ( (size_t)s * K + k[j] ) * A.out_stride;
#pragma unroll
	for ( int o = 0; o < kChO; o++ ) {
	    const uint64_t m = m0 + ol + (uint32_t)o * NOG;
	    if ( m < A.out_stride ) {
		OT v = {};
		if ( m < cnt ) {
		    const double2 w = A.w[p];
		    if constexpr ( IQ ) {
			v.x = (float)fma(re[o][j], w.x, -( im[o][j] * w.y ));
			v.y = (float)fma(re[o][j], w.y, im[o][j] * w.x);
		    } else
			v = (float)fma(re[o][j], w.x, -( im[o][j] * w.y ));
		}
		out[m] = v;
	    }
	    p += pstep;
	    if ( p >= P )
		p -= P;
	}
    }
    // the stream's other side: the record moved on, and what a later output can still read, virtual
    // elements [fit D, nv), as they came.  nv - fit D <= T - 1 (mifsk_channel_stream_check.h); with
    // k_s = 0 that is the tail and the record as they were.
    if constexpr ( STREAM ) {
	if ( blockIdx.x == 0u && blockIdx.z == 0u ) {
	    const uint64_t keep = fit * D;
	    uint64_t nt = nv > keep ? nv - keep : 0u;
	    if ( nt > S.tail_cap )					// (never)
		nt = S.tail_cap;
	    ET *to = reinterpret_cast<ET *>(S.tail_out + (size_t)s * S.tail_cap * sizeof(ET));
	    for ( uint32_t i = tid; i < (uint32_t)nt; i += blockDim.x ) {
		const uint64_t at = keep + i;
		const bool old = at < L;
		to[i] = reinterpret_cast<const ET *>(old ? tail : row)[old ? at : at - L + skip];
	    }
	    if ( tid == 0u )
		S.rec_out[s] = StreamRecord{rec.seen + ks, rec.next + fit};
	}
    }
}

// The launches of `plan`'s kernel over nstreams rows, A.s0 set for each: batch rows (Args:
// ChannelArgs) or the pieces of a channel stream (ChannelStreamArgs).  0 when all went out.
template <class Args>
inline int channel_launch( const mifsk_channel_plan &plan, const ChannelGeometry &g, size_t out_stride, int nstreams,
	Args &A, bool iq, hipStream_t st )
{
    constexpr bool STREAM = std::is_same_v<Args, ChannelStreamArgs>;
    if ( hipSetDevice(plan.device) != hipSuccess )
	return -EIO;
    const uint32_t nchunks = (uint32_t)( ( out_stride + g.OB - 1u ) / g.OB );
    const uint32_t gz = ( plan.K + g.C - 1u ) / g.C;
    return for_row_blocks((uint32_t)nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	const dim3 grid(nchunks, rows, gz), block(64u * kChWaves);
	auto launch = [&]( auto per_lane ) {
	    return dispatch_kind(plan.cx, plan.s16, [&]( auto cx, auto s16 ) {
		constexpr int NC = decltype(per_lane)::value;
		constexpr bool CX = decltype(cx)::value, S16 = decltype(s16)::value;
		return launch_lds(iq ? channelize_kernel<NC, CX, S16, true, STREAM> : channelize_kernel<NC, CX, S16, false, STREAM>,
				  grid, block, g.lds, st, A);
	    });
	};
	return g.nc == 2u ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 1>{});
    });
}

} // namespace mifsk
