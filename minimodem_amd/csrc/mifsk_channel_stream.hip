// mifsk_channel_stream.hip -- the channelizer fed in pieces (include/mifsk/channel_stream.h):
// mifsk_channel_stream_create / _destroy / _feed / _seek / _seen and the host's
// mifsk_channel_stream_outputs.
//
// A stream keeps a record (seen, next: the elements it has seen and the next output it delivers;
// mifsk_channel_stream_check.h) and a tail: elements [next D, seen) of the capture as they came, T - 1 at
// most.  A feed's kernel is channelize_kernel (mifsk_channel.hip) over the VIRTUAL row that starts at
// element next D of the capture: the tail, then the piece (less its first next D - seen elements when
// the tail is empty and D > T has left a gap).  Output ml of the feed is output next + ml of the
// capture and reads virtual elements ml D + t.  What differs from the batch kernel:
//   * the stager takes virtual element `at` from the tail (at < L) or from the piece (at - L + skip).
//     Only the source of a staged sample changes: it goes to the same xs[i], so the LDS layout, its
//     strides (D, or tt + 1: odd) and with them the bank behaviour of the inner loop are the batch
//     kernel's.  The seam costs a compare and a select per staged sample, outside the FMA loop.
//   * a row's length is 64 bits: L + k_s passes 2^32 - 1 when a piece of 2^32 - 1 elements follows a tail.
//   * the epilogue's phase walk starts at ((next + m0 + ol) D) mod P, each factor reduced mod P first,
//     in 64 bits, so it is the absolute m's at any index.
//   * the workgroup of chunk 0 and channel block 0 of a stream writes the stream's new record and its
//     new tail, virtual elements [cnt D, nv), the raw elements copied.
// No launch reads what it writes: records and tails exist twice, a feed reads side `parity` and
// writes the other (as session_append_kernel does), and the host flips the parity after a launch
// that went out whole.  So the kernel needs no fences, and any workgroup may write the new state
// while others still read the old.  Plain vector stores; no f64 MFMA, whose internal summation is
// not the definition's chain.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <memory>
#include <new>
#include <type_traits>

#include "mifsk.h"
#include "mifsk/channel_stream.h"
#include "mifsk_channel_plan.h"
#include "mifsk_channel_stream_check.h"

namespace mifsk {

struct ChannelStreamArgs {
    ChannelArgs		c;		// the piece's rows and the outputs, as the batch kernel takes them
    const StreamRecord	*rec_in;	// [nstreams]: the side this feed reads
    StreamRecord	*rec_out;	// ... and the one it writes
    const char		*tail_in;	// [nstreams][tail_cap] elements
    char		*tail_out;
    uint32_t		tail_cap;	// elements of a tail's room
};

// virtual element `at` of a stream, widened: tail [0, L), then the piece from its element `skip` on
template <bool CX, bool S16>
__device__ __forceinline__ auto stream_sample( const void *tail, const void *row, uint32_t L, uint64_t skip, uint64_t at )
{
    const bool old = at < L;
    return channel_sample<CX, S16>(old ? tail : row, old ? at : at - L + skip);
}

template <int NC, bool CX, bool S16, bool IQ>
__global__ __launch_bounds__(256)
void channel_stream_kernel( const ChannelStreamArgs S )
{
    using OT = std::conditional_t<IQ, float2, float>;
    using XT = std::conditional_t<CX, double2, double>;
    // a raw element: 2, 4 or 8 bytes
    using ET = std::conditional_t<CX, std::conditional_t<S16, uint32_t, uint64_t>, std::conditional_t<S16, uint16_t, uint32_t>>;
    extern __shared__ double2 chs_lds[];
    const ChannelArgs &A = S.c;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t T = A.T, D = A.D, K = A.K, P = A.P, tt = A.tt, ss = A.ss;
    const uint32_t cw = 1u << A.cwshift, cshift = A.cwshift + ( NC == 2 ? 1u : 0u ), C = 1u << cshift;
    const uint32_t ogw = 64u >> A.cwshift;			// groups of outputs in a wave
    const uint32_t NOG = kChWaves * ogw, OB = NOG * (uint32_t)kChO;	// ... and outputs in a chunk
    const uint32_t cl = lane & ( cw - 1u ), ol = wave * ogw + ( lane >> A.cwshift );
    // LDS: tt * C table entries [t][NC][cw] | (OB - 1) * ss + tt samples
    double2 *gl = chs_lds;
    XT *xs = reinterpret_cast<XT *>(chs_lds + (size_t)tt * C);
    const uint32_t R = ( OB - 1u ) * ss + tt;

    const uint32_t s = A.s0 + blockIdx.y, k0 = blockIdx.z * C;
    const uint32_t n_row = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    const uint32_t ks = n_row < A.in.stride ? n_row : (uint32_t)A.in.stride;	// new elements
    const char *row = reinterpret_cast<const char *>(A.in.x) + (size_t)s * A.in.stride * sizeof(ET);
    const char *tail = S.tail_in + (size_t)s * S.tail_cap * sizeof(ET);
    // the virtual row: element 0 is element next * D of the capture
    const StreamRecord rec = S.rec_in[s];
    const uint64_t first = rec.next * D;
    uint32_t L = rec.seen > first ? (uint32_t)( rec.seen - first ) : 0u;	// the tail's elements, T - 1 at most
    if ( L > S.tail_cap )						// (never: the tail's room is not left)
	L = S.tail_cap;
    const uint64_t skip = first > rec.seen ? first - rec.seen : 0u;	// of the piece, read by nobody
    const uint64_t nv = ks > skip ? L + ( ks - skip ) : L;		// elements the virtual row holds
    // outputs that exist: M(seen + ks) - next, every one delivered (the host has seen to the room);
    // `fit` of them move the record, `cnt` are written
    const uint64_t fit = nv >= T ? ( nv - T ) / D + 1u : 0u;
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
		if ( in && at < nv )
		    v = stream_sample<CX, S16>(tail, row, L, skip, at);
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
    // p = (dq * ((m D) mod P)) mod P for the absolute m = next + m0 + ol + o NOG: every factor reduced
    // first, so no product passes 2^41; from o to o + 1 it grows by (dq * ((NOG D) mod P)) mod P
    const uint64_t mabs = ( rec.next % P + ( m0 + ol ) % P ) % P;
    const uint32_t md0 = (uint32_t)( ( mabs * ( D % P ) ) % P ), mdstep = (uint32_t)( ( (uint64_t)NOG * D ) % P );
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
    if ( blockIdx.x == 0u && blockIdx.z == 0u ) {
	const uint64_t keep = fit * D;
	uint64_t nt = nv > keep ? nv - keep : 0u;
	if ( nt > S.tail_cap )						// (never)
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

} // namespace mifsk

struct mifsk_channel_stream {
    const mifsk_channel_plan		*plan;
    int					nstreams;
    uint32_t				tail_cap;	// elements per stream and side
    uint32_t				esz;		// bytes of an element
    unsigned				parity;		// the side the next feed reads
    mifsk::DevMem<mifsk::StreamRecord>	rec;		// [2][nstreams]
    mifsk::DevMem<char>			tails;		// [2][nstreams][tail_cap] elements
};

extern "C" uint64_t mifsk_channel_stream_outputs( uint32_t ntaps, uint32_t decim, uint64_t seen, uint64_t k )
{
    return mifsk::stream_outputs(ntaps, decim, seen, k);
}

extern "C" int mifsk_channel_stream_create( const mifsk_channel_plan *plan, int nstreams, mifsk_channel_stream **out )
{
    using namespace mifsk;
    if ( !plan || !out || nstreams <= 0 )
	return -EINVAL;
    std::unique_ptr<mifsk_channel_stream> cs(new (std::nothrow) mifsk_channel_stream);
    if ( !cs )
	return -ENOMEM;
    cs->plan = plan;
    cs->nstreams = nstreams;
    cs->esz = ( plan->s16 ? 2u : 4u ) * ( plan->cx ? 2u : 1u );
    cs->tail_cap = stream_tail_cap(plan->T, cs->esz);
    cs->parity = 0u;
    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    if ( int rc = cs->rec.alloc(2u * (size_t)nstreams, 0, true) )
	return rc;
    if ( int rc = cs->tails.alloc(2u * (size_t)nstreams * cs->tail_cap * cs->esz, 0, true) )
	return rc;
    *out = cs.release();
    return 0;
}

extern "C" void mifsk_channel_stream_destroy( mifsk_channel_stream *cs )
{
    if ( !cs )
	return;
    (void)hipSetDevice(cs->plan->device);
    (void)hipDeviceSynchronize();		// no kernel reads the tails any more
    delete cs;
}

extern "C" int mifsk_channel_stream_feed( mifsk_channel_stream *cs, const mifsk_channel_io *io, uint32_t flags, void *stream )
{
    using namespace mifsk;
    if ( !cs || !io )
	return -EINVAL;
    const mifsk_channel_plan *plan = cs->plan;
    if ( int rc = stream_feed_check(StreamShape{plan->cx, plan->s16, plan->D, plan->K, cs->nstreams}, io, flags) )
	return rc;
    const bool iq = ( flags & MIFSK_CHANNEL_STREAM_IQ ) != 0u;

    const ChannelGeometry g = channel_geometry(*plan);
    ChannelStreamArgs S = {};
    S.c = channel_args(*plan, io, g);
    const size_t n = (size_t)cs->nstreams, side = n * cs->tail_cap * cs->esz;
    S.rec_in = cs->rec.p + cs->parity * n;
    S.rec_out = cs->rec.p + ( cs->parity ^ 1u ) * n;
    S.tail_in = cs->tails.p + cs->parity * side;
    S.tail_out = cs->tails.p + ( cs->parity ^ 1u ) * side;
    S.tail_cap = cs->tail_cap;

    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    const uint32_t nchunks = (uint32_t)( ( io->out_stride + g.OB - 1u ) / g.OB );
    const uint32_t gz = ( plan->K + g.C - 1u ) / g.C;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	S.c.s0 = s0;
	const dim3 grid(nchunks, rows, gz), block(64u * kChWaves);
	auto launch = [&]( auto per_lane ) {
	    return dispatch_kind(plan->cx, plan->s16, [&]( auto cx, auto s16 ) {
		constexpr int NC = decltype(per_lane)::value;
		constexpr bool CX = decltype(cx)::value, S16 = decltype(s16)::value;
		return launch_lds(iq ? channel_stream_kernel<NC, CX, S16, true> : channel_stream_kernel<NC, CX, S16, false>,
				  grid, block, g.lds, st, S);
	    });
	};
	return g.nc == 2u ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 1>{});
    });
    // (a feed that did not go out whole leaves the side it read as the current one)
    if ( rc == 0 )
	cs->parity ^= 1u;
    return rc;
}

extern "C" int mifsk_channel_stream_seek( mifsk_channel_stream *cs, const uint64_t *seen, void *stream )
{
    using namespace mifsk;
    if ( !cs )
	return -EINVAL;
    const size_t n = (size_t)cs->nstreams;
    const std::unique_ptr<StreamRecord[]> rec(new (std::nothrow) StreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    for ( size_t s = 0; s < n; s++ ) {
	if ( seen && seen[s] > kStreamMaxSeen )
	    return -EINVAL;
	rec[s] = stream_record_at(cs->plan->D, seen ? seen[s] : 0u);
    }
    // behind the feeds queued on `stream`; the records are there when this returns
    if ( hipSetDevice(cs->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    return hipMemcpy(cs->rec.p + cs->parity * n, rec.get(), n * sizeof(StreamRecord), hipMemcpyHostToDevice) == hipSuccess
	? 0 : -EIO;
}

extern "C" int mifsk_channel_stream_seen( mifsk_channel_stream *cs, uint64_t *seen_out, void *stream )
{
    using namespace mifsk;
    if ( !cs || !seen_out )
	return -EINVAL;
    const size_t n = (size_t)cs->nstreams;
    const std::unique_ptr<StreamRecord[]> rec(new (std::nothrow) StreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    if ( hipSetDevice(cs->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    if ( hipMemcpy(rec.get(), cs->rec.p + cs->parity * n, n * sizeof(StreamRecord), hipMemcpyDeviceToHost) != hipSuccess )
	return -EIO;
    for ( size_t s = 0; s < n; s++ )
	seen_out[s] = rec[s].seen;
    return 0;
}
