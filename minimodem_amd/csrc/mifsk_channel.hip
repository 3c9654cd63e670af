// mifsk_channel.hip -- the channelizer (include/mifsk.h): mifsk_channel_plan_create / _destroy,
// mifsk_channelize_batch, the host helpers mifsk_channel_table and mifsk_channel_taps, and
// mifsk_channelize_iq_batch (include/mifsk/channel_iq.h): the same kernel body with the epilogue that
// keeps both halves of the rotated sum.  The plan, the kernel's arguments and the geometry of a launch
// are in mifsk_channel_plan.h, which mifsk_channel_stream.hip (rows fed in pieces) shares.
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
// MFMA: its internal summation is not that chain.  The kernel reads nothing it wrote, so it needs
// no fences; the outputs are plain vector stores.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <type_traits>

#include "mifsk.h"
#include "mifsk/channel_iq.h"
#include "mifsk_channel_plan.h"
#include "mifsk_ctx.h"

namespace mifsk {

// NC: channels per lane.  CX: complex rows.  S16: PCM16 scalars.  IQ: the epilogue of
// mifsk_channelize_iq_batch (include/mifsk/channel_iq.h): rows are [out_stride] (I, Q) pairs, I the
// real entry's output, Q the other half of the same rotation, one 8-byte store for both.  (A fourth
// parameter of this kernel, not a body shared by two kernels: inlined into a wrapper the IQ = false
// code comes out nine instructions longer, and it is to stay as it is.)
template <int NC, bool CX, bool S16, bool IQ>
__global__ __launch_bounds__(256)
void channelize_kernel( const ChannelArgs A )
{
    using OT = std::conditional_t<IQ, float2, float>;
    using XT = std::conditional_t<CX, double2, double>;
    extern __shared__ double2 ch_lds[];
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
    const uint32_t nv = n_row < A.in.stride ? n_row : (uint32_t)A.in.stride;	// elements the row holds
    const char *row = reinterpret_cast<const char *>(A.in.x)
	+ (size_t)s * A.in.stride * ( ( S16 ? 2u : 4u ) * ( CX ? 2u : 1u ) );
    // outputs that exist, of those the rows have room for: output m < cnt reads x[m D + t], t < T,
    // all below nv
    const uint32_t fit = nv >= T ? ( nv - T ) / D + 1u : 0u;
    const uint32_t cnt = fit < A.nout_cap ? fit : A.nout_cap;
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
		    v = channel_sample<CX, S16>(row, at);
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
    // p = (dq * ((m D) mod P)) mod P for m = m0 + ol + o NOG: from o to o + 1 it grows by
    // (dq * ((NOG D) mod P)) mod P
    const uint32_t md0 = (uint32_t)( ( ( m0 + ol ) * D ) % P ), mdstep = (uint32_t)( ( (uint64_t)NOG * D ) % P );
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
}

namespace {

// what both table makers refuse of params
int channel_check_params( const mifsk_channel_params *p )
{
    if ( int rc = phase_check_params(p, MIFSK_CHANNEL_COMPLEX) )
	return rc;
    if ( p->decim == 0 || p->decim > kChMaxD )
	return -EINVAL;
    if ( (uint64_t)p->nchannels * p->ntaps > kChMaxKT )
	return -EINVAL;
    return 0;
}

// channel k's G, tap t at g[t * gstride]: the taps turned back by the channel's centre
void channel_table( const mifsk_channel_params *p, uint32_t k, double2 *g, size_t gstride )
{
    phase_rotated_taps(p->taps, p->ntaps, p->centres[k], p->phase_steps, true, g, gstride);
}

} // namespace
} // namespace mifsk

extern "C" int mifsk_channel_table( const mifsk_channel_params *params, uint32_t k, double *g_out )
{
    if ( int rc = mifsk::channel_check_params(params) )
	return rc;
    if ( k >= params->nchannels || !g_out )
	return -EINVAL;
    static_assert(sizeof(double2) == 2 * sizeof(double), "G is [ntaps][2] doubles");
    mifsk::channel_table(params, k, reinterpret_cast<double2 *>(g_out), 1);
    return 0;
}

extern "C" int mifsk_channel_taps( uint32_t ntaps, double cutoff_hz, double sample_rate, double gain, float *out )
{
    if ( ntaps == 0 || ntaps > mifsk::kPhaseMaxTaps || !out )
	return -EINVAL;
    if ( !( cutoff_hz > 0.0 ) || !( sample_rate > 0.0 ) || !std::isfinite(cutoff_hz) || !std::isfinite(sample_rate) )
	return -EINVAL;
    if ( ntaps == 1 ) {
	out[0] = (float)gain;
	return 0;
    }
    double h[mifsk::kPhaseMaxTaps];
    const double f = 2.0 * cutoff_hz / sample_rate, mid = (double)( ntaps - 1u ) / 2.0;
    double sum = 0.0;
    for ( uint32_t t = 0; t < ntaps; t++ ) {
	const double a = M_PI * ( f * ( (double)t - mid ) );
	const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
	h[t] = f * sinc * ( 0.54 - 0.46 * cos(mifsk::kTwoPi * (double)t / (double)( ntaps - 1u )) );
	sum += h[t];
    }
    for ( uint32_t t = 0; t < ntaps; t++ )
	out[t] = (float)( h[t] * ( gain / sum ) );
    return 0;
}

extern "C" int mifsk_channel_plan_create( mifsk_ctx *ctx, const mifsk_channel_params *params, mifsk_channel_plan **out )
{
    using namespace mifsk;
    if ( !ctx || !params || !out )
	return -EINVAL;
    if ( int rc = channel_check_params(params) )
	return rc;
    const uint32_t T = params->ntaps, K = params->nchannels;
    const size_t ngt = (size_t)T * K;
    const auto gt = host_array<double2>(ngt);
    const auto dq = host_array<uint32_t>(K);
    std::unique_ptr<mifsk_channel_plan> plan(new (std::nothrow) mifsk_channel_plan);
    if ( !gt || !dq || !plan )
	return -ENOMEM;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_table(params, k, gt.get() + k, K);
	dq[k] = phase_diff(params->out_centre, params->centres[k], params->phase_steps);
    }
    plan->D = params->decim;
    int rc = phase_plan_init(*plan, ctx->device, params, ( params->flags & MIFSK_CHANNEL_COMPLEX ) != 0, dq.get());
    if ( rc == 0 )
	rc = upload(plan->gt, gt.get(), ngt);
    if ( rc )
	return rc;
    *out = plan.release();
    return 0;
}

extern "C" void mifsk_channel_plan_destroy( mifsk_channel_plan *plan ) { mifsk::phase_plan_destroy(plan); }

// Both batch entries: their checks, then the one launch path.  An output element is a float, or with
// `iq` an (I, Q) pair: out_vec of them are 16 bytes, a row is out_max of them at most.
static int channelize_rows( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream, bool iq )
{
    using namespace mifsk;
    if ( !plan || !io )
	return -EINVAL;
    const uint32_t out_vec = iq ? 2u : 4u;
    const uint64_t out_max = iq ? 0x7FFFFFFEull : 0xFFFFFFFCull;
    if ( int rc = phase_check_io(*plan, io, io->d_rows, rows_vec(plan->cx, plan->s16), out_vec, out_max) )
	return rc;

    const ChannelGeometry g = channel_geometry(*plan);
    ChannelArgs A = channel_args(*plan, io, g);

    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    const uint32_t nchunks = (uint32_t)( ( io->out_stride + g.OB - 1u ) / g.OB );
    const uint32_t gz = ( plan->K + g.C - 1u ) / g.C;
    const hipStream_t st = (hipStream_t)stream;
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	const dim3 grid(nchunks, rows, gz), block(64u * kChWaves);
	auto launch = [&]( auto per_lane ) {
	    return dispatch_kind(plan->cx, plan->s16, [&]( auto cx, auto s16 ) {
		constexpr int NC = decltype(per_lane)::value;
		constexpr bool CX = decltype(cx)::value, S16 = decltype(s16)::value;
		return launch_lds(iq ? channelize_kernel<NC, CX, S16, true> : channelize_kernel<NC, CX, S16, false>,
				  grid, block, g.lds, st, A);
	    });
	};
	return g.nc == 2u ? launch(std::integral_constant<int, 2>{}) : launch(std::integral_constant<int, 1>{});
    });
}

extern "C" int mifsk_channelize_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream )
{
    return channelize_rows(plan, io, stream, false);
}

extern "C" int mifsk_channelize_iq_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream )
{
    return channelize_rows(plan, io, stream, true);
}
