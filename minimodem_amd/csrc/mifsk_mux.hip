// mifsk_mux.hip -- the multiplexer (include/mifsk.h): mifsk_mux_plan_create / _destroy,
// mifsk_multiplex_batch, and the host helper mifsk_mux_table; mifsk_multiplex_iq_batch
// (include/mifsk/mux_iq.h): the same kernel with I/Q rows in (IQIN, at the kernel).
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
// Blocks beyond the stream's outputs store zeros only; block 0 stores the count.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk/mux_iq.h"
#include "mifsk_ctx.h"
#include "mifsk_phase.h"
#include "mifsk_rows.h"

namespace mifsk {

constexpr int kMxO = 8;					// outputs per lane
constexpr uint32_t kMxThreads = 256u;
constexpr uint32_t kMxLdsSamples = 48u * 1024u;		// table + samples: stage channels up to here (3 workgroups per CU)
constexpr uint32_t kMxMaxL = 65535u;

struct MuxArgs {
    const double2	*g;		// [T]
    const double2	*w;		// [P]: cos, sin
    const uint32_t	*dq;		// [K]: (q[k] - r) mod P
    const uint32_t	*ps;		// [K]: (dq[k] * (L mod P)) mod P
    const float		*gains;		// [K] or NULL
    RowsIn		in;		// floats; IQIN: (I, Q) pairs of floats
    uint32_t		T, L, K, P;
    uint32_t		jmax;		// ceil(T / L): tap steps of phase 0
    uint32_t		span;		// samples staged per channel, at most
    uint32_t		spanp;		// ... and doubles between the channels' spans (padded)
    uint32_t		cb;		// channels staged at a time
    uint32_t		s0;		// first stream of this launch
    void		*out;
    size_t		out_stride;	// elements
    uint32_t		nout_cap;
    uint32_t		*nout;
};

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
// kernels (mifsk_channel.hip says why): what the IQIN = false instantiations execute is the text it was.
template <bool CX, bool S16, bool IQIN>
__global__ __launch_bounds__(256)
void multiplex_kernel( const MuxArgs A )
{
    extern __shared__ double2 mx_lds[];
    __shared__ uint32_t nmax_sh;
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
    const uint32_t nmax = nmax_sh;
    const uint64_t total = nmax ? (uint64_t)( nmax - 1u ) * L + T : 0ull;
    const uint32_t cnt = total < A.nout_cap ? (uint32_t)total : A.nout_cap;
    if ( blockIdx.x == 0u && tid == 0u )
	A.nout[s] = cnt;

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
	const uint32_t nm0 = (uint32_t)( n0 % P );
	for ( uint32_t k0 = 0; k0 < K; k0 += A.cb ) {
	    const uint32_t cbn = K - k0 < A.cb ? K - k0 : A.cb;
	    __syncthreads();					// the spans before have been read
	    // a wave per channel: the row and its length are the wave's, the lanes read along the row
	    for ( uint32_t c = tid >> 6; c < cbn; c += kMxThreads / 64u ) {
		const int64_t nk = row_len(k0 + c);
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
		const int64_t nk = row_len(k);
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
		    if ( lo >= 0 && hi < nk ) {
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
				if ( i >= 0 && i < nk ) {
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
		if ( lo >= 0 && hi < nk ) {
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
			    if ( i >= 0 && i < nk ) {
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

namespace {

// what both table makers refuse of params
int mux_check_params( const mifsk_mux_params *p )
{
    if ( int rc = phase_check_params(p, MIFSK_MUX_COMPLEX) )
	return rc;
    if ( p->interp == 0 || p->interp > kMxMaxL )
	return -EINVAL;
    return phase_centre_ok(p->in_centre, p->phase_steps) ? 0 : -EINVAL;
}

// G: the taps turned forward by the rows' centre
void mux_table( const mifsk_mux_params *p, double2 *g )
{
    phase_rotated_taps(p->taps, p->ntaps, p->in_centre, p->phase_steps, false, g, 1);
}

} // namespace
} // namespace mifsk

struct mifsk_mux_plan : mifsk::PhasePlanCommon {
    uint32_t			L;
    mifsk::DevMem<double2>	g;
    mifsk::DevMem<uint32_t>	ps;
    mifsk::DevMem<float>	gains;		// empty: no gain step
};

extern "C" int mifsk_mux_table( const mifsk_mux_params *params, double *g_out )
{
    if ( int rc = mifsk::mux_check_params(params) )
	return rc;
    if ( !g_out )
	return -EINVAL;
    static_assert(sizeof(double2) == 2 * sizeof(double), "G is [ntaps][2] doubles");
    mifsk::mux_table(params, reinterpret_cast<double2 *>(g_out));
    return 0;
}

extern "C" int mifsk_mux_plan_create( mifsk_ctx *ctx, const mifsk_mux_params *params, mifsk_mux_plan **out )
{
    using namespace mifsk;
    if ( !ctx || !params || !out )
	return -EINVAL;
    if ( int rc = mux_check_params(params) )
	return rc;
    const uint32_t P = params->phase_steps, T = params->ntaps, K = params->nchannels, L = params->interp;
    const auto g = host_array<double2>(T);
    const auto dq = host_array<uint32_t>(K), ps = host_array<uint32_t>(K);
    std::unique_ptr<mifsk_mux_plan> plan(new (std::nothrow) mifsk_mux_plan);
    if ( !g || !dq || !ps || !plan )
	return -ENOMEM;
    mux_table(params, g.get());
    for ( uint32_t k = 0; k < K; k++ ) {
	dq[k] = phase_diff(params->centres[k], params->in_centre, P);
	ps[k] = (uint32_t)( ( (uint64_t)dq[k] * ( L % P ) ) % P );
    }
    plan->L = L;
    int rc = phase_plan_init(*plan, ctx->device, params, ( params->flags & MIFSK_MUX_COMPLEX ) != 0, dq.get());
    if ( rc == 0 ) rc = upload(plan->g, g.get(), T);
    if ( rc == 0 ) rc = upload(plan->ps, ps.get(), K);
    if ( rc == 0 && params->gains ) rc = upload(plan->gains, params->gains, K);
    if ( rc )
	return rc;
    *out = plan.release();
    return 0;
}

extern "C" void mifsk_mux_plan_destroy( mifsk_mux_plan *plan ) { mifsk::phase_plan_destroy(plan); }

// Both entries.  `iq`: the input rows are (I, Q) pairs of floats, 2 of them 16 bytes, and the kernel is
// the IQIN one; everything else is a function of the plan and the io alone.
static int multiplex_rows( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream, bool iq )
{
    using namespace mifsk;
    if ( !plan || !io )
	return -EINVAL;
    if ( int rc = phase_check_io(*plan, io, io->d_out, iq ? 2u : 4u, rows_vec(plan->cx, plan->s16), 0xFFFFFFF8ull) )
	return rc;

    MuxArgs A = {};
    A.g = plan->g.p;
    A.w = plan->w.p;
    A.dq = plan->dq.p;
    A.ps = plan->ps.p;
    A.gains = plan->gains.p;
    A.in = rows_in(io);
    A.T = plan->T;
    A.L = plan->L;
    A.K = plan->K;
    A.P = plan->P;
    A.out = io->d_out;
    A.out_stride = io->out_stride;
    A.nout_cap = io->nout_cap;
    A.nout = io->d_nout;

    // a block's 256 slots touch at most 255 / L + 2 groups of 8 values of m, and jmax - 1 samples
    // before the first; as many channels' spans at a time as fit beside the table, one at least
    A.jmax = ( plan->T + plan->L - 1u ) / plan->L;
    A.span = (uint32_t)kMxO * ( ( kMxThreads - 1u ) / plan->L + 2u ) + A.jmax - 1u;
    A.spanp = A.span + ( A.span >> 3 ) + 1u;
    const size_t table = (size_t)plan->T * sizeof(double2), one = (size_t)A.spanp * sizeof(double);
    A.cb = table + one < kMxLdsSamples ? (uint32_t)( ( kMxLdsSamples - table ) / one ) : 1u;
    if ( A.cb > plan->K )
	A.cb = plan->K;
    const size_t lds = table + (size_t)A.cb * one;

    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    // slots: L per group of 8 L outputs
    const uint64_t ngroups = ( io->out_stride + (uint64_t)kMxO * plan->L - 1u ) / ( (uint64_t)kMxO * plan->L );
    const uint32_t nblocks = (uint32_t)( ( ngroups * plan->L + kMxThreads - 1u ) / kMxThreads );
    const hipStream_t st = (hipStream_t)stream;
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	return dispatch_kind(plan->cx, plan->s16, [&]( auto cx, auto s16 ) {
	    constexpr bool CX = decltype(cx)::value, S16 = decltype(s16)::value;
	    return launch_lds(iq ? multiplex_kernel<CX, S16, true> : multiplex_kernel<CX, S16, false>, dim3(nblocks, rows, 1),
			      dim3(kMxThreads), lds, st, A);
	});
    });
}

extern "C" int mifsk_multiplex_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream )
{
    return multiplex_rows(plan, io, stream, false);
}

extern "C" int mifsk_multiplex_iq_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream )
{
    return multiplex_rows(plan, io, stream, true);
}
