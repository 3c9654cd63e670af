// mifsk_impair.hip -- the channel model (include/mifsk.h): mifsk_impair_batch and the host helper
// mifsk_impair_sigma.
//
// out = gain x + dc + sigma z, z the noise field of mifsk_gauss.h: a pure function of (seed, stream
// index, sample index), so the kernel carries no state and every thread makes its own normals.
//   * a thread owns one 16-byte vector of the narrower side: 4 samples when both sides are float32
//     (one Philox block, one 16-byte load, one 16-byte store), 8 samples when a side is PCM16 (two
//     blocks; the float32 side is then two 16-byte accesses).  Lanes of a wave are consecutive
//     vectors of one row.
//   * grid x runs over a row's vectors up to out_stride, y over the rows (blocks of 65 535 rows,
//     mifsk_batch.h); the same launch writes the rows' tails as zero: a vector wholly behind the
//     row's length stores zeros without a load or a normal.
//   * gain, sigma and dc are the block's (one row): scalar loads.
// Everything stays in vector registers: no LDS, no atomics; the kernel reads nothing it wrote (in
// place a thread reads its own vector before it stores it, and no other thread touches it), so it
// needs no fences; the outputs are plain vector stores.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>

#include "mifsk.h"
#include "mifsk_batch.h"
#include "mifsk_ctx.h"
#include "mifsk_gauss.h"
#include "mifsk_rows.h"

namespace mifsk {

constexpr uint32_t kImThreads = 256u;

struct ImpairArgs {
    RowsIn		in;		// x NULL: x = 0
    uint32_t		s0;		// first row of this launch
    void		*out;
    size_t		out_stride;	// elements
    uint64_t		seed, first_stream, first_sample;
    const float		*gain_v, *sigma_v, *dc_v;
    float		gain, sigma, dc;
};

// IN_S16 / OUT_S16: PCM16 scalars on that side
template <bool IN_S16, bool OUT_S16>
__global__ __launch_bounds__(256)
void impair_kernel( const ImpairArgs A )
{
    constexpr uint32_t V = ( IN_S16 || OUT_S16 ) ? 8u : 4u;	// samples of a thread
    const uint32_t s = A.s0 + blockIdx.y;
    const uint64_t i0 = (uint64_t)( blockIdx.x * kImThreads + threadIdx.x ) * V;
    if ( i0 >= A.out_stride )
	return;
    // (RowsIn::len(s, A.in.x, A.out_stride), written out: through the member the compiler orders this
    // kernel's argument loads differently, and its code is to stay as it is)
    uint64_t W = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    if ( A.in.x && W > A.in.stride )
	W = A.in.stride;
    if ( W > A.out_stride )
	W = A.out_stride;

    float o[V];
#pragma unroll
    for ( uint32_t u = 0; u < V; u++ )
	o[u] = 0.0f;
    if ( i0 < W ) {
	// the samples: whole 16-byte vectors that begin inside the row's length, and with it inside
	// its stride (a multiple of the vector)
	float x[V];
#pragma unroll
	for ( uint32_t u = 0; u < V; u++ )
	    x[u] = 0.0f;
	if ( A.in.x ) {
	    if constexpr ( IN_S16 ) {
		const S16x8 p = *reinterpret_cast<const S16x8 *>(
			reinterpret_cast<const int16_t *>(A.in.x) + (size_t)s * A.in.stride + i0);
#pragma unroll
		for ( uint32_t u = 0; u < 8u; u++ )
		    x[u] = rows_f32(p.v[u]);
	    } else {
		const float *row = reinterpret_cast<const float *>(A.in.x) + (size_t)s * A.in.stride + i0;
#pragma unroll
		for ( uint32_t h = 0; h < V; h += 4u ) {
		    if ( i0 + h < W ) {
			const float4 p = *reinterpret_cast<const float4 *>(row + h);
			x[h] = p.x;
			x[h + 1u] = p.y;
			x[h + 2u] = p.z;
			x[h + 3u] = p.w;
		    }
		}
	    }
	}
	const double g = (double)( A.gain_v ? A.gain_v[s] : A.gain ), sg = (double)( A.sigma_v ? A.sigma_v[s] : A.sigma ),
		     d = (double)( A.dc_v ? A.dc_v[s] : A.dc );
	const uint64_t S = A.first_stream + s, n0 = A.first_sample + i0;
#pragma unroll
	for ( uint32_t h = 0; h < V; h += 4u ) {
	    double z[4];
	    mifsk_gauss_block(A.seed, S, ( n0 + h ) >> 2, z);
#pragma unroll
	    for ( uint32_t u = 0; u < 4u; u++ ) {
		double v = fma(g, (double)x[h + u], d);
		v = fma(sg, z[u], v);
		o[h + u] = i0 + h + u < W ? (float)v : 0.0f;
	    }
	}
    }
    if constexpr ( OUT_S16 ) {
	// (out_stride is whole vectors of 8: the thread's vector lies inside the row)
	S16x8 p;
#pragma unroll
	for ( uint32_t u = 0; u < 8u; u++ )
	    p.v[u] = i0 + u < W ? rows_s16(o[u]) : (int16_t)0;
	*reinterpret_cast<S16x8 *>(reinterpret_cast<int16_t *>(A.out) + (size_t)s * A.out_stride + i0) = p;
    } else {
	float *row = reinterpret_cast<float *>(A.out) + (size_t)s * A.out_stride + i0;
#pragma unroll
	for ( uint32_t h = 0; h < V; h += 4u )
	    if ( i0 + h < A.out_stride )			// (out_stride is whole vectors of 4)
		*reinterpret_cast<float4 *>(row + h) = float4{o[h], o[h + 1u], o[h + 2u], o[h + 3u]};
    }
}

} // namespace mifsk

extern "C" float mifsk_impair_sigma( float amplitude, double snr_db )
{
    const double a = (double)amplitude;
    return (float)std::sqrt(( a * a / 2.0 ) / std::pow(10.0, snr_db / 10.0));
}

extern "C" int mifsk_impair_batch( mifsk_ctx *ctx, const mifsk_impair_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !io || !io->d_out )
	return -EINVAL;
    if ( io->nstreams <= 0 )
	return -EINVAL;
    if ( kind_check(io->kind) || kind_check(io->out_kind) )
	return -EINVAL;
    if ( io->flags != 0u )
	return -EINVAL;
    if ( io->first_sample % 4u != 0u )
	return -EINVAL;
    const bool in_s16 = io->kind == MIFSK_FEED_S16, out_s16 = io->out_kind == MIFSK_FEED_S16;
    if ( io->d_samples )
	if ( int rc = feed_rows_check(io->kind, 0.0f, io->d_samples, io->stream_stride) )
	    return rc;
    if ( int rc = out_rows_check(io->d_out, io->out_stride, rows_vec(false, out_s16), 0xFFFFFFF8ull) )
	return rc;

    ImpairArgs A = {};
    A.in = rows_in(io);
    A.out = io->d_out;
    A.out_stride = io->out_stride;
    A.seed = io->seed;
    A.first_stream = io->first_stream;
    A.first_sample = io->first_sample;
    A.gain_v = io->d_gain;
    A.sigma_v = io->d_sigma;
    A.dc_v = io->d_dc;
    A.gain = io->gain;
    A.sigma = io->sigma;
    A.dc = io->dc;

    if ( hipSetDevice(ctx->device) != hipSuccess )
	return -EIO;
    const uint32_t per_thread = ( in_s16 || out_s16 ) ? 8u : 4u;
    const uint64_t nvec = ( io->out_stride + per_thread - 1u ) / per_thread;
    const uint32_t nblocks = (uint32_t)( ( nvec + kImThreads - 1u ) / kImThreads );
    const hipStream_t st = (hipStream_t)stream;
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	return dispatch_kind(in_s16, out_s16, [&]( auto in16, auto out16 ) {
	    hipLaunchKernelGGL(( impair_kernel<decltype(in16)::value, decltype(out16)::value> ), dim3(nblocks, rows, 1),
			       dim3(kImThreads), 0, st, A);
	    return 0;
	});
    });
}
