// mifsk_fm.hip -- the FM stage (include/mifsk.h): mifsk_fm_demod_batch, mifsk_fm_modulate_batch and
// the host helpers mifsk_fm_gain, mifsk_fm_step.
//
// The discriminator: out[n] = gain * turn(z[n] conj z[n - 1]) (mifsk_angle.h), a pure function of two
// neighbouring samples, so the kernel carries no state:
//   * a thread owns four consecutive outputs (one 16-byte store): it loads its four complex samples
//     as whole 16-byte vectors (two of float32, one of PCM16) and the one sample before them.  Lanes
//     of a wave are consecutive along a row.
//   * grid x runs over a row's vectors up to out_stride, y over the rows (blocks of 65 535 rows,
//     mifsk_batch.h); the same launch writes the rows' tails as zero: a thread wholly behind the
//     row's length stores zeros without a load.
//   * the thread that owns the row's last valid sample stores it to d_last.
// The modulator: the phase is a 64-bit INTEGER sum of per-sample steps, so its value does not depend
// on the order of the additions and a parallel scan equals the serial loop.  Three launches:
//   1. fm_tile_sums_kernel: a workgroup sums the steps of its tile (256 threads x 8 samples) into
//      scratch [row][tile];
//   2. fm_row_scan_kernel: one wave per row turns the row's sums into the phase before each tile
//      (phase0 included), in place, and stores the row's last phase;
//   3. fm_tile_write_kernel: a workgroup recomputes its tile's steps, scans them (thread-serial, then
//      across the wave, then across the waves through LDS), and stores I, Q.
// No workgroup waits for another inside a kernel: the order is the stream's.  Nothing a kernel
// wrote is read back by the same kernel; the outputs are plain vector stores.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>

#include "mifsk.h"
#include "mifsk_angle.h"
#include "mifsk_batch.h"
#include "mifsk_ctx.h"
#include "mifsk_gauss.h"
#include "mifsk_hostmem.h"
#include "mifsk_rows.h"

namespace mifsk {

constexpr uint32_t kFmThreads = 256u;
constexpr uint32_t kFmPer = 8u;					// the modulator's samples per thread
constexpr uint32_t kFmTile = kFmThreads * kFmPer;		// ... and per workgroup

// ---------------------------------------------------------------------------
// the discriminator
// ---------------------------------------------------------------------------
struct FmDemodArgs {
    RowsIn		in;		// interleaved I, Q: complex elements
    uint32_t		s0;		// first row of this launch
    float		*out;
    size_t		out_stride;
    const float2	*prev;		// [nstreams] or NULL
    float2		*last;		// [nstreams] or NULL
    float		gain;
};

template <bool S16>
__global__ __launch_bounds__(256)
void fm_demod_kernel( const FmDemodArgs A )
{
    const uint32_t s = A.s0 + blockIdx.y;
    const uint64_t i0 = (uint64_t)( blockIdx.x * kFmThreads + threadIdx.x ) * 4u;
    if ( i0 >= A.out_stride )
	return;
    // (RowsIn::len(s, true, A.out_stride), written out: through the member the compiler orders this
    // kernel's argument loads differently, and its code is to stay as it is)
    uint64_t W = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    if ( W > A.in.stride )
	W = A.in.stride;
    if ( W > A.out_stride )
	W = A.out_stride;

    float o[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float2 before = float2{0.0f, 0.0f};				// the sample before the thread's four
    if ( i0 == 0u && A.prev )
	before = A.prev[s];
    if ( i0 < W ) {
	// the samples: whole 16-byte vectors that begin inside the row's length, and with it inside
	// its stride (a multiple of the vector)
	float zr[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, zi[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
	if constexpr ( S16 ) {
	    const int16_t *row = reinterpret_cast<const int16_t *>(A.in.x) + ( (size_t)s * A.in.stride + i0 ) * 2u;
	    const S16x8 p = *reinterpret_cast<const S16x8 *>(row);
#pragma unroll
	    for ( uint32_t u = 0; u < 4u; u++ ) {
		zr[u] = rows_f32(p.v[2u * u]);
		zi[u] = rows_f32(p.v[2u * u + 1u]);
	    }
	    if ( i0 > 0u ) {
		const short2 b = *reinterpret_cast<const short2 *>(row - 2);
		before = float2{rows_f32(b.x), rows_f32(b.y)};
	    }
	} else {
	    const float *row = reinterpret_cast<const float *>(A.in.x) + ( (size_t)s * A.in.stride + i0 ) * 2u;
#pragma unroll
	    for ( uint32_t h = 0; h < 2u; h++ ) {
		if ( i0 + 2u * h < W ) {
		    const float4 p = *reinterpret_cast<const float4 *>(row + 4u * h);
		    zr[2u * h] = p.x;
		    zi[2u * h] = p.y;
		    zr[2u * h + 1u] = p.z;
		    zi[2u * h + 1u] = p.w;
		}
	    }
	    if ( i0 > 0u )
		before = *reinterpret_cast<const float2 *>(row - 2);
	}
	const double g = (double)A.gain;
	double c = (double)before.x, d = (double)before.y;
#pragma unroll
	for ( uint32_t u = 0; u < 4u; u++ ) {
	    const double a = (double)zr[u], b = (double)zi[u];
	    const double re = fma(a, c, b * d);
	    const double im = fma(b, c, -( a * d ));
	    o[u] = i0 + u < W ? (float)( g * mifsk_turn(im, re) ) : 0.0f;
	    c = a;
	    d = b;
	}
	if ( A.last && W - i0 <= 4u ) {				// the row's last valid sample is this thread's
	    const uint32_t u = (uint32_t)( W - i0 ) - 1u;
	    A.last[s] = float2{zr[u], zi[u]};
	}
    } else if ( A.last && W == 0u && i0 == 0u ) {
	A.last[s] = before;
    }
    *reinterpret_cast<float4 *>(A.out + (size_t)s * A.out_stride + i0) = float4{o[0], o[1], o[2], o[3]};
}

// ---------------------------------------------------------------------------
// the modulator
// ---------------------------------------------------------------------------
struct FmModArgs {
    RowsIn		in;		// floats
    uint32_t		s0;		// first row of this launch
    uint32_t		nrows;		// all rows (the row scan)
    uint32_t		ntiles;		// tiles of a row: up to out_stride
    void		*out;
    size_t		out_stride;	// complex elements
    double		deviation, centre, amplitude;
    const uint64_t	*phase0;	// [nstreams] or NULL
    uint64_t		*phase_out;	// [nstreams] or NULL
    uint64_t		*tiles;		// scratch [nstreams][ntiles]: sums, then the phase before each tile
};

// the phase step of one sample
__device__ __forceinline__ uint64_t fm_step( float x, double deviation, double centre )
{
    const double d = fma((double)x, deviation, centre);
    return fabs(d) < 16384.0 ? (uint64_t)(long long)rint(d * 0x1p48) : 0ull;
}

// q[0 .. 8): the steps of the thread's samples i0 .. i0 + 7 of row s, zero from W on
__device__ __forceinline__ void fm_steps( const FmModArgs &A, uint32_t s, uint64_t i0, uint64_t W, uint64_t q[kFmPer] )
{
    const float *row = reinterpret_cast<const float *>(A.in.x) + (size_t)s * A.in.stride + i0;
#pragma unroll
    for ( uint32_t h = 0; h < kFmPer; h += 4u ) {
	float4 p = float4{0.0f, 0.0f, 0.0f, 0.0f};
	if ( i0 + h < W )					// a whole vector inside the row's stride
	    p = *reinterpret_cast<const float4 *>(row + h);
	const float x[4] = { p.x, p.y, p.z, p.w };
#pragma unroll
	for ( uint32_t u = 0; u < 4u; u++ )
	    q[h + u] = i0 + h + u < W ? fm_step(x[u], A.deviation, A.centre) : 0ull;
    }
}

// the sum over the lanes below this one, and (total) over all 64
__device__ __forceinline__ uint64_t fm_wave_exclusive( uint64_t v, uint32_t lane, uint64_t &total )
{
    uint64_t inc = v;
#pragma unroll
    for ( uint32_t d = 1u; d < 64u; d <<= 1 ) {
	const uint64_t up = (uint64_t)__shfl_up((unsigned long long)inc, d, 64);
	if ( lane >= d )
	    inc += up;
    }
    total = (uint64_t)__shfl((unsigned long long)inc, 63, 64);
    return inc - v;
}

__global__ __launch_bounds__(256)
void fm_tile_sums_kernel( const FmModArgs A )
{
    __shared__ uint64_t wave_sum[kFmThreads / 64u];
    const uint32_t s = A.s0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const uint64_t t0 = (uint64_t)blockIdx.x * kFmTile, W = A.in.len(s, true, A.out_stride);
    uint64_t mine = 0ull;
    if ( t0 < W ) {						// (the whole workgroup)
	uint64_t q[kFmPer];
	fm_steps(A, s, t0 + (uint64_t)tid * kFmPer, W, q);
#pragma unroll
	for ( uint32_t u = 0; u < kFmPer; u++ )
	    mine += q[u];
    }
    uint64_t total;
    (void)fm_wave_exclusive(mine, lane, total);
    if ( lane == 0u )
	wave_sum[tid >> 6] = total;
    __syncthreads();
    if ( tid == 0u )
	A.tiles[(size_t)s * A.ntiles + blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// one wave per row: tiles[row][t] = phase0 + the sums of the tiles before t; phase_out = ... of all
__global__ __launch_bounds__(256)
void fm_row_scan_kernel( const FmModArgs A )
{
    const uint32_t s = blockIdx.x * ( kFmThreads / 64u ) + ( threadIdx.x >> 6 ), lane = threadIdx.x & 63u;
    if ( s >= A.nrows )
	return;							// (whole waves)
    uint64_t carry = A.phase0 ? A.phase0[s] : 0ull;
    uint64_t *t = A.tiles + (size_t)s * A.ntiles;
    for ( uint32_t k0 = 0; k0 < A.ntiles; k0 += 64u ) {
	const uint32_t k = k0 + lane;
	const uint64_t v = k < A.ntiles ? t[k] : 0ull;
	uint64_t total;
	const uint64_t before = fm_wave_exclusive(v, lane, total);
	if ( k < A.ntiles )
	    t[k] = carry + before;
	carry += total;
    }
    if ( A.phase_out && lane == 0u )
	A.phase_out[s] = carry;
}

template <bool S16>
__global__ __launch_bounds__(256)
void fm_tile_write_kernel( const FmModArgs A )
{
    __shared__ uint64_t wave_sum[kFmThreads / 64u];
    const uint32_t s = A.s0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kFmTile, i0 = t0 + (uint64_t)tid * kFmPer, W = A.in.len(s, true, A.out_stride);
    float oi[kFmPer], oq[kFmPer];
#pragma unroll
    for ( uint32_t u = 0; u < kFmPer; u++ ) {
	oi[u] = 0.0f;
	oq[u] = 0.0f;
    }
    if ( t0 < W ) {						// (the whole workgroup)
	uint64_t q[kFmPer];
	fm_steps(A, s, i0, W, q);
#pragma unroll
	for ( uint32_t u = 1; u < kFmPer; u++ )
	    q[u] += q[u - 1u];					// inclusive, inside the thread
	uint64_t total;
	uint64_t before = fm_wave_exclusive(q[kFmPer - 1u], lane, total);
	if ( lane == 0u )
	    wave_sum[wave] = total;
	__syncthreads();
	for ( uint32_t w = 0; w < wave; w++ )
	    before += wave_sum[w];
	before += A.tiles[(size_t)s * A.ntiles + blockIdx.x];
#pragma unroll
	for ( uint32_t u = 0; u < kFmPer; u++ ) {
	    if ( i0 + u < W ) {
		const uint64_t phase = before + q[u];
		double c, sn;
		mifsk_gauss_cs((uint32_t)( phase >> 16 ), &c, &sn);
		oi[u] = (float)( A.amplitude * c );
		oq[u] = (float)( A.amplitude * sn );
	    }
	}
    }
    // whole 16-byte vectors that begin inside out_stride (a multiple of the vector)
    if constexpr ( S16 ) {
	int16_t *row = reinterpret_cast<int16_t *>(A.out) + ( (size_t)s * A.out_stride + i0 ) * 2u;
#pragma unroll
	for ( uint32_t h = 0; h < kFmPer; h += 4u ) {
	    if ( i0 + h < A.out_stride ) {
		S16x8 p;
#pragma unroll
		for ( uint32_t u = 0; u < 4u; u++ ) {
		    p.v[2u * u] = i0 + h + u < W ? rows_s16(oi[h + u]) : (int16_t)0;
		    p.v[2u * u + 1u] = i0 + h + u < W ? rows_s16(oq[h + u]) : (int16_t)0;
		}
		*reinterpret_cast<S16x8 *>(row + 2u * h) = p;
	    }
	}
    } else {
	float *row = reinterpret_cast<float *>(A.out) + ( (size_t)s * A.out_stride + i0 ) * 2u;
#pragma unroll
	for ( uint32_t h = 0; h < kFmPer; h += 2u )
	    if ( i0 + h < A.out_stride )
		*reinterpret_cast<float4 *>(row + 2u * h) = float4{oi[h], oq[h], oi[h + 1u], oq[h + 1u]};
    }
}

} // namespace mifsk

extern "C" float mifsk_fm_gain( double sample_rate, double deviation_hz ) { return (float)( sample_rate / deviation_hz ); }

extern "C" double mifsk_fm_step( double deviation_hz, double sample_rate ) { return deviation_hz / sample_rate; }

extern "C" int mifsk_fm_demod_batch( mifsk_ctx *ctx, const mifsk_fm_demod_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !io || !io->d_samples || !io->d_out )
	return -EINVAL;
    if ( io->nstreams <= 0 )
	return -EINVAL;
    if ( int rc = kind_check(io->kind) )
	return rc;
    if ( io->flags != 0u )
	return -EINVAL;
    const bool s16 = io->kind == MIFSK_FEED_S16;
    if ( !rows_aligned(io->d_samples, io->stream_stride, rows_vec(true, s16)) )
	return -EINVAL;
    if ( int rc = out_rows_check(io->d_out, io->out_stride, 4u, 0xFFFFFFF8ull) )
	return rc;

    FmDemodArgs A = {};
    A.in = rows_in(io);
    A.out = io->d_out;
    A.out_stride = io->out_stride;
    A.prev = reinterpret_cast<const float2 *>(io->d_prev);
    A.last = reinterpret_cast<float2 *>(io->d_last);
    A.gain = io->gain;

    if ( hipSetDevice(ctx->device) != hipSuccess )
	return -EIO;
    const uint64_t nvec = io->out_stride / 4u;
    const uint32_t nblocks = (uint32_t)( ( nvec + kFmThreads - 1u ) / kFmThreads );
    const hipStream_t st = (hipStream_t)stream;
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	return dispatch_kind(true, s16, [&]( auto, auto in16 ) {
	    hipLaunchKernelGGL(( fm_demod_kernel<decltype(in16)::value> ), dim3(nblocks, rows, 1), dim3(kFmThreads), 0, st, A);
	    return 0;
	});
    });
}

extern "C" int mifsk_fm_modulate_batch( mifsk_ctx *ctx, const mifsk_fm_mod_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !io || !io->d_samples || !io->d_out )
	return -EINVAL;
    if ( io->nstreams <= 0 )
	return -EINVAL;
    if ( int rc = kind_check(io->out_kind) )
	return rc;
    if ( io->flags != 0u )
	return -EINVAL;
    const bool s16 = io->out_kind == MIFSK_FEED_S16;
    if ( !rows_aligned(io->d_samples, io->stream_stride, rows_vec(false, false)) )
	return -EINVAL;
    if ( int rc = out_rows_check(io->d_out, io->out_stride, rows_vec(true, s16), 0xFFFFFFF8ull) )
	return rc;

    FmModArgs A = {};
    A.in = rows_in(io);
    A.nrows = (uint32_t)io->nstreams;
    A.ntiles = (uint32_t)( ( io->out_stride + kFmTile - 1u ) / kFmTile );
    A.out = io->d_out;
    A.out_stride = io->out_stride;
    A.deviation = io->deviation;
    A.centre = io->centre;
    A.amplitude = (double)io->amplitude;
    A.phase0 = io->d_phase0;
    A.phase_out = io->d_phase_out;

    if ( hipSetDevice(ctx->device) != hipSuccess )
	return -EIO;
    const hipStream_t st = (hipStream_t)stream;
    StreamMem scratch(st);					// freed in the stream's order, behind the launches
    if ( int rc = scratch.alloc((size_t)A.nrows * A.ntiles * sizeof(uint64_t)) )
	return rc;
    A.tiles = reinterpret_cast<uint64_t *>(scratch.p);
    if ( int rc = for_row_blocks(A.nrows, [&]( uint32_t s0, uint32_t rows ) {
	    A.s0 = s0;
	    hipLaunchKernelGGL(fm_tile_sums_kernel, dim3(A.ntiles, rows, 1), dim3(kFmThreads), 0, st, A);
	    return 0;
	}) )
	return rc;
    A.s0 = 0u;
    hipLaunchKernelGGL(fm_row_scan_kernel, dim3(( A.nrows + kFmThreads / 64u - 1u ) / ( kFmThreads / 64u )), dim3(kFmThreads), 0,
		       st, A);
    return for_row_blocks(A.nrows, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	return dispatch_kind(true, s16, [&]( auto, auto out16 ) {
	    hipLaunchKernelGGL(( fm_tile_write_kernel<decltype(out16)::value> ), dim3(A.ntiles, rows, 1), dim3(kFmThreads), 0,
			       st, A);
	    return 0;
	});
    });
}
