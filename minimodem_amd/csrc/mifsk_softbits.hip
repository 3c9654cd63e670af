// mifsk_softbits.hip -- mifsk_frame_softbits (include/mifsk.h): a second pass over frames the
// receive loop has found, which gives back what the loop computes every frame from and then drops
// -- the mark and space magnitudes of each bit window (fsk_bit_analyze, fsk.c:107-169).
//
// A case is (frame, bit) of one stream: the window of cfg.bit_nsamples samples at
// frame.start - origin + cfg.bit_offset[bit] over the row, zeros beyond the row's end.  One wave
// takes 64 consecutive cases of one stream; every lane runs the correlator (the DPP broadcasts
// need all 64), a lane without a case shadows the wave's first and stores nothing.  The kernels
// CALL the receive loops' correlators and band_mag() and restate none of their arithmetic; a
// translation unit of its own, like mifsk_selftest.hip, so that no receive kernel's code moves.
//
// Three paths, chosen per wave (a uniform choice), all the same sums in the same order:
//   slab     bit windows below kTileMinBit samples.  The wave's windows belong to a few consecutive
//            frames: the span they cover is staged once into LDS with 16-byte loads, twelve in
//            flight per lane (zeros behind the row's end, PCM16 converted on the way), and
//            correlated out of it -- corr_slab_plain, or, where the bit length would put the
//            lanes' reads on a few banks, out of rows a pad word apart (corr_slab_skewed).
//   tiled    bit windows from kTileMinBit samples on, float rows: corr_global_tiled, as the loop
//            reads them -- when every window of the wave keeps its precondition (whole steps of
//            TILE_K samples inside the row).
//   checked  everything else -- a span wider than the slab (frames a silence apart, an unsorted
//            table), a long window at the row's end, long windows of PCM16: every lane reads its
//            own window from memory, each element tested against the row's end.  It depends on
//            nothing but the window, so nothing a frame table holds can make it overrun.
// The frame table is caller data: a start is used only after it has been clamped into [0, row
// length], so no address is formed from a value that was not compared with the row's length.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "mifsk.h"
#include "mifsk_batch.h"
#include "mifsk_ctx.h"
#include "mifsk_devlib.h"

namespace mifsk {

constexpr uint32_t kSoftMaxLdsFloats = 12288u;		// 48 KiB of the 64 a workgroup may have

struct SoftArgs {
    const DevCfg	*cfg;
    const double	*tw;
    RowsIn		in;		// rows of Src
    float		dc;		// rxnoise_term(): PCM16 only
    const uint64_t	*origin;
    const mifsk_frame	*frames;
    const uint32_t	*nframes;
    uint32_t		frames_cap;	// (frames_cap * n_bits fits 32 bits: the host entry checks)
    uint32_t		s0;		// first stream of this launch
    uint32_t		lds_floats;	// floats of dynamic LDS
    uint32_t		skew;		// pad words between the slab's rows of one bit length (0 / 1)
    uint32_t		n_bits, bit_nsamples;	// cfg->n_bits, cfg->bit_nsamples
    float2		*mag;
    uint64_t		*rawbits;
};

template <typename Src>
__device__ __forceinline__ float soft_sample( Src v, float dc )
{
    if constexpr ( sizeof(Src) == sizeof(float) )
	return v;
    else
	return sample_from_s16(v, dc);
}

// the window row[a .. a + B) read from memory by its own lane, row[i] = 0 for i >= nv: whole
// groups of 16 are looked at, of which only elements below nv are loaded and only the window's
// are summed
template <typename Src>
__device__ __forceinline__ void corr_row_checked( const double *__restrict__ tw, const Src *__restrict__ row,
	uint32_t a, uint32_t nv, uint32_t B, uint32_t lane, float dc, double (&acc)[4] )
{
    const uint32_t ng = ( B + 15u ) >> 4;
    for ( uint32_t g = 0; g < ng; g++ ) {
	const TwGroup G = tw_group_load(tw, g, lane);
	const uint64_t i0 = (uint64_t)a + 16u * g;
	float xs[16];
#pragma unroll
	for ( int j = 0; j < 16; j++ ) {
	    const uint64_t i = i0 + (uint32_t)j;
	    xs[j] = i < nv ? soft_sample<Src>(row[i], dc) : 0.0f;
	}
	const float4 s0 = make_float4(xs[0], xs[1], xs[2], xs[3]), s1 = make_float4(xs[4], xs[5], xs[6], xs[7]);
	const float4 s2 = make_float4(xs[8], xs[9], xs[10], xs[11]), s3 = make_float4(xs[12], xs[13], xs[14], xs[15]);
	const uint32_t left = B - 16u * g;
	dpp_settle();
	if ( left >= 16u )
	    group_bcast(acc, G, s0, s1, s2, s3);
	else
	    group_bcast_tail(acc, G, s0, s1, s2, s3, left);
    }
}

// elements of Src in a 16-byte vector
template <typename Src> constexpr uint32_t soft_vec() { return 16u / (uint32_t)sizeof(Src); }

// The 16 bytes of the row at element i0 (a multiple of the vector), RAW, as load4_raw takes them:
// the address is clamped into the row and nothing is done with the data, so that a run of these
// loads stays in flight together.  A vector that starts below nv lies inside the row -- the row's
// stride is a multiple of the vector and nv does not exceed it -- and so does the row's first
// vector whenever nv > 0, which the caller guarantees (it stages only when a window reaches into
// the row).
template <typename Src>
__device__ __forceinline__ int4 soft_load_raw( const Src *__restrict__ row, uint64_t i0, uint32_t nv )
{
    const uint64_t ii = i0 < nv ? i0 : 0u;
    return *reinterpret_cast<const int4 *>(row + ii);	// 16 B per lane, coalesced
}

// ... and what the loop sees in them: elements at or beyond nv are 0.0, whatever the memory holds
template <typename Src>
__device__ __forceinline__ void soft_unpack( const int4 raw, uint64_t i0, uint32_t nv, float dc, float (&v)[16 / sizeof(Src)] )
{
    constexpr uint32_t V = soft_vec<Src>();
    const int w[4] = { raw.x, raw.y, raw.z, raw.w };
    if constexpr ( sizeof(Src) == sizeof(float) ) {
#pragma unroll
	for ( int k = 0; k < 4; k++ )
	    v[k] = __builtin_bit_cast(float, w[k]);
    } else {
#pragma unroll
	for ( int k = 0; k < 4; k++ ) {
	    v[2 * k] = sample_from_s16((int16_t)( w[k] & 0xFFFF ), dc);
	    v[2 * k + 1] = sample_from_s16((int16_t)( (uint32_t)w[k] >> 16 ), dc);
	}
    }
#pragma unroll
    for ( uint32_t e = 0; e < V; e++ )
	v[e] = i0 + e < nv ? v[e] : 0.0f;		// (a select: what lies there may be NaN)
}

// The slab: slab-relative sample r sits in word r + (r / B) * skew -- rows of one bit length with
// `skew` (0 or 1) pad words in between, as the receive loops' slabs (store4_skewed): lanes whose
// windows start a bit length apart then read different banks where the bit length alone would put
// them on a few (40 samples: four banks of ds_read_b32's 32).  The V samples from r0 (a multiple of
// V) on:
template <uint32_t V>
__device__ __forceinline__ void soft_store( const DevCfg &cfg, float *slab, uint32_t skew, uint32_t r0, const float (&v)[V] )
{
    if ( skew == 0u ) {
#pragma unroll
	for ( uint32_t q = 0; q < V / 4u; q++ )
	    *reinterpret_cast<float4 *>(slab + r0 + 4u * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
	return;
    }
    uint32_t q, r;
    divmod_bit(cfg, r0, q, r);
    uint32_t w = r0 + q * skew;
#pragma unroll
    for ( uint32_t e = 0; e < V; e++ ) {
	slab[w++] = v[e];
	if ( ++r == cfg.bit_nsamples ) {
	    r = 0;
	    w += skew;
	}
    }
}

// the window that starts `rel` samples after the slab's first: corr_skewed_stream's reads (one
// ds_read_b32 per sample, 16 at a time, the row boundary by a select) with this slab's own skew
__device__ __forceinline__ void corr_slab_skewed( const DevCfg &cfg, const double *__restrict__ tw, const float *slab,
	uint32_t rel, uint32_t skew, uint32_t lane, double (&acc)[4] )
{
    const uint32_t B = cfg.bit_nsamples;
    uint32_t row, col;
    divmod_bit(cfg, rel, row, col);
    const float *p = slab + rel + row * skew;
    const uint32_t wrap = B - col;			// first n that falls into the next row
    const uint32_t last = B - 1u;
    const uint32_t ng = ( B + 15u ) >> 4;
    for ( uint32_t g = 0; g < ng; g++ ) {
	const TwGroup G = tw_group_load(tw, g, lane);
	float xs[16];
#pragma unroll
	for ( int j = 0; j < 16; j++ ) {
	    uint32_t n = 16u * g + (uint32_t)j;
	    n = n < last ? n : last;			// (uniform) never past the window
	    xs[j] = p[n + ( n >= wrap ? skew : 0u )];
	}
	const float4 s0 = make_float4(xs[0], xs[1], xs[2], xs[3]), s1 = make_float4(xs[4], xs[5], xs[6], xs[7]);
	const float4 s2 = make_float4(xs[8], xs[9], xs[10], xs[11]), s3 = make_float4(xs[12], xs[13], xs[14], xs[15]);
	const uint32_t left = B - 16u * g;
	dpp_settle();
	if ( left >= 16u )
	    group_bcast(acc, G, s0, s1, s2, s3);
	else
	    group_bcast_tail(acc, G, s0, s1, s2, s3, left);
    }
}

constexpr int kSoftStage = 12;		// 16-byte loads a lane keeps in flight while it stages

// LONG: bit windows of kTileMinBit samples or more (the LDS is the tile, TILE_FLOATS)
template <typename Src, bool LONG>
__global__ __launch_bounds__(64)
void softbits_kernel( const SoftArgs A )
{
    extern __shared__ float4 soft_lds4[];
    float *lds = reinterpret_cast<float *>(soft_lds4);
    const DevCfg &cfg = *A.cfg;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = A.s0 + blockIdx.y;
    const uint32_t nb = A.n_bits, B = A.bit_nsamples;		// (= cfg's; in the arguments, so that no load waits for them)
    const uint32_t c0 = 64u * blockIdx.x;
    // Everything the wave needs before it can stage is loaded at once, before the frame count is
    // known: the frame this lane's case would belong to -- its index clamped into the table, which
    // is [frames_cap] wide whatever the count says -- and its bit's offset.
    const uint32_t cs = c0 + lane;
    const uint32_t js_raw = cs / nb, ks = cs - js_raw * nb;
    const uint32_t js = js_raw < A.frames_cap ? js_raw : A.frames_cap - 1u;
    const uint64_t start_s = A.frames[(size_t)s * A.frames_cap + js].start;
    const uint32_t off_s = cfg.bit_offset[ks];
    const uint32_t nfr = A.nframes[s];
    const uint32_t n = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    const uint64_t origin = A.origin ? A.origin[s] : 0u;
    const uint32_t total = ( nfr < A.frames_cap ? nfr : A.frames_cap ) * nb;
    if ( c0 >= total )
	return;							// (whole waves: beyond this stream's frames)
    const uint32_t nw = total - c0 < 64u ? total - c0 : 64u;	// cases of this wave (uniform)
    const bool active = lane < nw;
    const uint32_t c = c0 + ( active ? lane : 0u );
    // a lane without a case shadows the wave's first (lane 0's: that one always has a case)
    const uint64_t start0 = ( (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)( start_s >> 32 )) << 32 )
			  | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)start_s);
    const uint32_t off0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)off_s);
    const uint64_t start = active ? start_s : start0;
    const uint32_t off = active ? off_s : off0;

    const uint32_t nv = n < A.in.stride ? n : (uint32_t)A.in.stride;	// samples the row holds
    const Src *row = reinterpret_cast<const Src *>(A.in.x) + (size_t)s * A.in.stride;
    const bool before = start < origin;				// samples the caller no longer holds
    const uint64_t rel = start - origin;
    // the window's start inside the row, nv for a window that lies wholly beyond it: a in [0, nv]
    uint32_t a = nv;
    if ( !before && rel < nv ) {
	const uint64_t a64 = rel + off;
	a = a64 < nv ? (uint32_t)a64 : nv;
    }
    const double *tw = A.tw;
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };

    if constexpr ( LONG ) {
	bool tiled = false;
	if constexpr ( sizeof(Src) == sizeof(float) ) {
	    // corr_global_tiled loads whole steps of TILE_K samples: all of them inside the row
	    const uint64_t reach = (uint64_t)TILE_K * ( ( (uint64_t)B + TILE_K - 1u ) / TILE_K );
	    tiled = __all((uint64_t)a + reach <= nv) != 0;
	    if ( tiled )
		corr_global_tiled(tw, reinterpret_cast<const float *>(row), a, nw, B, lane, lds, acc);
	}
	if ( !tiled )
	    corr_row_checked<Src>(tw, row, a, nv, B, lane, A.dc, acc);
    } else {
	// the span of the wave's windows that reach into the row; the LDS holds B zeros (whole
	// float4s) for the windows that do not, and the span behind them
	constexpr uint32_t V = soft_vec<Src>();
	const bool zero = a >= nv;
	const uint32_t lo = wave_min_u32(zero ? 0xFFFFFFFFu : a);
	const uint32_t amax = wave_max_u32(zero ? 0u : a);
	const uint32_t zpad = ( B + 3u ) & ~3u;
	const uint32_t lo_al = lo & ~( V - 1u );
	const bool any = lo != 0xFFFFFFFFu;
	// (64 bits: a row may end just below 2^32)
	const uint64_t span = any ? ( ( (uint64_t)amax + B - lo_al + ( V - 1u ) ) & ~(uint64_t)( V - 1u ) ) : 0u;
	const uint32_t skew = A.skew;
	const uint64_t words = span + ( span / B + 1u ) * skew;		// (soft_store's layout)
	if ( (uint64_t)zpad + words <= A.lds_floats ) {
	    float *slab = lds + zpad;
	    for ( uint32_t i = lane; i < zpad; i += 64u )
		lds[i] = 0.0f;
	    // kSoftStage loads in flight per lane, then their stores: a load whose vector lies beyond
	    // the span is made all the same (clamped into the row) and dropped
	    const uint32_t nvec = (uint32_t)span / V;
	    for ( uint32_t v0 = 0; v0 < nvec; v0 += 64u * (uint32_t)kSoftStage ) {
		int4 raw[kSoftStage];
#pragma unroll
		for ( int u = 0; u < kSoftStage; u++ )
		    raw[u] = soft_load_raw<Src>(row, (uint64_t)lo_al + (uint64_t)( v0 + 64u * (uint32_t)u + lane ) * V, nv);
#pragma unroll
		for ( int u = 0; u < kSoftStage; u++ ) {
		    const uint32_t v = v0 + 64u * (uint32_t)u + lane;
		    if ( v < nvec ) {
			float e[V];
			soft_unpack<Src>(raw[u], (uint64_t)lo_al + (uint64_t)v * V, nv, A.dc, e);
			soft_store<V>(cfg, slab, skew, v * V, e);
		    }
		}
	    }
	    wave_lds_sync();
	    if ( skew == 0u )
		corr_slab_plain(tw, zero ? lds : slab + ( a - lo_al ), B, lane, acc);
	    else
		corr_slab_skewed(cfg, tw, zero ? lds : slab, zero ? 0u : a - lo_al, skew, lane, acc);
	} else {
	    corr_row_checked<Src>(tw, row, a, nv, B, lane, A.dc, acc);
	}
    }
    if ( active ) {
	float2 m;
	if ( before )
	    m = make_float2(-1.0f, -1.0f);
	else
	    m = make_float2(band_mag(acc[0], acc[1], cfg.magscalar), band_mag(acc[2], acc[3], cfg.magscalar));
	A.mag[(size_t)s * A.frames_cap * nb + c] = m;		// 8 bytes per lane, contiguous across the wave
    }
}

// bit k of rawbits[s][j] = mark > space of bit window k, from the magnitudes just written (a
// frame's bits may lie in two waves of the kernel above); a frame before the origin (-1, -1)
// gives 0.  A block takes 256 / n_bits whole frames: one thread per (frame, bit) reads its pair --
// consecutive threads, consecutive pairs -- the waves' ballots make the block's string of
// decisions in LDS, and one thread per frame cuts its n_bits out of it.
__global__ __launch_bounds__(256)
void softbits_rawbits_kernel( const float2 *__restrict__ mag, const uint32_t *__restrict__ nframes,
	uint32_t frames_cap, uint32_t nb, uint32_t s0, unsigned long long *__restrict__ rawbits )
{
    __shared__ unsigned long long votes[4];
    const uint32_t s = s0 + blockIdx.y;
    const uint32_t per = 256u / nb;				// frames per block (n_bits <= 64: four or more)
    const uint32_t j0 = blockIdx.x * per;
    const uint32_t nfr = nframes[s] < frames_cap ? nframes[s] : frames_cap;
    if ( j0 >= nfr )
	return;							// (whole blocks)
    const uint32_t here = nfr - j0 < per ? nfr - j0 : per;	// frames of this block
    const uint32_t t = threadIdx.x;
    bool one = false;
    if ( t < here * nb ) {
	const float2 v = mag[( (size_t)s * frames_cap + j0 ) * nb + t];
	one = v.x > v.y;
    }
    const unsigned long long vote = __ballot(one);
    if ( ( t & 63u ) == 0u )
	votes[t >> 6] = vote;
    __syncthreads();
    if ( t < here ) {
	const uint32_t p = t * nb, w = p >> 6, sh = p & 63u;	// the frame's first decision: bit sh of word w
	unsigned long long bits = votes[w] >> sh;
	if ( sh + nb > 64u )
	    bits |= votes[w + 1u] << ( 64u - sh );		// (p + n_bits <= 256: word w + 1 exists; sh > 0 here)
	if ( nb < 64u )
	    bits &= ( 1ull << nb ) - 1ull;
	rawbits[(size_t)s * frames_cap + j0 + t] = bits;
    }
}

namespace {

// How many lanes of a 32-lane half share a bank of ds_read_b32 (32 banks of 4 bytes) at worst, when
// lane l reads the window that starts l bit lengths into a slab with `skew` pad words per row: the
// wave's pattern, consecutive bits of consecutive frames.
uint32_t soft_bank_ways( uint32_t B, uint32_t skew )
{
    uint32_t count[32] = {}, worst = 0;
    for ( uint32_t l = 0; l < 32u; l++ ) {
	const uint32_t c = ++count[( l * ( B + skew ) ) & 31u];
	worst = c > worst ? c : worst;
    }
    return worst;
}

template <typename Src>
void launch_softbits( const SoftArgs &A, bool long_windows, dim3 grid, hipStream_t st )
{
    const size_t lds = (size_t)A.lds_floats * sizeof(float);
    if ( long_windows )
	hipLaunchKernelGGL(( softbits_kernel<Src, true> ), grid, dim3(64), lds, st, A);
    else
	hipLaunchKernelGGL(( softbits_kernel<Src, false> ), grid, dim3(64), lds, st, A);
}

} // namespace
} // namespace mifsk

extern "C" int mifsk_frame_softbits( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_softbits_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !cfg || !io || !io->d_samples || !io->d_frames || !io->d_nframes || !io->d_mag )
	return -EINVAL;
    if ( io->nstreams <= 0 || io->frames_cap == 0 )
	return -EINVAL;
    if ( int rc = feed_rows_check(io->kind, io->rxnoise, io->d_samples, io->stream_stride) )
	return rc;			// (coalesced 16-byte staging)
    const bool s16 = io->kind == MIFSK_FEED_S16;
    if ( int rc = mifsk_check_cfg(cfg) )
	return rc;
    if ( cfg->auto_carrier_threshold > 0.0f )
	return -ENOTSUP;		// (a frame's bands are then its episode's)
    // a stream's cases are counted in 32 bits
    if ( io->frames_cap > ( 0xFFFFFFFFull - 64u ) / cfg->expect_n_bits )
	return -EINVAL;

    std::shared_lock<std::shared_mutex> gate;	// held until the launches are enqueued
    DevCfg d;
    const double *d_tw = nullptr;
    const DevCfg *d_cfg = nullptr;
    if ( int rc = lookup_tables(ctx, cfg, gate, d, &d_tw, &d_cfg) )
	return rc;

    SoftArgs A = {};
    A.cfg = d_cfg;
    A.tw = d_tw;
    A.in = rows_in(io);
    A.dc = s16 ? rxnoise_term(io->rxnoise) : 0.0f;
    A.origin = io->d_origin;
    A.frames = io->d_frames;
    A.nframes = io->d_nframes;
    A.frames_cap = (uint32_t)io->frames_cap;
    A.mag = reinterpret_cast<float2 *>(io->d_mag);
    A.rawbits = io->d_rawbits;
    const uint32_t B = d.bit_nsamples;
    A.n_bits = d.n_bits;
    A.bit_nsamples = B;
    const bool long_windows = B >= kTileMinBit;
    if ( long_windows ) {
	A.lds_floats = TILE_FLOATS;
    } else {
	// B zeros, 64 windows end to end, a quarter more for what lies between frames, and the
	// rounding of both ends: what a wave of consecutive frames needs.  A wave that needs more
	// reads its windows from memory.
	A.skew = soft_bank_ways(B, 1u) < soft_bank_ways(B, 0u) ? 1u : 0u;
	const uint32_t want = ( ( B + 3u ) & ~3u ) + 64u * B + 16u * B + 2u * B + 16u + ( 64u + 16u + 3u ) * A.skew;
	A.lds_floats = ( want < kSoftMaxLdsFloats ? want : kSoftMaxLdsFloats ) & ~3u;
    }
    const uint64_t cases = (uint64_t)A.frames_cap * d.n_bits;
    const unsigned waves = (unsigned)( ( cases + 63u ) / 64u );
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t per = 256u / d.n_bits;			// frames per block of softbits_rawbits_kernel
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	if ( s16 )
	    launch_softbits<int16_t>(A, long_windows, dim3(waves, rows), st);
	else
	    launch_softbits<float>(A, long_windows, dim3(waves, rows), st);
	if ( io->d_rawbits )
	    hipLaunchKernelGGL(softbits_rawbits_kernel, dim3(( A.frames_cap + per - 1u ) / per, rows), dim3(256), 0, st,
		    (const float2 *)A.mag, A.nframes, A.frames_cap, d.n_bits, s0,
		    reinterpret_cast<unsigned long long *>(io->d_rawbits));
	return 0;
    });
}
