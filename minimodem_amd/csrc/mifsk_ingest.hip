// mifsk_ingest.hip -- the step before the path: what the reference
// does between the file and samplebuf[] -- libsndfile's S16 -> float conversion
// (simpleaudio-sndfile.c:42-56, sf_readf_float on a PCM16 file) and the
// --Xrxnoise term (simpleaudio-sndfile.c:64-69) -- on the device, over a whole
// batch of streams, so that 16-bit recordings cross PCIe and are read from HBM
// at 2 bytes per sample; the resident session's compact-and-append of a feed's
// new samples (session_append_kernel); plus the RIFF/WAVE header parse for the
// batched file loader.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <cstring>

#include "mifsk.h"
#include "mifsk_device.h"

namespace mifsk {

// One thread converts 8 consecutive samples: one 16-byte load, two 16-byte
// stores.  HBM-bound: 2 B read + 4 B written per sample.  Samples at or beyond
// the stream's length are written as 0.0 up to the row's stride, so the whole
// row is defined afterwards.
//   value / 32768 : libsndfile's normalisation of PCM16 (a power of two: exact)
//   + dc          : what --Xrxnoise really adds -- `rand()/RAND_MAX` is an
//                   integer division, i.e. 0, so the "noise" is the constant
//                   (0 - 0.5f) * (2 * factor)
__global__ __launch_bounds__(256)
void ingest_s16_kernel( const int16_t *__restrict__ pcm, size_t pcm_stride,
	float *__restrict__ out, size_t out_stride,
	const uint32_t *__restrict__ nsamples_v, uint32_t nsamples_u, float dc, int vec_ok )
{
    const uint32_t s = blockIdx.y;
    const uint32_t n = nsamples_v ? nsamples_v[s] : nsamples_u;
    const int16_t *row = pcm + (size_t)s * pcm_stride;
    float *dst = out + (size_t)s * out_stride;
    const size_t i0 = ( (size_t)blockIdx.x * blockDim.x + threadIdx.x ) * 8u;
    if ( i0 >= out_stride )
	return;
    float v[8];
    if ( vec_ok && i0 + 8 <= n ) {
	const int4 raw = *reinterpret_cast<const int4 *>(row + i0);	// 8 x int16, coalesced
	const int w[4] = { raw.x, raw.y, raw.z, raw.w };
#pragma unroll
	for ( int k = 0; k < 4; k++ ) {
	    v[2 * k] = sample_from_s16((int16_t)( w[k] & 0xFFFF ), dc);
	    v[2 * k + 1] = sample_from_s16((int16_t)( (uint32_t)w[k] >> 16 ), dc);
	}
    } else {
#pragma unroll
	for ( int k = 0; k < 8; k++ )
	    v[k] = i0 + k < n ? sample_from_s16(row[i0 + k], dc) : 0.0f;
    }
    if ( vec_ok && i0 + 8 <= out_stride ) {
	*reinterpret_cast<float4 *>(dst + i0) = make_float4(v[0], v[1], v[2], v[3]);
	*reinterpret_cast<float4 *>(dst + i0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
	for ( int k = 0; k < 8; k++ )
	    if ( i0 + k < out_stride )
		dst[i0 + k] = v[k];
    }
}

// --Xrxnoise on input that is already float: x += dc over the valid samples
__global__ __launch_bounds__(256)
void offset_f32_kernel( float *__restrict__ x, size_t stride,
	const uint32_t *__restrict__ nsamples_v, uint32_t nsamples_u, float dc )
{
    const uint32_t s = blockIdx.y;
    const uint32_t n = nsamples_v ? nsamples_v[s] : nsamples_u;
    float *row = x + (size_t)s * stride;
    const size_t i0 = ( (size_t)blockIdx.x * blockDim.x + threadIdx.x ) * 4u;
    for ( int k = 0; k < 4; k++ )
	if ( i0 + k < n )
	    row[i0 + k] = sample_from_f32(row[i0 + k], dc);
}

// The resident session's feed (mifsk_session.cpp): every stream's row is rebuilt in the OTHER
// row buffer -- what the loop has not passed of the old row, moved to the front, the new samples
// behind it, zeros up to the feed's width.  The kept part moves by an arbitrary offset and
// overlaps itself, so it is never compacted in place.  One thread makes one float4 of the
// destination (rows are 16-byte aligned, width is a multiple of 4): 16-byte stores always.  The
// sources sit wherever `drop` and the caller's layout put them: a vector that lies whole inside
// the kept part or inside the new samples is read with the widest load its address allows (16 B;
// 8 B for four PCM16 samples), element by element otherwise, and so is the vector that straddles
// an end.  Nothing outside old[i][drop .. drop + keep) and fresh_i[0 .. k) is ever read: behind a
// caller's piece the memory is the caller's, or nobody's.  HBM-bound: per sample 4 B read (2 B for
// new PCM16) and 4 B written.  dc: rxnoise_term(), applied to the new samples only (the kept ones
// got it when they came); `offset` == 0 leaves new floats exactly as they are.
template <class Src>
__device__ inline float session_fresh( const Src *__restrict__ f, uint32_t i, float dc, int offset )
{
    if constexpr ( sizeof(Src) == sizeof(float) )
	return offset ? sample_from_f32(f[i], dc) : f[i];
    else
	return sample_from_s16(f[i], dc);
}

template <class Src>
__global__ __launch_bounds__(256)
void session_append_kernel( const float *__restrict__ old_rows, size_t old_stride,
	float *__restrict__ new_rows, size_t new_stride, uint32_t width,
	const Src *__restrict__ fresh, const SessionRow *__restrict__ table,
	uint32_t *__restrict__ lens, uint64_t *__restrict__ origins, int nstreams, float dc, int offset )
{
    const uint32_t j0 = ( blockIdx.x * blockDim.x + threadIdx.x ) * 4u;
    for ( int i = blockIdx.y; i < nstreams; i += gridDim.y ) {
	const SessionRow r = table[i];
	const uint32_t end = r.keep + r.k;		// (the host keeps this below 2^32)
	if ( j0 == 0u ) {
	    lens[i] = end;
	    origins[i] = r.origin;
	}
	if ( j0 >= width )
	    continue;
	const float *old = old_rows + (size_t)i * old_stride + r.drop;
	const Src *f = fresh + r.src_off;
	float4 o;
	if ( j0 + 4u <= r.keep ) {
	    const float *p = old + j0;
	    if ( ( (uintptr_t)p & 15u ) == 0u )
		o = *reinterpret_cast<const float4 *>(p);
	    else
		o = make_float4(p[0], p[1], p[2], p[3]);
	} else if ( j0 >= end ) {
	    o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	} else if ( j0 >= r.keep && j0 + 4u <= end ) {
	    const uint32_t q = j0 - r.keep;
	    const Src *p = f + q;
	    if constexpr ( sizeof(Src) == sizeof(float) ) {
		if ( ( (uintptr_t)p & 15u ) == 0u ) {
		    o = *reinterpret_cast<const float4 *>(p);
		    if ( offset )
			o = make_float4(sample_from_f32(o.x, dc), sample_from_f32(o.y, dc),
					sample_from_f32(o.z, dc), sample_from_f32(o.w, dc));
		} else {
		    o = make_float4(session_fresh(f, q, dc, offset), session_fresh(f, q + 1u, dc, offset),
				    session_fresh(f, q + 2u, dc, offset), session_fresh(f, q + 3u, dc, offset));
		}
	    } else {
		if ( ( (uintptr_t)p & 7u ) == 0u ) {
		    const int2 raw = *reinterpret_cast<const int2 *>(p);
		    o = make_float4(sample_from_s16((int16_t)( raw.x & 0xFFFF ), dc),
				    sample_from_s16((int16_t)( (uint32_t)raw.x >> 16 ), dc),
				    sample_from_s16((int16_t)( raw.y & 0xFFFF ), dc),
				    sample_from_s16((int16_t)( (uint32_t)raw.y >> 16 ), dc));
		} else {
		    o = make_float4(session_fresh(f, q, dc, offset), session_fresh(f, q + 1u, dc, offset),
				    session_fresh(f, q + 2u, dc, offset), session_fresh(f, q + 3u, dc, offset));
		}
	    }
	} else {
	    float e[4];
#pragma unroll
	    for ( uint32_t c = 0; c < 4u; c++ ) {
		const uint32_t j = j0 + c;
		e[c] = j < r.keep ? old[j] : j < end ? session_fresh(f, j - r.keep, dc, offset) : 0.0f;
	    }
	    o = make_float4(e[0], e[1], e[2], e[3]);
	}
	*reinterpret_cast<float4 *>(new_rows + (size_t)i * new_stride + j0) = o;
    }
}

} // namespace mifsk

using mifsk::rxnoise_term;	// (mifsk_device.h)

int mifsk::launch_session_append( const float *old_rows, size_t old_stride, float *new_rows, size_t new_stride,
	uint32_t width, const void *fresh, bool s16, const SessionRow *d_table, uint32_t *d_lens,
	uint64_t *d_origin, int nstreams, float dc, void *stream )
{
    if ( nstreams <= 0 || width == 0u || ( width & 3u ) || ( old_stride & 3u ) || ( new_stride & 3u )
	    || width > new_stride || !new_rows || !d_table || !d_lens || !d_origin )
	return -EINVAL;
    const uint32_t per_block = 256u * 4u;
    dim3 grid(( width + per_block - 1u ) / per_block, (unsigned)( nstreams < 65535 ? nstreams : 65535 ));
    if ( s16 )
	hipLaunchKernelGGL(mifsk::session_append_kernel<int16_t>, grid, dim3(256), 0, (hipStream_t)stream,
			   old_rows, old_stride, new_rows, new_stride, width, (const int16_t *)fresh, d_table,
			   d_lens, d_origin, nstreams, dc, 1);
    else
	hipLaunchKernelGGL(mifsk::session_append_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream,
			   old_rows, old_stride, new_rows, new_stride, width, (const float *)fresh, d_table,
			   d_lens, d_origin, nstreams, dc, dc != 0.0f ? 1 : 0);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mifsk_ingest_s16( mifsk_ctx *ctx, const int16_t *d_pcm, size_t pcm_stride,
	float *d_samples, size_t stream_stride, const uint32_t *d_nsamples, uint32_t nsamples,
	int nstreams, float rxnoise, void *stream )
{
    if ( !ctx || !d_pcm || !d_samples || nstreams < 0 )
	return -EINVAL;
    if ( nstreams == 0 || stream_stride == 0 )
	return 0;
    if ( !d_nsamples && ( nsamples > pcm_stride || nsamples > stream_stride ) )
	return -EINVAL;
    if ( hipSetDevice(mifsk::ctx_device(ctx)) != hipSuccess )
	return -EIO;
    const int vec_ok = pcm_stride % 8 == 0 && stream_stride % 4 == 0
		     && (uintptr_t)d_pcm % 16 == 0 && (uintptr_t)d_samples % 16 == 0;
    const size_t per_block = 256 * 8;
    dim3 grid((unsigned)( ( stream_stride + per_block - 1 ) / per_block ), (unsigned)nstreams);
    hipLaunchKernelGGL(mifsk::ingest_s16_kernel, grid, dim3(256), 0, (hipStream_t)stream,
		       d_pcm, pcm_stride, d_samples, stream_stride, d_nsamples, nsamples,
		       rxnoise_term(rxnoise), vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mifsk_ingest_rxnoise_f32( mifsk_ctx *ctx, float *d_samples, size_t stream_stride,
	const uint32_t *d_nsamples, uint32_t nsamples, int nstreams, float rxnoise, void *stream )
{
    if ( !ctx || !d_samples || nstreams < 0 )
	return -EINVAL;
    if ( nstreams == 0 || stream_stride == 0 || rxnoise == 0.0f )
	return 0;
    if ( hipSetDevice(mifsk::ctx_device(ctx)) != hipSuccess )
	return -EIO;
    const size_t per_block = 256 * 4;
    dim3 grid((unsigned)( ( stream_stride + per_block - 1 ) / per_block ), (unsigned)nstreams);
    hipLaunchKernelGGL(mifsk::offset_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream,
		       d_samples, stream_stride, d_nsamples, nsamples, rxnoise_term(rxnoise));
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// ---- RIFF/WAVE header (host) -------------------------------------------------
static uint32_t rd32( const unsigned char *p ) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
static uint32_t rd16( const unsigned char *p ) { return p[0] | p[1] << 8; }

// `have` bytes of the file are in memory at `file`, the file itself is `len` bytes long
// (the batched loader reads headers only)
namespace mifsk { int wav_parse_sized( const void *file, size_t have, size_t len, mifsk_wav_info *info ); }

extern "C" int mifsk_wav_parse( const void *file, size_t len, mifsk_wav_info *info )
{
    return mifsk::wav_parse_sized(file, len, len, info);
}

int mifsk::wav_parse_sized( const void *file, size_t have, size_t len, mifsk_wav_info *info )
{
    if ( !file || !info || have > len )
	return -EINVAL;
    memset(info, 0, sizeof *info);
    const unsigned char *p = (const unsigned char *)file;
    if ( have < 12 || memcmp(p, "RIFF", 4) != 0 || memcmp(p + 8, "WAVE", 4) != 0 )
	return -EINVAL;
    bool have_fmt = false;
    unsigned block_align = 0;
    size_t pos = 12;
    while ( pos + 8 <= have ) {
	const uint32_t sz = rd32(p + pos + 4);
	const unsigned char *body = p + pos + 8;
	const size_t avail = len - ( pos + 8 );		// of the file
	const size_t here = have - ( pos + 8 );		// of it, in memory
	if ( memcmp(p + pos, "fmt ", 4) == 0 ) {
	    if ( sz < 16 || here < 16 )
		return -EINVAL;
	    unsigned tag = rd16(body);
	    info->channels = rd16(body + 2);
	    info->sample_rate = rd32(body + 4);
	    block_align = rd16(body + 12);
	    info->bits_per_sample = rd16(body + 14);
	    if ( tag == 0xFFFE && sz >= 26 && here >= 26 )	// WAVE_FORMAT_EXTENSIBLE: sub-format GUID
		tag = rd16(body + 24);
	    if ( tag == 1 && info->bits_per_sample == 16 )
		info->is_float = 0;
	    else if ( tag == 3 && info->bits_per_sample == 32 )
		info->is_float = 1;
	    else
		return -ENOTSUP;				// the reference's tests use PCM16 and float32 only
	    have_fmt = true;
	} else if ( memcmp(p + pos, "data", 4) == 0 ) {
	    if ( !have_fmt || block_align == 0 )
		return -EINVAL;
	    info->data_offset = pos + 8;
	    const size_t bytes = sz <= avail ? sz : avail;	// a truncated file yields what is there
	    info->nframes = bytes / block_align;
	    return info->channels == 1 ? 0 : -ENOTSUP;		// minimodem opens its input mono
	}
	pos += 8 + (size_t)sz + ( sz & 1u );
    }
    return -EINVAL;
}
