// mifsk_rows.h -- the device side that the row stages' kernels share (mifsk_mux.hip, mifsk_impair.hip,
// mifsk_fm.hip, mifsk_channel.hip): a row's length, the PCM16 conversions both ways and the 16-byte
// PCM16 vector.  (sample_from_s16 of mifsk_devlib.h adds the rxnoise term: another function.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mifsk_batch.h"

namespace mifsk {

__device__ __forceinline__ uint64_t RowsIn::len( size_t s, bool to_stride, uint64_t out_stride ) const
{
    uint64_t W = nsamples_v ? nsamples_v[s] : nsamples_u;
    if ( to_stride && W > stride )
	W = stride;
    if ( W > out_stride )
	W = out_stride;
    return W;
}

// 16 bytes of PCM16
struct alignas(16) S16x8 { int16_t v[8]; };

// PCM16 as the float the definitions read (libsndfile's normalisation: a power of two, exact)
__device__ __forceinline__ float rows_f32( int16_t v ) { return (float)v / 32768.0f; }

// the float as the PCM16 write conversion stores it
__device__ __forceinline__ int16_t rows_s16( float v )
{
    float t = v * 32767.0f;
    if ( t > 32767.0f )
	t = 32767.0f;
    if ( t < -32768.0f )
	t = -32768.0f;
    return t != t ? (int16_t)0 : (int16_t)(int)rintf(t);
}

} // namespace mifsk
