// mifsk_batch.h -- the host side that the batch entries share (mifsk_carrier.hip, mifsk_softbits.hip,
// mifsk_channel.hip, mifsk_mux.hip): what they refuse of a batch of rows, how a batch of any number
// of rows becomes launches, and how a kernel with dynamic LDS is launched.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <type_traits>

#include "mifsk.h"

namespace mifsk {

constexpr uint32_t kMaxGridRows = 65535u;		// rows per launch (grid.y)

// `kernel` with lds_bytes of dynamic LDS: beyond 48 KiB the kernel's limit is raised first
template <class Args>
inline int launch_lds( void (*kernel)( const Args ), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
	const Args &args )
{
    if ( lds_bytes > 48u * 1024u
	    && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
				   (int)lds_bytes) != hipSuccess )
	return -EIO;
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args);
    return 0;
}

// nrows rows as blocks of kMaxGridRows at most: launch(s0, rows) for each, up to the first that
// returns non-zero; then what the launches left behind
template <class Launch>
inline int for_row_blocks( uint32_t nrows, Launch &&launch )
{
    for ( uint32_t s0 = 0; s0 < nrows; s0 += kMaxGridRows ) {
	const uint32_t rows = nrows - s0 < kMaxGridRows ? nrows - s0 : kMaxGridRows;
	if ( int rc = launch(s0, rows) )
	    return rc;
    }
    return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// elements of 16 bytes: PCM16 or float scalars, one or two (I, Q) per element
inline uint32_t rows_vec( bool cx, bool s16 ) { return 16u / ( ( s16 ? 2u : 4u ) * ( cx ? 2u : 1u ) ); }

// rows start on 16 bytes and lie whole 16-byte vectors apart, as every entry takes them
inline bool rows_aligned( const void *rows, size_t stride, uint32_t vec )
{
    return ( (uintptr_t)rows & 15u ) == 0 && stride % vec == 0;
}

// what the entries that read a feed of real rows refuse of it
inline int feed_rows_check( uint32_t kind, float rxnoise, const void *d_samples, size_t stride )
{
    if ( kind != MIFSK_FEED_F32 && kind != MIFSK_FEED_S16 )
	return -EINVAL;
    const bool s16 = kind == MIFSK_FEED_S16;
    if ( !s16 && !( rxnoise == 0.0f ) )
	return -EINVAL;
    return rows_aligned(d_samples, stride, rows_vec(false, s16)) ? 0 : -EINVAL;
}

// f(complex rows, PCM16 scalars) with both as compile-time constants
template <class F>
inline int dispatch_kind( bool cx, bool s16, F &&f )
{
    if ( cx )
	return s16 ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return s16 ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

} // namespace mifsk
