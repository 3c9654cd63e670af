// mifsk_batch.h -- the host side that the batch entries share (mifsk_carrier.hip, mifsk_softbits.hip,
// mifsk_channel.hip, mifsk_mux.hip, mifsk_impair.hip, mifsk_fm.hip): what a batch of rows is (RowsIn),
// what they refuse of one, how a batch of any number of rows becomes launches, and how a kernel with
// dynamic LDS is launched.  Host only, but for RowsIn::len (mifsk_rows.h); the checks call no HIP
// (tools/rows_check.cpp runs them on a CPU).
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

// a kind of scalars that the entries know
inline int kind_check( uint32_t kind ) { return kind == MIFSK_FEED_F32 || kind == MIFSK_FEED_S16 ? 0 : -EINVAL; }

// what the entries refuse of their output rows: `vec` elements are 16 bytes, a row is 1 .. out_max elements
inline int out_rows_check( const void *d_out, size_t out_stride, uint32_t vec, uint64_t out_max )
{
    return rows_aligned(d_out, out_stride, vec) && out_stride != 0 && out_stride <= out_max ? 0 : -EINVAL;
}

// what the entries that read a feed of real rows refuse of it
inline int feed_rows_check( uint32_t kind, float rxnoise, const void *d_samples, size_t stride )
{
    if ( int rc = kind_check(kind) )
	return rc;
    const bool s16 = kind == MIFSK_FEED_S16;
    if ( !s16 && !( rxnoise == 0.0f ) )
	return -EINVAL;
    return rows_aligned(d_samples, stride, rows_vec(false, s16)) ? 0 : -EINVAL;
}

// The input rows of a batch as the row stages' kernels take them.  28 bytes, so that the 32-bit member
// behind it in a kernel's arguments lies where it lay behind four loose members: grouping them moves
// no kernel argument and changes no kernel's code.
struct __attribute__((packed, aligned(4))) RowsIn {
    const void		*x;		// NULL where the entry allows it
    size_t		stride;		// elements between rows
    const uint32_t	*nsamples_v;	// [rows] or NULL
    uint32_t		nsamples_u;	// ... then every row's length
    // row s's length, no more than the stride (`to_stride`) and than out_stride (mifsk_rows.h)
    __device__ uint64_t len( size_t s, bool to_stride = true, uint64_t out_stride = ~0ull ) const;
};

static_assert(sizeof(RowsIn) == 28, "three pointers and a count");

// ... of any io that begins with d_samples, stream_stride, d_nsamples, nsamples
template <class IO>
inline RowsIn rows_in( const IO *io )
{
    return RowsIn{io->d_samples, io->stream_stride, io->d_nsamples, io->nsamples};
}

// ... and the most that one call gives a row of it, as the host knows it: a row's length is a
// uint32_t and stops at the stride, and with per-row lengths any of them may be the stride
template <class IO>
inline uint64_t stream_kmax( const IO *io )
{
    const uint64_t stride = io->stream_stride < 0xFFFFFFFFull ? io->stream_stride : 0xFFFFFFFFull;
    return io->d_nsamples || io->nsamples > stride ? stride : io->nsamples;
}

// An output element of the channelizer is a float, or with `iq` an (I, Q) pair: `vec` of them are 16
// bytes, a row is `max` of them at most
struct OutKind {
    uint32_t	vec;
    uint64_t	max;
};

constexpr OutKind channel_out_kind( bool iq ) { return iq ? OutKind{2u, 0x7FFFFFFEull} : OutKind{4u, 0xFFFFFFFCull}; }

// What the channelizer's and the multiplexer's entries refuse of an io (mifsk_channel_io, mifsk_mux_io:
// rows in, d_nout, out_stride, nout_cap; `d_out` its output rows), in the headers' order: `in_vec` and
// `out_vec` elements are 16 bytes of an input and an output row, an output row is out_max elements at
// most, K rows go out per stream.
template <class IO>
inline int rows_io_check( uint32_t K, const IO *io, const void *d_out, uint32_t in_vec, uint32_t out_vec, uint64_t out_max )
{
    if ( !io->d_samples || !d_out || !io->d_nout || io->nstreams <= 0 )
	return -EINVAL;
    if ( !rows_aligned(io->d_samples, io->stream_stride, in_vec) )
	return -EINVAL;
    if ( int rc = out_rows_check(d_out, io->out_stride, out_vec, out_max) )
	return rc;
    if ( io->nout_cap > io->out_stride || (uint64_t)io->nstreams * K > 0x7FFFFFFFull )
	return -EINVAL;
    return 0;
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
