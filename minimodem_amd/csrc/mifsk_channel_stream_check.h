// mifsk_channel_stream_check.h -- the host logic of a channel stream (include/mifsk/channel_stream.h,
// mifsk_channel_stream.hip) that needs no device: the counting of outputs, a stream's record and its
// tail, and what a feed refuses of its arguments; what it shares with the multiplexer's stream is in
// mifsk_stream_check.h.  It calls no HIP: tools/channel_stream_check.cpp runs it on a CPU under the
// sanitizers (tests/test_channel_stream_args.py).
#pragma once

#include <cerrno>
#include <cstdint>

#include "mifsk.h"
#include "mifsk/channel_stream.h"
#include "mifsk_batch.h"
#include "mifsk_stream_check.h"

namespace mifsk {

// M(n): the outputs whose windows lie whole in the first n elements
inline uint64_t stream_outputs_of( uint32_t T, uint32_t D, uint64_t n )
{
    return T != 0u && D != 0u && n >= T ? ( n - T ) / D + 1u : 0u;
}

// M(seen + k) - M(seen); a sum that would pass 2^64 counts up to 2^64 - 1
inline uint64_t stream_outputs( uint32_t T, uint32_t D, uint64_t seen, uint64_t k )
{
    const uint64_t end = seen + k < seen ? ~0ull : seen + k;
    return stream_outputs_of(T, D, end) - stream_outputs_of(T, D, seen);
}

// What a stream keeps between feeds: the elements it has seen and the next output it delivers.
// `next` is M(seen), but behind a seek to n0: there it is the first m with m D >= n0, which M(seen)
// reaches T - 1 elements later at the latest, and an output below it is never delivered.
struct StreamRecord {
    uint64_t	seen, next;
};

// a seek's record: the first output that reads nothing in front of n0
inline StreamRecord stream_record_at( uint32_t D, uint64_t n0 ) { return StreamRecord{n0, n0 / D + ( n0 % D != 0u )}; }

// seeks go this far: next * D <= seen + D and the sums of a feed stay far below 2^64
constexpr uint64_t kStreamMaxSeen = 1ull << 63;

// The tail, elements [next D, seen) of the stream, or none when next D >= seen.
// It never holds more than T - 1 elements, which its room is made for (stream_tail_room of T - 1,
// mifsk_stream_check.h).  next >= M(seen) always (it is M(seen), or a seek's
// first output, which is no smaller), so the tail is no longer than seen - M(seen) D.  For seen < T,
// M = 0 and that is seen <= T - 1.  For seen >= T, M = floor((seen - T) / D) + 1 > (seen - T) / D, so
// M D > seen - T, seen - M D < T, and both sides are integers: seen - M D <= T - 1.
inline uint64_t stream_tail_len( uint32_t D, const StreamRecord &r )
{
    return r.seen > r.next * D ? r.seen - r.next * D : 0u;
}

// what a feed has to know of its object
struct StreamShape {
    bool	cx, s16;	// the plan's kind
    uint32_t	D, K;		// ... its decimation and channels
    int		nstreams;
};

// What mifsk_channel_stream_feed refuses behind the NULL object and io, in the header's order:
// everything the batch entry of the same flag refuses of the io, a number of streams that is not the
// object's, unknown flags, then an out_stride and a nout_cap below ceil(kmax / D): a feed delivers
// M(seen + k) - M(seen) <= ceil(k / D) outputs per row, and dropping one would break the continuation.
inline int stream_feed_check( const StreamShape &sh, const mifsk_channel_io *io, uint32_t flags )
{
    const OutKind ok = channel_out_kind(( flags & MIFSK_CHANNEL_STREAM_IQ ) != 0u);
    if ( int rc = rows_io_check(sh.K, io, io->d_rows, rows_vec(sh.cx, sh.s16), ok.vec, ok.max) )
	return rc;
    if ( io->nstreams != sh.nstreams )
	return -EINVAL;
    if ( flags & ~MIFSK_CHANNEL_STREAM_IQ )
	return -EINVAL;
    const uint64_t kmax = stream_kmax(io), need = ( kmax + sh.D - 1u ) / sh.D;
    if ( io->out_stride < need )
	return -EINVAL;
    if ( io->nout_cap < need )
	return -EINVAL;
    return 0;
}

} // namespace mifsk
