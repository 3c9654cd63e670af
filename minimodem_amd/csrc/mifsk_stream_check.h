// mifsk_stream_check.h -- what the stream objects of the row stages share and needs no device
// (mifsk_channel_stream_check.h, mifsk_mux_stream_check.h; the owner that calls HIP is
// mifsk_stream_state.h): a tail's room, the five fields a feed's kernel gets of an object's state, and
// where the two sides of that state lie.  It calls no HIP: tools/stream_shared_check.h checks it on a
// CPU under the sanitizers, from the two stages' programs.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mifsk {

// a tail's room per row and side, in elements of `esz` bytes: n of them rounded up to whole 16-byte
// vectors, one vector at least
inline uint32_t stream_tail_room( uint32_t n, uint32_t esz )
{
    const uint32_t bytes = ( n * esz + 15u ) / 16u * 16u;
    return ( bytes ? bytes : 16u ) / esz;
}

// What a feed's kernel gets of the object, behind the stage's batch arguments (ChannelStreamArgs,
// MuxStreamArgs).  Records and tails exist twice: a feed reads one side and writes the other.
template <class Rec>
struct StreamSides {
    const Rec	*rec_in;	// [nstreams]: the side this feed reads
    Rec		*rec_out;	// ... and the one it writes
    const char	*tail_in;	// [nstreams * rows][tail_cap] elements
    char	*tail_out;
    uint32_t	tail_cap;	// elements of a tail's room
};

static_assert(sizeof(StreamSides<void>) == 40 && offsetof(StreamSides<void>, tail_in) == 16
	      && offsetof(StreamSides<void>, tail_cap) == 32, "four pointers and a count, as the kernels' code reads them");

// Where the sides lie in an object of nstreams streams with `rows` rows each: side `parity` of the
// records [2][nstreams] and of the tails [2][nstreams * rows][tail_cap] elements is the one the next
// feed reads, and only a feed that went out whole flips the parity.
struct StreamHalves {
    size_t	rec_in, rec_out;	// records from the first record
    size_t	tail_in, tail_out;	// bytes from the first tail
    size_t	nrec, tail_bytes;	// both sides: what the object allocates
};

inline StreamHalves stream_halves( unsigned parity, size_t nstreams, size_t rows, uint32_t tail_cap, uint32_t esz )
{
    const size_t in = parity & 1u, side = nstreams * rows * tail_cap * esz;
    return StreamHalves{in * nstreams, ( in ^ 1u ) * nstreams, in * side, ( in ^ 1u ) * side, 2u * nstreams, 2u * side};
}

} // namespace mifsk
