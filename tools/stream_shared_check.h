// stream_shared_check.h -- the checks of what the two stream objects share
// (minimodem_amd/csrc/mifsk_stream_check.h), for channel_stream_check.cpp (one row per stream) and
// mux_stream_check.cpp (K rows per stream): a tail's room, and where the two sides of an object's
// records and tails lie.  `expect` is the program's own.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mifsk_stream_check.h"

// records of `rec_bytes` bytes; objects of 1, 2, 3 and 65537 streams with `rows` rows each
template <class Expect>
inline void stream_shared_checks( Expect expect, size_t rec_bytes, uint32_t rows )
{
    using namespace mifsk;
    expect(rec_bytes % 16u, 0, "a record is whole 16-byte vectors", rec_bytes, 0);
    for ( uint32_t esz : { 2u, 4u, 8u } ) {
	for ( uint32_t n : { 0u, 1u, 3u, 4u, 384u } ) {
	    // the room: n elements in whole 16-byte vectors, one at least, and no vector more
	    const uint32_t cap = stream_tail_room(n, esz);
	    expect(cap >= n && cap * esz >= 16u, 1, "stream_tail_room holds n, a vector at least", n, esz);
	    expect(cap * esz % 16u, 0, "stream_tail_room is whole vectors", n, esz);
	    expect(cap * esz < n * esz + 16u + ( n == 0u ? 16u : 0u ), 1, "stream_tail_room is no vector more", n, esz);
	    for ( size_t nstreams : { (size_t)1, (size_t)2, (size_t)3, (size_t)65537 } ) {
		const size_t side = nstreams * rows * cap * esz;
		for ( unsigned parity : { 0u, 1u } ) {
		    const StreamHalves h = stream_halves(parity, nstreams, rows, cap, esz);
		    expect(h.nrec == 2u * nstreams && h.tail_bytes == 2u * side, 1, "two sides are allocated", nstreams, rows);
		    // inside the allocation, apart, each on 16 bytes
		    expect(h.rec_in + nstreams <= h.nrec && h.rec_out + nstreams <= h.nrec, 1, "records inside", nstreams, parity);
		    expect(h.rec_in + nstreams <= h.rec_out || h.rec_out + nstreams <= h.rec_in, 1, "records apart", nstreams, parity);
		    expect(h.tail_in + side <= h.tail_bytes && h.tail_out + side <= h.tail_bytes, 1, "tails inside", nstreams, parity);
		    expect(h.tail_in + side <= h.tail_out || h.tail_out + side <= h.tail_in, 1, "tails apart", nstreams, parity);
		    expect(( h.rec_in * rec_bytes | h.rec_out * rec_bytes | h.tail_in | h.tail_out ) % 16u, 0, "sides on 16 bytes", nstreams, parity);
		    // a flip exchanges the halves
		    const StreamHalves f = stream_halves(parity ^ 1u, nstreams, rows, cap, esz);
		    expect(f.rec_in == h.rec_out && f.rec_out == h.rec_in && f.tail_in == h.tail_out && f.tail_out == h.tail_in,
			   1, "a flip exchanges the halves", nstreams, parity);
		}
		// the owner's rule over a run of feeds, some refused: a feed that went out is read next where
		// it wrote, one that did not is followed by a read of the same half
		unsigned parity = 0u;
		const bool went_out[8] = { true, false, true, true, false, false, true, false };
		for ( bool ok : went_out ) {
		    const StreamHalves h = stream_halves(parity, nstreams, rows, cap, esz);
		    if ( ok )
			parity ^= 1u;
		    const StreamHalves next = stream_halves(parity, nstreams, rows, cap, esz);
		    expect(next.rec_in == ( ok ? h.rec_out : h.rec_in ) && next.tail_in == ( ok ? h.tail_out : h.tail_in ),
			   1, ok ? "the next feed reads what this one wrote" : "no flip: the same half is read again", nstreams, ok);
		}
	    }
	}
    }
}
