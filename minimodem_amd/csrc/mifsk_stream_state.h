// mifsk_stream_state.h -- the one owner of what a stream object keeps on the device between feeds
// (mifsk_channel_stream.hip, mifsk_mux_stream.hip): per stream a record (Rec: the stage's counters, `seen`
// among them) and per row a tail, both twice.  Where the sides lie is plain arithmetic, checked
// without a device (mifsk_stream_check.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk_hostmem.h"
#include "mifsk_stream_check.h"

namespace mifsk {

template <class Rec>
struct StreamState {
    int			device = 0;
    int			nstreams = 0;
    uint32_t		rows = 0;	// per stream
    uint32_t		tail_cap = 0;	// elements per row and side
    uint32_t		esz = 0;	// bytes of an element
    unsigned		parity = 0;	// the side the next feed reads
    DevMem<Rec>		rec;		// [2][nstreams]
    DevMem<char>	tails;		// [2][nstreams * rows][tail_cap] elements

    StreamHalves halves() const { return stream_halves(parity, (size_t)nstreams, rows, tail_cap, esz); }

    // both sides, zeroed: -EIO for the device, then the allocation's code
    int alloc( int device_, int nstreams_, uint32_t rows_, uint32_t tail_cap_, uint32_t esz_ )
    {
	device = device_, nstreams = nstreams_, rows = rows_, tail_cap = tail_cap_, esz = esz_, parity = 0u;
	if ( hipSetDevice(device) != hipSuccess )
	    return -EIO;
	if ( int rc = rec.alloc(halves().nrec, 0, true) )
	    return rc;
	return tails.alloc(halves().tail_bytes, 0, true);
    }
    // what a feed's kernel takes ...
    StreamSides<Rec> sides() const
    {
	const StreamHalves h = halves();
	return StreamSides<Rec>{rec.p + h.rec_in, rec.p + h.rec_out, tails.p + h.tail_in, tails.p + h.tail_out, tail_cap};
    }
    // ... and what the feed does when its launches all went out: otherwise the side it read stays the current one
    void commit() { parity ^= 1u; }

    // behind the feeds queued on `stream`: what follows is there, or read, when its call returns
    int wait( hipStream_t stream ) const { return hipSetDevice(device) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess ? 0 : -EIO; }
    // every stream's record becomes record_at(seen[s]) (seen NULL: of 0): -ENOMEM, -EINVAL for a count
    // above max_seen, -EIO
    template <class RecordAt>
    int seek( const uint64_t *seen, uint64_t max_seen, RecordAt record_at, hipStream_t stream )
    {
	const size_t n = (size_t)nstreams;
	const std::unique_ptr<Rec[]> host(new (std::nothrow) Rec[n]);
	if ( !host )
	    return -ENOMEM;
	for ( size_t s = 0; s < n; s++ ) {
	    if ( seen && seen[s] > max_seen )
		return -EINVAL;
	    host[s] = record_at(seen ? seen[s] : 0u);
	}
	if ( int rc = wait(stream) )
	    return rc;
	return hipMemcpy(rec.p + halves().rec_in, host.get(), n * sizeof(Rec), hipMemcpyHostToDevice) == hipSuccess ? 0 : -EIO;
    }
    // seen_out[s]: what stream s has seen: -ENOMEM, -EIO
    int seen( uint64_t *seen_out, hipStream_t stream ) const
    {
	const size_t n = (size_t)nstreams;
	const std::unique_ptr<Rec[]> host(new (std::nothrow) Rec[n]);
	if ( !host )
	    return -ENOMEM;
	if ( int rc = wait(stream) )
	    return rc;
	if ( hipMemcpy(host.get(), rec.p + halves().rec_in, n * sizeof(Rec), hipMemcpyDeviceToHost) != hipSuccess )
	    return -EIO;
	for ( size_t s = 0; s < n; s++ )
	    seen_out[s] = host[s].seen;
	return 0;
    }
    // before the object goes: no kernel reads the tails any more
    void quiesce() const { (void)hipSetDevice(device), (void)hipDeviceSynchronize(); }
};

} // namespace mifsk
