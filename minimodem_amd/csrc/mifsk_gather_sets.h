// mifsk_gather_sets.h -- the receive and send sets of a gather (mifsk_gather.cpp), apart from RCCL
// so that a host-only program can drive them (tools/hostmem_check.cpp).
#pragma once

#include <vector>

#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"

namespace mifsk {

// one receive set of the root (or the loopback rank): what every peer sent in one gather
struct RxSet {
    std::vector<DevMem<uint8_t>>	bytes;		// [peer] rows[peer] x cols, dense
    std::vector<DevMem<int32_t>>	counts;		// [peer] rows[peer]
    std::vector<int>			rows;
    int					cols = 0;
    bool				filled = false;	// its receives have been enqueued
};

struct TxSet {
    DevMem<uint8_t>	bytes;			// the narrow staging copy
};

// Room in `s` for `rows[p] x cols` (rows == NULL: rows_all x cols) from each of `npeers` peers;
// peer `self` (-1: none) sends nothing: the root's own rows stay where they are.  The new set is
// built apart and takes the old one's place only when every allocation has succeeded: after a
// failure the set is empty, and the next fit allocates again.
inline int fit_rx( RxSet &s, int npeers, int self, const int *rows, int rows_all, int cols )
{
    bool same = s.cols == cols && (int)s.rows.size() == npeers;
    for ( int p = 0; same && p < npeers; p++ )
	same = s.rows[p] == ( rows ? rows[p] : rows_all );
    if ( same )
	return 0;
    // (a set being replaced may still be the target of a receive in flight)
    HIP_OK(hipDeviceSynchronize());
    s = RxSet();
    RxSet fresh;
    fresh.bytes.resize(npeers);
    fresh.counts.resize(npeers);
    fresh.rows.assign(npeers, 0);
    fresh.cols = cols;
    for ( int p = 0; p < npeers; p++ ) {
	const int r = rows ? rows[p] : rows_all;
	fresh.rows[p] = r;
	if ( p == self )
	    continue;
	if ( fresh.bytes[p].alloc((size_t)r * (size_t)cols, 1) || fresh.counts[p].alloc((size_t)r, sizeof(int32_t)) )
	    return -ENOMEM;
    }
    s = std::move(fresh);
    return 0;
}

} // namespace mifsk
