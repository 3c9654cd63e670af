// mifsk_session_book.cpp -- the per-stream book of a session (mifsk_session_book.h), for both kinds:
// plan() is every check and every size of a feed that needs no device, commit() the arithmetic
// behind the loop.  Plain C++: tools/session_book.cpp runs it on a CPU.
#include <cerrno>
#include <new>

#include "mifsk_session_book.h"

namespace mifsk {

SessionBook::SessionBook( size_t nstreams, const SessionPolicy &policy )
    : policy_(policy), st_(nstreams, Stream{0, 0u, 0u, false}) {}

int SessionBook::plan( const FeedSource &src, FeedPlan &out ) const
{
    if ( closed_ || ( src.kind != MIFSK_FEED_F32 && src.kind != MIFSK_FEED_S16 ) )
	return -EINVAL;				// (closed: the final piece has been fed)
    try {
	out.rows.resize(st_.size());
    } catch ( const std::bad_alloc & ) {
	return -ENOMEM;
    }
    out.esz = src.kind == MIFSK_FEED_S16 ? sizeof(int16_t) : sizeof(float);
    uint64_t width = 4, off = 0;
    for ( size_t i = 0; i < st_.size(); i++ ) {
	const Stream &h = st_[i];
	uint32_t k = src.nsamples ? src.nsamples[i] : 0u;
	if ( k && ( src.on_device ? ( !src.device || k > src.stride ) : ( !src.host || !src.host[i] ) ) )
	    return -EINVAL;
	if ( policy_.finished_lets_go && h.done )
	    k = 0;				// a finished stream: later samples are ignored
	const uint64_t len = (uint64_t)h.held + k;
	if ( len > policy_.max_row )
	    return -EOVERFLOW;
	width = len > width ? len : width;
	off = ( off + 15 ) & ~15ull;
	out.rows[i] = FeedRow{h.skip, h.held, k, off};
	off += (uint64_t)k * out.esz;
    }
    out.width = ( width + 3 ) & ~3ull;
    out.piece_bytes = ( off + 15 ) & ~15ull;
    out.serial = serial_;
    return 0;
}

bool SessionBook::commit( const FeedPlan &plan, const uint64_t *base, const uint8_t *finished, bool final )
{
    if ( plan.serial != serial_ || plan.rows.size() != st_.size() )
	return false;
    serial_++;
    for ( size_t i = 0; i < st_.size(); i++ ) {
	Stream &h = st_[i];
	h.held = plan.rows[i].keep + plan.rows[i].k;
	h.skip = 0;
	// everything before the cursor has been passed for good
	if ( base[i] > h.origin ) {
	    const uint64_t passed = base[i] - h.origin;
	    h.skip = passed < h.held ? (uint32_t)passed : h.held;
	    h.held -= h.skip;
	    h.origin += h.skip;
	}
	if ( !policy_.passed_stay )
	    h.skip = 0;				// (the caller keeps row[len - held .. len) alone)
	h.done = h.done || finished[i];
	if ( h.done && policy_.finished_lets_go )
	    h.held = h.skip = 0;		// --rx-one, an aborted loop, the final feed: nothing is held
    }
    closed_ = final;
    return true;
}

} // namespace mifsk
