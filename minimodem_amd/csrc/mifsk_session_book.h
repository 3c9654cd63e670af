// mifsk_session_book.h -- what a session knows of its streams between the feeds, as integers
// (mifsk_session_book.cpp): where the samples it holds start in the stream, how
// many it holds, how many of them the loop has passed, who is done.  Plain C++, no HIP: the feed
// driver in mifsk_session.cpp and a stand-alone program (tools/session_book.cpp) share it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "mifsk.h"

namespace mifsk {

// Where the two kinds of session differ, set once where the session is made.
struct SessionPolicy {
    uint64_t	max_row;		// the most samples a row may hold: more is -EOVERFLOW
    bool	finished_lets_go;	// a stream whose loop has FINISHED holds nothing and ignores later samples
    bool	passed_stay;		// what the loop passed stays in front of the row until the next feed drops it
};
// (the kernels index rows in 32 bits)
constexpr SessionPolicy kHostTailPolicy = { 0xFFFFFFF0ull, false, false };
constexpr SessionPolicy kResidentPolicy = { 0xFFFFF000ull, true, true };

// Where a feed's new samples are.  The book reads the counts; of the pointers it asks only whether
// they are there.
struct FeedSource {
    const uint32_t	*nsamples = nullptr;	// [n] new samples per stream, or NULL: none
    const void *const	*host = nullptr;	// one host pointer per stream, or ...
    const void		*device = nullptr;	// ... rows of one device array (`on_device`),
    size_t		stride = 0;		//     `stride` elements apart
    bool		on_device = false;
    unsigned		kind = MIFSK_FEED_F32;
};

// A feed's row of stream i: old[drop .. drop + keep) | k new samples | zeros up to the width.
struct FeedRow {
    uint32_t	drop, keep, k;
    uint64_t	off;		// host pieces packed one behind the other: where this one starts (bytes, 16-aligned)
};

struct FeedPlan {
    uint64_t		width = 0;		// samples per row: a multiple of 4, at least 4
    uint64_t		piece_bytes = 0;	// the packed host pieces in all (a multiple of 16)
    size_t		esz = 0;		// bytes per new element
    std::vector<FeedRow>	rows;		// [n]
    uint64_t		serial = 0;		// the state of the book it was made for
};

class SessionBook {
public:
    SessionBook( size_t nstreams, const SessionPolicy &policy );	// (may throw std::bad_alloc)

    // Everything a feed can be refused for without a device -- a feed after the final one, an
    // unknown kind, a count without its pointer, a stride smaller than a count (-EINVAL), a row
    // beyond the policy's limit (-EOVERFLOW), no memory for the plan (-ENOMEM) -- and else the
    // feed's width, rows and pieces.  The book does not change.
    int plan( const FeedSource &src, FeedPlan &out ) const;
    // After the loop has run over the plan's rows: base[i] is stream i's cursor, finished[i] whether
    // its loop is done; `final`: no feed may follow.  What the loop passed leaves the held samples
    // and moves the origin.  Allocates nothing; false, and nothing changes, for a plan that was not
    // made for this state of the book (one committed before, say).
    bool commit( const FeedPlan &plan, const uint64_t *base, const uint8_t *finished, bool final );

    size_t	size() const { return st_.size(); }
    uint64_t	origin( size_t i ) const { return st_[i].origin; }
    uint32_t	held( size_t i ) const { return st_[i].held; }
    uint32_t	skip( size_t i ) const { return st_[i].skip; }
    bool	done( size_t i ) const { return st_[i].done; }
    bool	closed() const { return closed_; }
    const SessionPolicy &policy() const { return policy_; }

private:
    struct Stream {
	uint64_t	origin;		// stream index of the first sample held
	uint32_t	held, skip;	// samples held behind `skip` passed ones at the row's front
	bool		done;
    };
    SessionPolicy	policy_;
    std::vector<Stream>	st_;
    uint64_t		serial_ = 0;
    bool		closed_ = false;
};

} // namespace mifsk
