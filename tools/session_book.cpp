// session_book.cpp -- the per-stream book of a session without a device: plan() and commit() of
// minimodem_amd/csrc/mifsk_session_book.cpp under both policies, with a model in the place of the
// receive loop: after each feed a stream's cursor moves to any point of
// [origin, origin + held], both ends included, and any stream may finish at any feed.
//
//   g++ -std=c++17 -Iinclude -Iminimodem_amd/csrc -fsanitize=address,undefined -o session_book
//       tools/session_book.cpp minimodem_amd/csrc/mifsk_session_book.cpp && ./session_book
//
// Prints "session_book: N cases, F failed" (each failed check with a line of its own before it);
// exit status 1 when F > 0.  (tests/test_session_book.py)
#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mifsk_session_book.h"

using namespace mifsk;

static long g_cases = 0, g_failed = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;

#define CHECK(cond, ...) do { if ( !( cond ) ) { if ( g_failed++ < 50 ) { std::printf("FAILED %s: ", #cond); \
	std::printf(__VA_ARGS__); std::printf("\n"); } return; } } while (0)

static uint64_t rnd()		// splitmix64
{
    uint64_t z = ( g_rng += 0x9E3779B97F4A7C15ull );
    z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
    z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull;
    return z ^ ( z >> 31 );
}

// every field of a book
struct Snapshot {
    std::vector<uint64_t>	v;
    explicit Snapshot( const SessionBook &b )
    {
	for ( size_t i = 0; i < b.size(); i++ )
	    v.insert(v.end(), { b.origin(i), b.held(i), b.skip(i), b.done(i) });
	v.push_back(b.closed());
    }
    bool operator==( const Snapshot &o ) const { return v == o.v; }
};

static const int kSome = 1;		// (an address that is there)

// a source of the counts `k`: host pieces, every pointer there, or rows of a device array
static FeedSource source( const std::vector<uint32_t> &k, std::vector<const void *> &ptrs, bool device, unsigned kind )
{
    FeedSource src;
    src.nsamples = k.data();
    src.kind = kind;
    if ( device ) {
	src.on_device = true;
	src.device = &kSome;
	for ( uint32_t v : k )
	    src.stride = v > src.stride ? v : src.stride;
    } else {
	ptrs.assign(k.size(), &kSome);
	src.host = ptrs.data();
    }
    return src;
}

// ---- a random session: the invariants of every plan and every commit, and the refusals at one feed
static void session_case( const SessionPolicy &pol )
{
    g_cases++;
    static const uint32_t kPieces[] = { 0, 1, 3, 4, 5, 4800 };
    const size_t n = 1 + rnd() % 5;
    const int nfeeds = 1 + (int)( rnd() % 10 ), probe = (int)( rnd() % nfeeds );
    SessionBook book(n, pol);
    FeedPlan plan;
    std::vector<uint64_t> fed(n, 0), base(n, 0);
    std::vector<uint8_t> fin(n, 0);
    std::vector<uint32_t> k(n);
    std::vector<const void *> ptrs;
    for ( int f = 0; f < nfeeds; f++ ) {
	const bool final = f == nfeeds - 1, device = pol.finished_lets_go && rnd() % 3 == 0;
	const unsigned kind = pol.finished_lets_go && rnd() % 2 ? MIFSK_FEED_S16 : MIFSK_FEED_F32;
	const uint64_t esz = kind == MIFSK_FEED_S16 ? 2 : 4;
	for ( uint32_t &v : k ) {
	    v = kPieces[rnd() % 6];
	    if ( v == 4800 )
		v = 1000 + (uint32_t)( rnd() % 9000 );
	}
	FeedSource src = source(k, ptrs, device, kind);
	if ( rnd() % 8 == 0 && !device ) {		// nothing new for a stream may be said with NULL too
	    const size_t i = rnd() % n;
	    k[i] = 0;
	    ptrs[i] = nullptr;
	}
	const Snapshot before(book);
	if ( f == probe ) {				// what is refused, and leaves the book as it was
	    std::vector<uint32_t> kk(n, 5);
	    std::vector<const void *> pp;
	    FeedPlan bad;
	    for ( size_t i = 0; i < n; i++ ) {		// a count without its pointer, at every position
		FeedSource s = source(kk, pp, false, MIFSK_FEED_F32);
		pp[i] = nullptr;
		CHECK(book.plan(s, bad) == -EINVAL && Snapshot(book) == before, "stream %zu's pointer is missing", i);
	    }
	    FeedSource s = source(kk, pp, false, MIFSK_FEED_F32);
	    s.host = nullptr;
	    CHECK(book.plan(s, bad) == -EINVAL && Snapshot(book) == before, "no pointers at all");
	    s = source(kk, pp, true, MIFSK_FEED_S16);
	    s.device = nullptr;
	    CHECK(book.plan(s, bad) == -EINVAL && Snapshot(book) == before, "no device array");
	    s = source(kk, pp, true, MIFSK_FEED_F32);
	    s.stride = 4;
	    CHECK(book.plan(s, bad) == -EINVAL && Snapshot(book) == before, "k > stride");
	    s = source(kk, pp, false, 2u);
	    CHECK(book.plan(s, bad) == -EINVAL && Snapshot(book) == before, "an unknown kind");
	    s = source(kk, pp, false, MIFSK_FEED_F32);
	    const size_t big = rnd() % n;		// (a resident stream that is done ignores it)
	    kk[big] = 0xFFFFFFFFu;
	    CHECK(book.plan(s, bad) == ( pol.finished_lets_go && book.done(big) ? 0 : -EOVERFLOW ) && Snapshot(book) == before,
		  "a piece beyond the limit");
	}
	CHECK(book.plan(src, plan) == 0 && Snapshot(book) == before, "feed %d is refused, or its plan changed the book", f);
	uint64_t width = 4, end = 0;
	for ( size_t i = 0; i < n; i++ ) {
	    const FeedRow &r = plan.rows[i];
	    const bool gone = pol.finished_lets_go && book.done(i);
	    CHECK(r.drop == book.skip(i) && r.keep == book.held(i) && r.k == ( gone ? 0u : k[i] ), "stream %zu's row", i);
	    CHECK(!gone || r.keep == 0, "a resident stream that is done holds %u", r.keep);
	    CHECK(r.off % 16 == 0 && r.off >= end, "piece %zu at %" PRIu64 ", the one before ends at %" PRIu64, i, r.off, end);
	    end = r.off + r.k * esz;
	    width = std::max<uint64_t>(width, (uint64_t)r.keep + r.k);
	    fed[i] += r.k;
	}
	CHECK(plan.width % 4 == 0 && plan.width >= width && plan.width < width + 4, "width %" PRIu64 " for rows of %" PRIu64,
	      plan.width, width);
	CHECK(plan.piece_bytes % 16 == 0 && plan.piece_bytes >= end && plan.piece_bytes < end + 16 && plan.esz == esz,
	      "%" PRIu64 " bytes of pieces that end at %" PRIu64, plan.piece_bytes, end);
	// the loop: a cursor anywhere in the row, both ends included; a finished loop stays so and moves no more
	const std::vector<uint64_t> was(base);
	for ( size_t i = 0; i < n; i++ ) {
	    const uint64_t len = (uint64_t)plan.rows[i].keep + plan.rows[i].k;
	    if ( !fin[i] ) {
		const uint64_t to = rnd() % 4 == 0 ? ( rnd() % 2 ? len : 0 ) : rnd() % ( len + 1 );
		base[i] = std::max(base[i], book.origin(i) + to);
		fin[i] = final || rnd() % 12 == 0;
	    }
	}
	CHECK(book.commit(plan, base.data(), fin.data(), final), "feed %d's commit", f);
	const Snapshot after(book);
	CHECK(!book.commit(plan, base.data(), fin.data(), final) && Snapshot(book) == after, "a plan was committed twice");
	CHECK(book.closed() == final, "closed %d after feed %d of %d", book.closed(), f, nfeeds);
	for ( size_t i = 0; i < n; i++ ) {
	    CHECK(base[i] >= was[i] && book.origin(i) >= before.v[4 * i], "stream %zu's cursor or origin went back", i);
	    CHECK(book.done(i) == ( fin[i] != 0 ), "stream %zu: done %d, finished %d", i, book.done(i), fin[i]);
	    if ( pol.finished_lets_go && fin[i] ) {
		CHECK(book.held(i) == 0 && book.skip(i) == 0, "a resident stream that is done holds %u", book.held(i));
		continue;
	    }
	    // nothing fed is lost (a host-tail stream that is done keeps growing), and what the loop passed is gone
	    CHECK(book.origin(i) + book.held(i) == fed[i], "stream %zu: origin %" PRIu64 " + held %u, fed %" PRIu64, i,
		  book.origin(i), book.held(i), fed[i]);
	    CHECK(book.origin(i) == base[i], "stream %zu: origin %" PRIu64 ", cursor %" PRIu64, i, book.origin(i), base[i]);
	    CHECK(book.skip(i) == ( pol.passed_stay ? book.origin(i) - before.v[4 * i] : 0 ), "stream %zu's skip %u", i, book.skip(i));
	}
    }
    for ( uint32_t &v : k )
	v = 0;
    const Snapshot closed(book);
    CHECK(book.plan(source(k, ptrs, false, MIFSK_FEED_F32), plan) == -EINVAL && Snapshot(book) == closed, "a feed after the final one");
}

// ---- rows at the policy's limit: `held` samples are there (fed, the cursor unmoved), `k` come
static void limit_case( const SessionPolicy &pol, uint64_t held, uint64_t k, bool device )
{
    g_cases++;
    SessionBook book(2, pol);
    FeedPlan plan;
    std::vector<const void *> ptrs;
    const std::vector<uint64_t> base(2, 0);
    const std::vector<uint8_t> fin(2, 0);
    std::vector<uint32_t> kk = { 3, (uint32_t)held };
    CHECK(book.plan(source(kk, ptrs, device, MIFSK_FEED_F32), plan) == 0 && book.commit(plan, base.data(), fin.data(), false)
	  && book.held(1) == held, "%" PRIu64 " samples to begin with", held);
    const Snapshot before(book);
    kk[1] = (uint32_t)k;
    const int rc = book.plan(source(kk, ptrs, device, MIFSK_FEED_F32), plan);
    CHECK(Snapshot(book) == before, "a plan changed the book");
    if ( held + k > pol.max_row ) {
	CHECK(rc == -EOVERFLOW, "%" PRIu64 " + %" PRIu64 " over %" PRIu64 ": %d", held, k, pol.max_row, rc);
	return;
    }
    CHECK(rc == 0 && plan.width == ( ( held + k + 3 ) & ~3ull ) && plan.rows[1].off == 16
	  && plan.piece_bytes == ( ( 16 + 4 * k + 15 ) & ~15ull ), "%" PRIu64 " + %" PRIu64 ": %d, width %" PRIu64 ", %" PRIu64 " bytes",
	  held, k, rc, plan.width, plan.piece_bytes);
    CHECK(book.commit(plan, base.data(), fin.data(), false) && book.held(1) == held + k, "held %u", book.held(1));
}

int main()
{
    for ( const SessionPolicy &pol : { kHostTailPolicy, kResidentPolicy } ) {
	for ( int i = 0; i < 20000; i++ )
	    session_case(pol);
	const uint64_t deltas[] = { UINT64_MAX, 0, 1 };		// (-1, 0, +1)
	for ( uint64_t delta : deltas )
	    for ( uint64_t held : { (uint64_t)0, (uint64_t)7, pol.max_row / 2, pol.max_row - 1, pol.max_row } )
		for ( int device = 0; device < 2; device++ )
		    if ( held <= pol.max_row + delta )
			limit_case(pol, held, pol.max_row + delta - held, device != 0);
	// sums that a 32-bit addition would wrap into the limit
	limit_case(pol, pol.max_row, 0xFFFFFFFFu, false);
	limit_case(pol, 0x80000000u, 0x80000004u, true);
    }
    std::printf("session_book: %ld cases, %ld failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
