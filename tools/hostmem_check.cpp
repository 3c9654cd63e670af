// hostmem_check.cpp -- the host-side owners and the output table of libmifsk.so without a device:
// minimodem_amd/csrc/mifsk_hostmem.h, mifsk_outputs.h and mifsk_gather_sets.h over a HIP made of
// malloc() (tools/fake_hip.h), whose N-th allocation can be made to fail.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc -Itools
//       -fsanitize=address,undefined -o hostmem_check tools/hostmem_check.cpp && ./hostmem_check
//
// A leak or a double free is the sanitizer's to report; what a scenario leaves allocated is also
// counted here (g_live).  Exit status 0 and "hostmem_check: N checks, 0 failed" when all is well.
// (tests/test_hostmem.py)
#include <utility>

#include "fake_hip.h"
#include "mifsk_gather_sets.h"
#include "mifsk_hostmem.h"
#include "mifsk_outputs.h"

using namespace mifsk;

// ---- DevMem / PinMem

template <class Mem>
static void owner_scenario()
{
    Mem a;
    CHECK(a.p == nullptr && a.cap == 0);
    int rc = a.fit(100);
    if ( rc ) {
	CHECK(rc == -ENOMEM && a.p == nullptr && a.cap == 0);
    } else {
	CHECK(a.p != nullptr && a.cap == 125);		// 25 % head-room
	auto *was = a.p;
	CHECK(a.fit(125) == 0 && a.p == was && a.cap == 125);	// what is there is enough
	CHECK(a.fit(0) == 0 && a.p == was);
    }
    rc = a.fit(126);					// grows: the old block goes first
    if ( rc )
	CHECK(rc == -ENOMEM && a.p == nullptr && a.cap == 0);
    else
	CHECK(a.p != nullptr && a.cap == 126 + 126 / 4);
    rc = a.fit(3);
    CHECK(rc == 0 ? a.cap >= 3 && a.p != nullptr : a.p == nullptr && a.cap == 0);

    Mem b;
    rc = b.alloc(10, 0, true);				// exact, zero-filled
    if ( rc ) {
	CHECK(rc == -ENOMEM && b.p == nullptr && b.cap == 0);
    } else {
	CHECK(b.cap == 10);
	bool zero = true;
	for ( size_t i = 0; i < 10 * sizeof(*b.p); i++ )
	    zero = zero && ( (const unsigned char *)b.p )[i] == 0;
	CHECK(zero);
    }
    rc = b.alloc(0, 16);				// at least min_bytes
    CHECK(rc == 0 ? b.p != nullptr && b.cap == 16 / sizeof(*b.p) : b.p == nullptr && b.cap == 0);

    // move construction, move assignment over something held, self-assignment, release
    Mem c(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0);
    auto *cp = c.p;
    b = std::move(c);
    CHECK(c.p == nullptr && c.cap == 0 && b.p == cp);
    Mem &self = b;
    b = std::move(self);
    CHECK(b.p == cp);
    auto *raw = b.release();
    CHECK(raw == cp && b.p == nullptr && b.cap == 0);
    if ( raw )
	(void)fake_free(raw);				// (released: the caller's)
    b.reset();
    b.reset();
}

static void stream_scenario()
{
    StreamMem a(nullptr), b(nullptr);
    int rc = a.alloc(0);				// (16 bytes at least: the sanitizer watches the fill)
    CHECK(rc == 0 ? a.p != nullptr : rc == -ENOMEM && a.p == nullptr);
    if ( a.p )
	std::memset(a.p, 0, 16);
    rc = a.alloc(1000);					// again: the first block goes
    CHECK(rc == 0 ? a.p != nullptr : rc == -ENOMEM && a.p == nullptr);
    rc = b.alloc(8);
    void *ap = a.p;
    b = std::move(a);
    CHECK(a.p == nullptr && b.p == ap);
    StreamMem c(std::move(b));
    CHECK(b.p == nullptr && c.p == ap);
    void *raw = c.release();
    CHECK(raw == ap && c.p == nullptr);
    if ( raw )
	(void)fake_free(raw);
}

// ---- the gather's receive sets

static bool rx_empty( const RxSet &s )
{
    return s.bytes.empty() && s.counts.empty() && s.rows.empty() && s.cols == 0 && !s.filled;
}

static bool rx_whole( const RxSet &s, int npeers, int self, const int *rows, int cols )
{
    bool ok = (int)s.bytes.size() == npeers && (int)s.counts.size() == npeers && (int)s.rows.size() == npeers
	   && s.cols == cols && !s.filled;
    for ( int p = 0; ok && p < npeers; p++ ) {
	ok = s.rows[p] == rows[p];
	if ( p == self ) {				// the root's own rows stay where they are
	    ok = ok && s.bytes[p].p == nullptr && s.counts[p].p == nullptr;
	    continue;
	}
	ok = ok && s.bytes[p].p != nullptr && s.counts[p].p != nullptr;
	if ( ok ) {					// (the whole of it is there: the sanitizer watches)
	    std::memset(s.bytes[p].p, 1, (size_t)rows[p] * (size_t)cols);
	    std::memset(s.counts[p].p, 1, (size_t)rows[p] * sizeof(int32_t));
	}
    }
    return ok;
}

// rank 0 of 3, peers 1 and 2 send: the fit fails somewhere (or not), the next start has the same shape
static void gather_scenario()
{
    RxSet s;
    const int rows[3] = { 4, 5, 6 };
    const int rc = fit_rx(s, 3, 0, rows, 0, 7);
    if ( rc ) {
	CHECK(rc == -ENOMEM && rx_empty(s));
	CHECK(g_live == 0);				// (what the half-built set held is gone already)
    }
    g_alloc.fail_at = 0;
    CHECK(fit_rx(s, 3, 0, rows, 0, 7) == 0);		// allocates again after a failure
    CHECK(rx_whole(s, 3, 0, rows, 7));
    // the same shape once more: nothing moves, nothing is allocated
    const uint8_t *was = s.bytes[1].p;
    const long before = g_alloc.n;
    s.filled = true;
    CHECK(fit_rx(s, 3, 0, rows, 0, 7) == 0 && s.bytes[1].p == was && g_alloc.n == before && s.filled);
}

// a slot reused with another shape and back (loopback: one peer, which sends; also no rows at all):
// after every fit the set is whole or empty
static void gather_reuse_scenario()
{
    RxSet s;
    const int shapes[4][2] = { { 8, 16 }, { 24, 40 }, { 0, 3 }, { 8, 16 } };
    for ( const auto &sh : shapes ) {
	const int rc = fit_rx(s, 1, -1, nullptr, sh[0], sh[1]);
	if ( rc ) {
	    CHECK(rc == -ENOMEM && rx_empty(s));
	    CHECK(g_live == 0);
	} else {
	    CHECK(rx_whole(s, 1, -1, &sh[0], sh[1]));
	    s.filled = true;				// (as a gather that went through leaves it)
	}
    }
}

// ---- the table

static const size_t kRowBytes[] = {		// by hand, frames_cap 7 and episodes_cap 3: the table's order
    7 * sizeof(uint8_t), sizeof(uint32_t), 7 * sizeof(uint64_t), 7 * sizeof(mifsk_frame), sizeof(uint32_t),
    3 * sizeof(mifsk_episode), sizeof(uint32_t), sizeof(uint32_t), MIFSK_NCOUNTERS * sizeof(uint64_t), sizeof(int32_t),
};

static mifsk_demod_io fake_io( uintptr_t base )
{
    mifsk_demod_io io;
    std::memset(&io, 0, sizeof(io));
    io.frames_cap = 7;
    io.episodes_cap = 3;
    for ( size_t i = 0; i < kNumOutArrays; i++ )
	out_set(io, kOutArrays[i], (void *)( base + 0x100000 * ( i + 1 ) ));
    return io;
}

static void table_checks()
{
    CHECK(kNumOutArrays == sizeof(kRowBytes) / sizeof(kRowBytes[0]));
    const mifsk_demod_io io = fake_io(0x10000000);
    for ( size_t i = 0; i < kNumOutArrays; i++ )
	CHECK(out_row_bytes(io, kOutArrays[i]) == kRowBytes[i]);

    // outputs_advance: every array by rows x its row, one array at a time and all at once; null stays null
    const size_t rows = 11;
    for ( size_t only = 0; only <= kNumOutArrays; only++ ) {
	mifsk_demod_io a = io;
	if ( only < kNumOutArrays )
	    for ( size_t i = 0; i < kNumOutArrays; i++ )
		if ( i != only )
		    out_set(a, kOutArrays[i], nullptr);
	const mifsk_demod_io before = a;
	outputs_advance(a, rows);
	for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	    const char *was = (const char *)out_get(before, kOutArrays[i]);
	    CHECK(out_get(a, kOutArrays[i]) == ( was ? was + rows * kRowBytes[i] : nullptr ));
	}
	// nothing else of the io moves
	mifsk_demod_io rest = a;
	for ( size_t i = 0; i < kNumOutArrays; i++ )
	    out_set(rest, kOutArrays[i], out_get(before, kOutArrays[i]));
	CHECK(std::memcmp(&rest, &before, sizeof(rest)) == 0);
    }
    {	// the closed forms the time split's rows_of() was written with
	mifsk_demod_io a = io;
	a.d_bytes = nullptr;
	outputs_advance(a, rows);
	CHECK(a.d_frames == io.d_frames + rows * io.frames_cap);
	CHECK(a.d_episodes == io.d_episodes + rows * io.episodes_cap);
	CHECK(a.d_bytes == nullptr);
	mifsk_demod_io b = io;
	outputs_advance(b, rows);
	CHECK(b.d_bytes == io.d_bytes + rows * io.frames_cap);
	CHECK(b.d_bits == io.d_bits + rows * io.frames_cap);
	CHECK(b.d_nframes == io.d_nframes + rows && b.d_nbytes == io.d_nbytes + rows
	      && b.d_nepisodes == io.d_nepisodes + rows && b.d_status == io.d_status + rows);
	CHECK(b.d_counters == io.d_counters + rows * MIFSK_NCOUNTERS && b.d_carrier_band == io.d_carrier_band + rows);
    }

    // outputs_want: counts and status always, the rest by its bit, nothing a pipeline does not hand out
    for ( unsigned bits = 0; bits < 16; bits++ ) {
	const unsigned want = ( bits & 1 ? MIFSK_WANT_BYTES : 0 ) | ( bits & 2 ? MIFSK_WANT_BITS : 0 )
			    | ( bits & 4 ? MIFSK_WANT_FRAMES : 0 ) | ( bits & 8 ? MIFSK_WANT_EPISODES : 0 );
	const mifsk_demod_io w = outputs_want(want, 9, 0);
	CHECK(w.d_nframes && w.d_nbytes && w.d_status && !w.d_counters && !w.d_carrier_band && w.frames_cap == 9);
	CHECK(!w.d_bytes == !( bits & 1 ) && !w.d_bits == !( bits & 2 ) && !w.d_frames == !( bits & 4 ));
	CHECK(!w.d_episodes == !( bits & 8 ) && !w.d_nepisodes == !( bits & 8 ) && w.episodes_cap == ( bits & 8 ? 1u : 0u ));
	CHECK(w.d_samples == nullptr && w.d_nsamples == nullptr && w.nstreams == 0 && w.flags == 0);
    }
    CHECK(outputs_want(MIFSK_WANT_EPISODES, 1, 5).episodes_cap == 5);

    // outputs_assign: the pipeline's ten fields, and nothing else of dst
    const mifsk_demod_io src = fake_io(0x20000000);
    mifsk_demod_io dst;
    std::memset(&dst, 0x5A, sizeof(dst));
    mifsk_demod_io expect = dst;
    expect.d_bytes = src.d_bytes;		expect.d_nbytes = src.d_nbytes;
    expect.d_bits = src.d_bits;			expect.d_frames = src.d_frames;
    expect.d_nframes = src.d_nframes;		expect.frames_cap = src.frames_cap;
    expect.d_episodes = src.d_episodes;		expect.d_nepisodes = src.d_nepisodes;
    expect.episodes_cap = src.episodes_cap;	expect.d_status = src.d_status;
    outputs_assign(dst, src);
    CHECK(std::memcmp(&dst, &expect, sizeof(dst)) == 0);
}

// ---- the mirror

static void mirror_scenario()
{
    mifsk_demod_io want = fake_io(0x30000000);		// (asked whether there, never followed)
    want.d_bits = nullptr;
    want.d_counters = nullptr;
    const size_t nrows = 5;
    OutMirror m;
    const int rc = m.alloc(want, nrows, true);
    CHECK(rc == 0 || rc == -ENOMEM);
    CHECK(m.io.frames_cap == 7 && m.io.episodes_cap == 3 && m.io.d_samples == nullptr && m.io.nstreams == 0);
    CHECK(m.io.d_bits == nullptr && m.io.d_counters == nullptr);
    if ( rc == 0 ) {
	// host arrays of 8 rows; rows [2, 7) come from the mirror's first five
	unsigned char *host[kNumOutArrays] = {};
	mifsk_demod_io ho = want;
	for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	    const OutArray &a = kOutArrays[i];
	    if ( !out_get(want, a) )
		continue;
	    CHECK(out_get(m.io, a) == m.mem[i].p && m.mem[i].p != nullptr);
	    std::memset(m.mem[i].p, (int)( i + 1 ), nrows * kRowBytes[i]);
	    host[i] = (unsigned char *)std::calloc(8, kRowBytes[i]);
	    out_set(ho, a, host[i]);
	}
	ho.d_status = nullptr;				// an array the host lacks is passed over
	uint64_t bytes = 0, expect = 0;
	CHECK(m.copy_out(ho, 2, 7, nullptr, &bytes) == 0);
	for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	    if ( !host[i] )
		continue;
	    const bool copied = out_get(ho, kOutArrays[i]) != nullptr;
	    bool ok = true;
	    for ( size_t j = 0; j < 8 * kRowBytes[i]; j++ ) {
		const bool inside = j >= 2 * kRowBytes[i] && j < 7 * kRowBytes[i];
		ok = ok && host[i][j] == ( copied && inside ? i + 1 : 0 );
	    }
	    CHECK(ok);
	    if ( copied )
		expect += 5 * kRowBytes[i];
	    std::free(host[i]);
	}
	CHECK(bytes == expect);
    }
    const mifsk_demod_io held = m.io, none = {};
    OutMirror n(std::move(m));				// (a lane of a pipeline moves into its vector)
    CHECK(std::memcmp(&m.io, &none, sizeof(none)) == 0 && std::memcmp(&n.io, &held, sizeof(held)) == 0);
    for ( size_t i = 0; i < kNumOutArrays; i++ )	// io points into mem on both sides
	CHECK(m.mem[i].p == nullptr && out_get(n.io, kOutArrays[i]) == n.mem[i].p);
    m = std::move(n);
    CHECK(std::memcmp(&n.io, &none, sizeof(none)) == 0 && std::memcmp(&m.io, &held, sizeof(held)) == 0);
    n = std::move(m);
    n.reset();
    CHECK(n.io.d_bytes == nullptr && n.io.frames_cap == 0);
}

int main()
{
    every_failure(g_alloc, owner_scenario<DevMem<float>>);
    every_failure(g_alloc, owner_scenario<PinMem<uint64_t>>);
    every_failure(g_alloc, owner_scenario<DevMem<uint8_t>>);
    every_failure(g_alloc, stream_scenario);
    every_failure(g_alloc, gather_scenario);
    every_failure(g_alloc, gather_reuse_scenario);
    every_failure(g_alloc, mirror_scenario);
    table_checks();
    CHECK(g_live == 0);
    std::printf("hostmem_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
