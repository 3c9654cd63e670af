// mux_stream_check.cpp -- the host logic of a multiplexer stream without a device: H, the tails' room,
// kmax and the capacity rule in 64 bits, the seek limit and a seek's record, and the ladder of what a feed
// refuses (minimodem_amd/csrc/mifsk_mux_stream_check.h), and what it shares with the channelizer's stream
// (mifsk_stream_check.h, stream_shared_check.h) for K rows per stream, under the address and
// undefined-behaviour sanitizers.  The checks call no HIP.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc
//       -fsanitize=address,undefined -o mux_stream_check tools/mux_stream_check.cpp && ./mux_stream_check
//
// Exit status 0 and "mux_stream_check: N checks, 0 failed" when all is well.
// (tests/test_mux_stream_args.py)
#include <cerrno>
#include <cstdint>
#include <cstdio>

#include "mifsk_mux_stream_check.h"
#include "stream_shared_check.h"

static long g_checks = 0, g_failed = 0;

static void expect( uint64_t got, uint64_t want, const char *what, unsigned long long a, unsigned long long b )
{
    g_checks++;
    if ( got != want ) {
	g_failed++;
	std::printf("FAILED %s(%llu, %llu): %llu, expected %llu\n", what, a, b, (unsigned long long)got, (unsigned long long)want);
    }
}

// the largest j with a tap phi + j L < T for some phase phi, one tap step at a time
static uint32_t brute_drain( uint32_t T, uint32_t L )
{
    uint32_t j = 0;
    while ( (uint64_t)( j + 1u ) * L < T )
	j++;
    return j;
}

static uint64_t rc64( int rc ) { return (uint64_t)(int64_t)rc; }

int main()
{
    using namespace mifsk;
    const int no = -EINVAL;

    // H = ceil(T / L) - 1: T < L, T = L, T = q L - 1, q L, q L + 1, and the limits
    const uint32_t Ls[8] = { 1u, 2u, 3u, 40u, 64u, 300u, 4096u, 65535u };
    for ( uint32_t L : Ls ) {
	const uint32_t Ts[12] = { 1u, L > 1u ? L - 1u : 1u, L, L + 1u, 2u * L - 1u, 2u * L, 2u * L + 1u, 7u * L - 1u, 7u * L, 7u * L + 1u,
				  4095u, 4096u };
	for ( uint32_t T : Ts ) {
	    const uint32_t H = mux_stream_drain(T, L);
	    expect(H, brute_drain(T, L), "mux_stream_drain", T, L);
	    expect(H, ( T + L - 1u ) / L - 1u, "ceil(T / L) - 1", T, L);
	    if ( T <= L )
		expect(H, 0, "no tail up to T = L", T, L);
	    // the tails' room: H elements in whole 16-byte vectors, one at least
	    for ( uint32_t esz : { 4u, 8u } ) {
		const uint32_t cap = stream_tail_room(H, esz);
		expect(cap >= H && cap * esz % 16u == 0u && cap * esz >= 16u && cap * esz < H * esz + 16u + ( H == 0u ? 16u : 0u ),
		       1, "stream_tail_room", H, esz);
	    }
	    // the tail samples that exist: min(seen - first, H)
	    const uint64_t firsts[4] = { 0u, 1u, 1ull << 32, kMuxStreamMaxSeen };
	    for ( uint64_t first : firsts ) {
		const uint64_t mores[5] = { 0u, 1u, H ? H - 1u : 0u, H, (uint64_t)H + 1000u };
		for ( uint64_t more : mores ) {
		    const MuxStreamRecord r = { first + more, first };
		    expect(mux_stream_back(H, r), more < H ? more : H, "mux_stream_back", first, more);
		}
		const MuxStreamRecord j = mux_stream_record_at(first);
		expect(j.seen == first && j.first == first && mux_stream_back(H, j) == 0u, 1, "a seek's record", first, H);
	    }
	}
    }
    for ( uint32_t K : { 3u, 65u } )
	stream_shared_checks(expect, sizeof(MuxStreamRecord), K);
    expect(mux_stream_drain(100u, 0u), 0, "no interpolation", 0, 0);
    expect(mux_stream_drain(0u, 4u), 0, "no taps", 0, 0);
    // the seek limit: seen * L below 2^62 for the largest L
    expect(kMuxStreamMaxSeen * 65535ull < ( 1ull << 62 ), 1, "seen L below 2^62", 0, 0);
    expect(( kMuxStreamMaxSeen + 0xFFFFFFFFull ) * 65535ull < ( 1ull << 63 ), 1, "... and a feed behind it", 0, 0);

    // the capacity rule in 64 bits, at the 2^32 edge: kmax L against the room
    expect(mux_stream_fits(0xFFFFFFFFull, 65535u, 0xFFFFFFF8ull), 0, "2^32 x 2^16 does not wrap", 0, 0);
    expect(mux_stream_fits(65537ull, 65535u, 0xFFFFFFF8ull), 0, "65537 x 65535 = 2^32 - 1 + 65536 ... above the room", 0, 0);
    expect(mux_stream_fits(65536ull, 65535u, 0xFFFFFFF8ull), 1, "65536 x 65535 = 2^32 - 65536", 0, 0);
    expect(mux_stream_fits(1ull << 30, 4u, 0xFFFFFFF8ull), 0, "2^30 x 4 = 2^32", 0, 0);
    expect(mux_stream_fits(( 1ull << 30 ) - 2u, 4u, 0xFFFFFFF8ull), 1, "(2^30 - 2) x 4 = 2^32 - 8", 0, 0);
    expect(mux_stream_fits(( 1ull << 30 ) - 1u, 4u, 0xFFFFFFF8ull), 0, "(2^30 - 1) x 4 = 2^32 - 4", 0, 0);
    expect(mux_stream_fits(0u, 65535u, 0u), 1, "nothing new needs no room", 0, 0);

    // what a feed refuses, in the header's order.  Real float32 rows in and out, L = 4, K = 3, two streams.
    alignas(16) static char buf[64];
    static uint32_t counts[6] = { 5u, 9u, 0u, 1u, 2u, 3u };
    const MuxStreamShape sh = { false, false, false, 4u, 3u, 2 }, shiq = { false, false, true, 4u, 3u, 2 };
    mifsk_mux_io good = {};
    good.d_samples = reinterpret_cast<const float *>(buf);
    good.stream_stride = 100u;
    good.nsamples = 98u;			// kmax 98: 392 outputs
    good.nstreams = 2;
    good.d_out = buf;
    good.out_stride = 392u;
    good.nout_cap = 392u;
    good.d_nout = counts;
    expect(rc64(mux_stream_feed_check(sh, &good)), 0, "a good feed", 0, 0);
    expect(stream_kmax(&good), 98, "kmax", 0, 0);
    // each violation alone, then each with every later one: the earlier one's refusal is what comes
    // back (they all return -EINVAL, so the order shows in the code, and here: none passes)
    struct Bad { const char *what; void (*set)( mifsk_mux_io & ); };
    const Bad bad[] = {
	{ "NULL d_samples", []( mifsk_mux_io &io ) { io.d_samples = nullptr; } },
	{ "NULL d_out", []( mifsk_mux_io &io ) { io.d_out = nullptr; } },
	{ "NULL d_nout", []( mifsk_mux_io &io ) { io.d_nout = nullptr; } },
	{ "nstreams 0", []( mifsk_mux_io &io ) { io.nstreams = 0; } },
	{ "input base + 8", []( mifsk_mux_io &io ) { io.d_samples = reinterpret_cast<const float *>(buf + 8); } },
	{ "stride 102", []( mifsk_mux_io &io ) { io.stream_stride = 102u; } },
	{ "output base + 8", []( mifsk_mux_io &io ) { io.d_out = buf + 8; } },
	{ "out_stride 394", []( mifsk_mux_io &io ) { io.out_stride = 394u; } },
	{ "nout_cap above out_stride", []( mifsk_mux_io &io ) { io.nout_cap = 393u; } },
	{ "three streams", []( mifsk_mux_io &io ) { io.nstreams = 3; } },
	{ "out_stride one vector short", []( mifsk_mux_io &io ) { io.out_stride = 388u; io.nout_cap = 388u; } },
	{ "nout_cap one short", []( mifsk_mux_io &io ) { io.nout_cap = 391u; } },
    };
    const int nbad = (int)( sizeof bad / sizeof bad[0] );
    for ( int i = 0; i < nbad; i++ ) {
	for ( int j = i; j < nbad; j++ ) {
	    mifsk_mux_io io = good;
	    bad[j].set(io);
	    bad[i].set(io);
	    expect(rc64(mux_stream_feed_check(sh, &io)), rc64(no), bad[i].what, i, j);
	}
    }
    // the room a feed needs: kmax L, kmax from nsamples without d_nsamples, from the stride with it
    mifsk_mux_io io = good;
    io.nsamples = 101u;						// beyond the stride: the stride counts
    expect(stream_kmax(&io), 100, "kmax beyond the stride", 0, 0);
    expect(rc64(mux_stream_feed_check(sh, &io)), rc64(no), "400 outputs do not fit into 392", 0, 0);
    io.out_stride = io.nout_cap = 400u;
    expect(rc64(mux_stream_feed_check(sh, &io)), 0, "400 outputs fit into 400", 0, 0);
    io = good;
    io.nsamples = 4u;
    io.d_nsamples = counts;					// per-row lengths: any of them may be the stride
    expect(rc64(mux_stream_feed_check(sh, &io)), rc64(no), "the stride bounds per-row lengths", 0, 0);
    io.d_nsamples = nullptr;
    io.out_stride = io.nout_cap = 16u;
    expect(rc64(mux_stream_feed_check(sh, &io)), 0, "four samples need sixteen outputs", 0, 0);
    io.nout_cap = 15u;
    expect(rc64(mux_stream_feed_check(sh, &io)), rc64(no), "... and not fifteen", 0, 0);
    io = good;
    io.nsamples = 0u;
    io.out_stride = 4u;
    io.nout_cap = 0u;
    expect(rc64(mux_stream_feed_check(sh, &io)), 0, "nothing new needs no room", 0, 0);
    // (I, Q) rows in: two elements are 16 bytes
    io = good;
    io.stream_stride = 98u;
    expect(rc64(mux_stream_feed_check(shiq, &io)), 0, "pairs in twos", 0, 0);
    expect(rc64(mux_stream_feed_check(sh, &io)), rc64(no), "floats in fours", 0, 0);
    io.stream_stride = 99u;
    expect(rc64(mux_stream_feed_check(shiq, &io)), rc64(no), "an odd stride of pairs", 0, 0);
    // the output's kind is the plan's: complex PCM16 rows in fours, real PCM16 rows in eights
    const MuxStreamShape s16 = { false, true, false, 4u, 3u, 2 }, cs16 = { true, true, false, 4u, 3u, 2 };
    io = good;
    io.out_stride = io.nout_cap = 396u;
    expect(rc64(mux_stream_feed_check(cs16, &io)), 0, "complex PCM16 in fours", 0, 0);
    expect(rc64(mux_stream_feed_check(s16, &io)), rc64(no), "real PCM16 in eights", 0, 0);
    // the 2^32 edge through the ladder: L = 65535, a stride of 65536 pairs of ... floats
    const MuxStreamShape big = { false, false, false, 65535u, 1u, 1 };
    io = good;
    io.nstreams = 1;
    io.stream_stride = 65540u;
    io.nsamples = 65536u;					// 65536 x 65535 = 2^32 - 65536
    io.out_stride = io.nout_cap = 0xFFFF0000ull;
    expect(rc64(mux_stream_feed_check(big, &io)), 0, "2^32 - 65536 outputs fit", 0, 0);
    io.nsamples = 65537u;					// 2^32 - 1 + ... : beyond any out_stride
    io.out_stride = io.nout_cap = 0xFFFFFFF8ull;
    expect(rc64(mux_stream_feed_check(big, &io)), rc64(no), "kmax L beyond 2^32 is refused, not wrapped", 0, 0);
    // a stride beyond 32 bits: k_s is a uint32_t, so kmax stops at 2^32 - 1
    io = good;
    io.stream_stride = 1ull << 33;
    io.d_nsamples = counts;
    expect(stream_kmax(&io), 0xFFFFFFFFull, "kmax of a huge stride", 0, 0);

    std::printf("mux_stream_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
