// channel_stream_check.cpp -- the host logic of a channel stream without a device: the counting of
// outputs, the records and tails, and the ladder of what a feed refuses
// (minimodem_amd/csrc/mifsk_channel_stream_check.h), and what it shares with the multiplexer's stream
// (mifsk_stream_check.h, stream_shared_check.h) for one row per stream, under the address and
// undefined-behaviour sanitizers.  The checks call no HIP.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc
//       -fsanitize=address,undefined -o channel_stream_check tools/channel_stream_check.cpp && ./channel_stream_check
//
// Exit status 0 and "channel_stream_check: N checks, 0 failed" when all is well.
// (tests/test_channel_stream_args.py)
#include <cerrno>
#include <cstdint>
#include <cstdio>

#include "mifsk_channel_stream_check.h"
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

// the outputs whose last element, m D + T - 1, is one of elements seen .. seen + k, one by one
static uint64_t brute( uint32_t T, uint32_t D, uint64_t seen, uint64_t k )
{
    uint64_t m = seen > (uint64_t)T + D ? ( seen - T ) / D - 1u : 0u, count = 0;
    for ( ; m * D + T - 1u < seen + k; m++ )
	count += m * D + T - 1u >= seen;
    return count;
}

int main()
{
    using namespace mifsk;
    const int no = -EINVAL;
    const uint32_t Ts[6] = { 1u, 2u, 63u, 64u, 65u, 385u };

    // counting, and the tail's bound, at small and very large indices
    for ( uint32_t T : Ts ) {
	const uint32_t Ds[7] = { 1u, 3u, 4u, 7u, T, T + 5u, 2u * T + 3u };
	for ( uint32_t D : Ds ) {
	    const uint64_t seens[8] = { 0u, 1u, T - 1u, T, (uint64_t)T + D - 1u, 0xFFFFFFFFull, 1ull << 32, 1ull << 63 };
	    const uint64_t ks[6] = { 0u, 1u, D - 1u, D, T, 1000u };
	    for ( uint64_t seen : seens ) {
		for ( uint64_t k : ks ) {
		    expect(stream_outputs(T, D, seen, k), brute(T, D, seen, k), "stream_outputs", seen, k);
		    expect(stream_outputs(T, D, seen, k) <= ( k + D - 1u ) / D, 1, "at most ceil(k / D)", seen, k);
		}
		// a stream in flight, and one joined at `seen`
		const StreamRecord flight = { seen, stream_outputs_of(T, D, seen) }, joined = stream_record_at(D, seen);
		expect(stream_tail_len(D, flight) <= T - 1u, 1, "tail <= T - 1", seen, D);
		expect(stream_tail_len(D, joined), 0, "no tail behind a seek", seen, D);
		expect(joined.next >= flight.next && joined.next * D >= seen && ( joined.next == 0u || ( joined.next - 1u ) * D < seen ),
		       1, "a seek's first output", seen, D);
	    }
	    // the sum over a cut is the whole, whatever the cut
	    uint64_t seen = 0, sum = 0, x = 88172645463325252ull;
	    for ( int i = 0; i < 200; i++ ) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;		// xorshift64
		const uint64_t k = x % ( 3u * T + 2u * D );
		sum += stream_outputs(T, D, seen, k);
		seen += k;
		expect(sum, stream_outputs_of(T, D, seen), "sum over the cut", seen, k);
	    }
	}
	// the tail's room: T - 1 elements in whole 16-byte vectors, one at least
	for ( uint32_t esz : { 2u, 4u, 8u } ) {
	    const uint32_t cap = stream_tail_room(T - 1u, esz);
	    expect(cap >= T - 1u && cap * esz % 16u == 0u && cap * esz >= 16u && cap * esz < ( T - 1u ) * esz + 16u + ( T == 1u ? 16u : 0u ),
		   1, "stream_tail_room", T, esz);
	}
    }
    stream_shared_checks(expect, sizeof(StreamRecord), 1u);
    expect(stream_outputs(0u, 4u, 100u, 100u), 0, "no taps", 0, 0);
    expect(stream_outputs(4u, 0u, 100u, 100u), 0, "no decimation", 0, 0);
    expect(stream_outputs(4u, 1u, ~0ull - 5u, 100u), 5, "a sum beyond 2^64 counts to 2^64 - 1", 0, 0);

    // what a feed refuses, in the header's order.  Real float32 rows, D = 4, K = 3, two streams.
    alignas(16) static char buf[64];
    static uint32_t counts[2] = { 5u, 9u };
    const StreamShape sh = { false, false, 4u, 3u, 2 };
    mifsk_channel_io good = {};
    good.d_samples = buf;
    good.stream_stride = 400u;
    good.nsamples = 398u;			// kmax 398: 100 outputs at most
    good.nstreams = 2;
    good.d_rows = reinterpret_cast<float *>(buf);
    good.out_stride = 100u;
    good.nout_cap = 100u;
    good.d_nout = counts;
    expect(stream_feed_check(sh, &good, 0u), 0, "a good feed", 0, 0);
    expect(stream_feed_check(sh, &good, MIFSK_CHANNEL_STREAM_IQ), 0, "a good I/Q feed", 0, 0);
    expect(stream_kmax(&good), 398, "kmax", 0, 0);
    // each violation alone, then each with every later one: the earlier one's refusal is what comes
    // back (they all return -EINVAL, so the order shows in the code, and here: none passes)
    struct Bad { const char *what; void (*set)( mifsk_channel_io &, uint32_t & ); };
    const Bad bad[] = {
	{ "NULL d_nout", []( mifsk_channel_io &io, uint32_t & ) { io.d_nout = nullptr; } },
	{ "nstreams 0", []( mifsk_channel_io &io, uint32_t & ) { io.nstreams = 0; } },
	{ "input base + 8", []( mifsk_channel_io &io, uint32_t & ) { io.d_samples = buf + 8; } },
	{ "stride 402", []( mifsk_channel_io &io, uint32_t & ) { io.stream_stride = 402u; } },
	{ "output base + 8", []( mifsk_channel_io &io, uint32_t & ) { io.d_rows = reinterpret_cast<float *>(buf + 8); } },
	{ "out_stride 102", []( mifsk_channel_io &io, uint32_t & ) { io.out_stride = 102u; } },
	{ "nout_cap above out_stride", []( mifsk_channel_io &io, uint32_t & ) { io.nout_cap = 101u; } },
	{ "three streams", []( mifsk_channel_io &io, uint32_t & ) { io.nstreams = 3; } },
	{ "flag 2", []( mifsk_channel_io &, uint32_t &flags ) { flags |= 2u; } },
	{ "flag 2^31", []( mifsk_channel_io &, uint32_t &flags ) { flags |= 0x80000000u; } },
	{ "out_stride one vector short", []( mifsk_channel_io &io, uint32_t & ) { io.out_stride = 96u; io.nout_cap = 96u; } },
	{ "nout_cap one short", []( mifsk_channel_io &io, uint32_t & ) { io.nout_cap = 99u; } },
    };
    const int nbad = (int)( sizeof bad / sizeof bad[0] );
    for ( int i = 0; i < nbad; i++ ) {
	for ( int j = i; j < nbad; j++ ) {
	    mifsk_channel_io io = good;
	    uint32_t flags = 0u;
	    bad[j].set(io, flags);
	    bad[i].set(io, flags);
	    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, flags), (uint64_t)(int64_t)no, bad[i].what, i, j);
	}
    }
    // the room a feed needs: ceil(kmax / D), kmax from nsamples without d_nsamples, from the stride with it
    mifsk_channel_io io = good;
    io.nsamples = 401u;					// beyond the stride: the stride counts
    expect(stream_kmax(&io), 400, "kmax beyond the stride", 0, 0);
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, 0u), 0, "100 outputs fit", 0, 0);
    io = good;
    io.nsamples = 4u;
    io.d_nsamples = counts;					// per-row lengths: any of them may be the stride
    io.out_stride = io.nout_cap = 96u;
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, 0u), (uint64_t)(int64_t)no, "the stride bounds per-row lengths", 0, 0);
    io.d_nsamples = nullptr;
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, 0u), 0, "one output needs little room", 0, 0);
    io = good;
    io.nsamples = 0u;
    io.out_stride = 4u;
    io.nout_cap = 0u;
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, 0u), 0, "nothing new needs no room", 0, 0);
    // pairs: out_stride % 2, up to 2^31 - 2
    io = good;
    io.out_stride = 102u;
    io.nout_cap = 100u;
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, MIFSK_CHANNEL_STREAM_IQ), 0, "pairs in twos", 0, 0);
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, 0u), (uint64_t)(int64_t)no, "floats in fours", 0, 0);
    io.out_stride = 0x80000000ull;
    expect((uint64_t)(int64_t)stream_feed_check(sh, &io, MIFSK_CHANNEL_STREAM_IQ), (uint64_t)(int64_t)no, "pairs above 2^31 - 2", 0, 0);
    // a stride beyond 32 bits: k_s is a uint32_t, so kmax stops at 2^32 - 1
    io = good;
    io.stream_stride = 1ull << 33;
    io.d_nsamples = counts;
    expect(stream_kmax(&io), 0xFFFFFFFFull, "kmax of a huge stride", 0, 0);

    std::printf("channel_stream_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
