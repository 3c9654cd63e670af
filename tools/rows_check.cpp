// rows_check.cpp -- what the batch entries refuse of a batch of rows, without a device: kind_check,
// out_rows_check, feed_rows_check, rows_in and stream_kmax of minimodem_amd/csrc/mifsk_batch.h with the argument
// ladders of mifsk_impair_batch, mifsk_fm_demod_batch and mifsk_fm_modulate_batch (and the output rows
// of the channelizer and the multiplexer, phase_check_io's).  The checks call no HIP.
//
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Iminimodem_amd/csrc
//       -fsanitize=address,undefined -o rows_check tools/rows_check.cpp && ./rows_check
//
// Exit status 0 and "rows_check: N checks, 0 failed" when all is well.  (tests/test_rows_check.py)
#include <cerrno>
#include <cstdint>
#include <cstdio>

#include "mifsk_batch.h"

static long g_checks = 0, g_failed = 0;

static void expect( int got, int want, const char *what, unsigned long long a, unsigned long long b )
{
    g_checks++;
    if ( got != want ) {
	g_failed++;
	std::printf("FAILED %s(%llu, %llu): %d, expected %d\n", what, a, b, got, want);
    }
}

int main()
{
    using namespace mifsk;
    alignas(16) static char buf[64];
    const void *aligned = buf, *off4 = buf + 4, *off8 = buf + 8;
    const int no = -EINVAL;

    // the kinds
    expect(kind_check(MIFSK_FEED_F32), 0, "kind_check", MIFSK_FEED_F32, 0);
    expect(kind_check(MIFSK_FEED_S16), 0, "kind_check", MIFSK_FEED_S16, 0);
    for ( uint32_t kind : { 2u, 7u, 0x80000000u, 0xFFFFFFFFu } )
	if ( kind != MIFSK_FEED_F32 && kind != MIFSK_FEED_S16 )
	    expect(kind_check(kind), no, "kind_check", kind, 0);

    // elements of 16 bytes
    expect((int)rows_vec(false, false), 4, "rows_vec", 0, 0);
    expect((int)rows_vec(false, true), 8, "rows_vec", 0, 1);
    expect((int)rows_vec(true, false), 2, "rows_vec", 1, 0);
    expect((int)rows_vec(true, true), 4, "rows_vec", 1, 1);

    // output rows: strides 0, 4, 6, 8, 0xFFFFFFF8, 0xFFFFFFFC, 2^32 against vectors of 2, 4 and 8
    // elements and the entries' two limits; [v][i]: what an aligned base gives
    const uint64_t strides[7] = { 0u, 4u, 6u, 8u, 0xFFFFFFF8ull, 0xFFFFFFFCull, 0x100000000ull };
    const uint32_t vecs[3] = { 2u, 4u, 8u };
    //                           0   4   6   8  F8  FC 2^32
    const int below_f8[3][7] = { { no,  0,  0,  0,  0, no, no },	// the modulator's float32 I, Q
				 { no,  0, no,  0,  0, no, no },	// float32 rows; PCM16 I, Q
				 { no, no, no,  0,  0, no, no } };	// PCM16 rows
    const int below_fc[3][7] = { { no,  0,  0,  0,  0,  0, no },
				 { no,  0, no,  0,  0,  0, no },	// the channelizer's rows
				 { no, no, no,  0,  0, no, no } };
    for ( int v = 0; v < 3; v++ ) {
	for ( int i = 0; i < 7; i++ ) {
	    expect(out_rows_check(aligned, strides[i], vecs[v], 0xFFFFFFF8ull), below_f8[v][i], "out_rows_check F8", strides[i], vecs[v]);
	    expect(out_rows_check(aligned, strides[i], vecs[v], 0xFFFFFFFCull), below_fc[v][i], "out_rows_check FC", strides[i], vecs[v]);
	    // a base that is not on 16 bytes is refused whatever the stride
	    expect(out_rows_check(off4, strides[i], vecs[v], 0xFFFFFFF8ull), no, "out_rows_check +4", strides[i], vecs[v]);
	    expect(out_rows_check(off8, strides[i], vecs[v], 0xFFFFFFFCull), no, "out_rows_check +8", strides[i], vecs[v]);
	    expect(out_rows_check(nullptr, strides[i], vecs[v], 0xFFFFFFF8ull), below_f8[v][i], "out_rows_check NULL", strides[i], vecs[v]);
	}
    }

    // the entries' ladders, output side: impair (either kind), the discriminator (float32), the
    // modulator (I, Q of either kind)
    expect(out_rows_check(aligned, 8u, rows_vec(false, false), 0xFFFFFFF8ull), 0, "impair f32", 8, 0);
    expect(out_rows_check(aligned, 4u, rows_vec(false, true), 0xFFFFFFF8ull), no, "impair s16", 4, 0);
    expect(out_rows_check(aligned, 6u, 4u, 0xFFFFFFF8ull), no, "fm_demod", 6, 0);
    expect(out_rows_check(aligned, 6u, rows_vec(true, false), 0xFFFFFFF8ull), 0, "fm_modulate f32", 6, 0);
    expect(out_rows_check(aligned, 6u, rows_vec(true, true), 0xFFFFFFF8ull), no, "fm_modulate s16", 6, 0);

    // input side: a feed of real rows (impair, the survey, soft bits) and the discriminator's I, Q rows
    expect(feed_rows_check(MIFSK_FEED_F32, 0.0f, aligned, 4u), 0, "feed f32", 4, 0);
    expect(feed_rows_check(MIFSK_FEED_F32, 0.0f, aligned, 6u), no, "feed f32", 6, 0);
    expect(feed_rows_check(MIFSK_FEED_F32, 0.5f, aligned, 4u), no, "feed f32 rxnoise", 4, 0);
    expect(feed_rows_check(MIFSK_FEED_S16, 0.5f, aligned, 8u), 0, "feed s16 rxnoise", 8, 0);
    expect(feed_rows_check(MIFSK_FEED_S16, 0.0f, aligned, 4u), no, "feed s16", 4, 0);
    expect(feed_rows_check(MIFSK_FEED_S16, 0.0f, off8, 8u), no, "feed s16 +8", 8, 0);
    expect(feed_rows_check(7u, 0.0f, aligned, 8u), no, "feed kind 7", 8, 0);
    expect(rows_aligned(aligned, 0xFFFFFFFCull, rows_vec(true, false)) ? 0 : no, 0, "fm_demod rows", 0xFFFFFFFCull, 2);
    expect(rows_aligned(off4, 8u, rows_vec(true, true)) ? 0 : no, no, "fm_demod rows +4", 8, 4);

    // the rows of an io, field by field
    static_assert(sizeof(RowsIn) == 28, "RowsIn");
    uint32_t counts[3] = { 0u, 5u, 64u };
    mifsk_impair_io io = {};
    io.d_samples = aligned;
    io.stream_stride = 64u;
    io.d_nsamples = counts;
    io.nsamples = 60u;
    io.nstreams = 3;
    const RowsIn in = rows_in(&io);
    expect(in.x == aligned && in.stride == 64u && in.nsamples_v == counts && in.nsamples_u == 60u ? 0 : no, 0, "rows_in", 0, 0);
    const mifsk_fm_mod_io none = {};
    const RowsIn zero = rows_in(&none);
    expect(!zero.x && zero.stride == 0u && !zero.nsamples_v && zero.nsamples_u == 0u ? 0 : no, 0, "rows_in {}", 0, 0);

    // the most one call gives a row of it: nsamples up to the stride, the stride with per-row lengths
    // (any of them may reach it), and never more than a uint32_t holds
    expect(stream_kmax(&none) == 0u ? 0 : no, 0, "kmax {}", 0, 0);
    for ( uint64_t stride : { 64ull, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull, 1ull << 33 } ) {
	const uint64_t most = stride < 0xFFFFFFFFull ? stride : 0xFFFFFFFFull;
	io.stream_stride = stride;
	for ( uint32_t n : { 0u, 1u, 60u, 64u, 65u, 0xFFFFFFFFu } ) {
	    io.nsamples = n;
	    io.d_nsamples = nullptr;
	    expect(stream_kmax(&io) == ( n < most ? n : most ) ? 0 : no, 0, "kmax of nsamples", stride, n);
	    io.d_nsamples = counts;
	    expect(stream_kmax(&io) == most ? 0 : no, 0, "kmax with per-row lengths", stride, n);
	}
    }

    std::printf("rows_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
