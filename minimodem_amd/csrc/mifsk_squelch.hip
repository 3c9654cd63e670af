// mifsk_squelch.hip -- the FM stage's power squelch (include/mifsk/squelch.h): mifsk_fm_squelch_batch and
// the host helper mifsk_fm_squelch_level.
//
// A sample's energy is an INTEGER (40 fractional bits), so a window's sum does not depend on the order
// of its additions: the device adds it in a tree, tile by tile, and a host adds it in a loop.  Three
// launches, the modulator's shape (mifsk_fm.hip):
//   1. squelch_energy_kernel: a workgroup owns a tile of a row (256 threads x 8 complex samples, loaded
//      as whole 16-byte vectors) and sums it per window: the runs of equal window index inside a
//      thread, then across the wave (a segmented scan: window indices only grow along a row, so "same
//      index" is the segment), then across the four waves through 64 bytes of LDS.  A window that lies
//      inside the tile is finished here and goes to scratch [row][window]; the tile's first and last
//      window may cross its edge and go to scratch [row][tile][2] as pieces.  A tile behind the row's
//      length loads nothing and stores nothing.
//   2. squelch_gate_kernel: one wave per row takes the row's windows 64 at a time: a lane joins the
//      pieces of its window (and the state's acc into the first), the gate comes from three ballots
//      (windows at or above open_level, low windows, low windows that complete a run of hang + 1), and
//      the lanes store energies, gates, spans, counts and the new state.
//   3. squelch_mute_kernel, with d_audio only: a thread owns four floats of the audio row and stores
//      zeros where the gate of that moment is closed: one 16-byte vector, or scalars at a ragged end.
// No workgroup waits for another inside a kernel: the order is the stream's.  What a launch hands to
// the next lies in stream-ordered scratch, never in the caller's arrays: nothing a kernel wrote there
// is read back.  The outputs are plain vector stores.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>

#include "mifsk.h"
#include "mifsk/squelch.h"
#include "mifsk_batch.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"
#include "mifsk_rows.h"

namespace mifsk {

constexpr uint32_t kSqThreads = 256u;
constexpr uint32_t kSqWaves = kSqThreads / 64u;
constexpr uint32_t kSqPer = 8u;					// the energy launch's samples per thread
constexpr uint32_t kSqTile = kSqThreads * kSqPer;		// ... and per workgroup
constexpr uint32_t kSqMutePer = 4u;				// the mute launch's floats per thread

struct SquelchArgs {
    RowsIn		in;		// interleaved I, Q: complex elements
    uint32_t		s0;		// first row of this launch
    uint32_t		nrows;		// all rows (the gate launch)
    uint32_t		ntiles;		// tiles of a row: up to kmax
    uint32_t		B, hang, span_cap;
    uint64_t		wcap;		// windows a call completes in a row at most: kmax / B + 1
    uint64_t		open_level, close_level;
    const mifsk_fm_squelch_state	*state;		// [nrows] or NULL
    mifsk_fm_squelch_state		*state_out;	// [nrows] or NULL
    uint64_t		*energy;	// [nrows][win_stride] or NULL
    uint8_t		*gate;		// [nrows][win_stride] or NULL
    size_t		win_stride;
    uint32_t		*nwindows;
    mifsk_fm_squelch_span	*spans;	// [nrows][span_cap] or NULL
    uint32_t		*nspans;	// [nrows] or NULL
    float		*audio;		// [nrows][audio_stride] or NULL
    size_t		audio_stride;
    // scratch
    uint64_t		*pieces;	// [nrows][ntiles][2]: the sums of a tile's first and last window
    uint64_t		*inner;		// [nrows][wcap]: the sums of the windows inside a tile
    uint8_t		*applied;	// [nrows][wcap + 1]: the gate over the samples of the call's window j (with d_audio)
    uint32_t		*rem;		// [nrows]: seen mod B before the call (with d_audio)
};

// the energy of one sample.  p * 2^40 is below 2^48: adding 2^52 rounds it to an integer, ties to even,
// and leaves that integer in the low bits of the mantissa, which is (uint64_t)rint(p * 2^40)
__device__ __forceinline__ uint64_t sq_energy( float i, float q )
{
    const double a = (double)i, b = (double)q;
    const double p = fma(a, a, b * b);
    const double m = p * 0x1p40 + 0x1p52;
    return p < 256.0 ? (uint64_t)__double_as_longlong(m) & 0xFFFFFFFFFFFFFull : 1ull << 48;
}

// ---------------------------------------------------------------------------
// 1. the windows' sums, tile by tile
// ---------------------------------------------------------------------------
template <bool S16>
__global__ __launch_bounds__(256)
void squelch_energy_kernel( const SquelchArgs A )
{
    __shared__ uint64_t wave_run[kSqWaves];
    __shared__ uint32_t wave_first[kSqWaves], wave_last[kSqWaves];
    const uint32_t s = A.s0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * kSqTile, W = A.in.len(s);
    if ( t0 >= W )
	return;							// (the whole workgroup)
    const uint32_t B = A.B;
    // the tile's first element is element rt of the call's window jbase
    const uint64_t x = ( A.state ? A.state[s].seen : 0ull ) % B + t0;
    const uint64_t jbase = x / B;
    const uint32_t rt = (uint32_t)( x % B );
    const uint32_t nv = W - t0 < kSqTile ? (uint32_t)( W - t0 ) : kSqTile;
    const uint32_t klast = ( rt + nv - 1u ) / B;		// the tile's windows are 0 .. klast
    const uint32_t p0 = tid * kSqPer;
    const uint64_t i0 = t0 + p0;

    // the samples: whole 16-byte vectors that begin inside the row's length, and with it inside its
    // stride (a multiple of the vector); e = 0 from W on
    uint64_t e[kSqPer];
    if constexpr ( S16 ) {
	const int16_t *row = reinterpret_cast<const int16_t *>(A.in.x) + ( (size_t)s * A.in.stride + i0 ) * 2u;
#pragma unroll
	for ( uint32_t h = 0; h < kSqPer; h += 4u ) {
	    S16x8 p = {};
	    if ( i0 + h < W )
		p = *reinterpret_cast<const S16x8 *>(row + 2u * h);
#pragma unroll
	    for ( uint32_t u = 0; u < 4u; u++ )
		e[h + u] = i0 + h + u < W ? sq_energy(rows_f32(p.v[2u * u]), rows_f32(p.v[2u * u + 1u])) : 0ull;
	}
    } else {
	const float *row = reinterpret_cast<const float *>(A.in.x) + ( (size_t)s * A.in.stride + i0 ) * 2u;
#pragma unroll
	for ( uint32_t h = 0; h < kSqPer; h += 2u ) {
	    float4 p = float4{0.0f, 0.0f, 0.0f, 0.0f};
	    if ( i0 + h < W )
		p = *reinterpret_cast<const float4 *>(row + 2u * h);
	    e[h] = i0 + h < W ? sq_energy(p.x, p.y) : 0ull;
	    e[h + 1u] = i0 + h + 1u < W ? sq_energy(p.z, p.w) : 0ull;
	}
    }

    // key[u]: the window of the thread's element u, key[kSqPer] of the next thread's first; elements
    // from W on count (as zeros) to the last window
    uint32_t key[kSqPer + 1u];
    {
	uint32_t q = ( rt + p0 ) / B, r = ( rt + p0 ) % B;
#pragma unroll
	for ( uint32_t u = 0; u <= kSqPer; u++ ) {
	    key[u] = q < klast ? q : klast;
	    if ( ++r == B ) {
		r = 0u;
		q++;
	    }
	}
    }
    // the runs inside the thread: e[u] becomes the sum of its run up to u
#pragma unroll
    for ( uint32_t u = 1; u < kSqPer; u++ )
	if ( key[u] == key[u - 1u] )
	    e[u] += e[u - 1u];
    const uint32_t kf = key[0], kl = key[kSqPer - 1u];
    // across the wave: run = the sum of the lanes up to this one whose last window is this one's.  The
    // windows only grow along the row, so a lane d below with another window has none of this one's
    // below it either.
    uint64_t run = e[kSqPer - 1u];
#pragma unroll
    for ( uint32_t d = 1u; d < 64u; d <<= 1 ) {
	const uint64_t up = (uint64_t)__shfl_up((unsigned long long)run, d, 64);
	const uint32_t up_key = (uint32_t)__shfl_up((int)kl, d, 64);
	if ( lane >= d && up_key == kl )
	    run += up;
    }
    // what the lanes and the waves before this thread hold of its first window
    const uint64_t below = (uint64_t)__shfl_up((unsigned long long)run, 1u, 64);
    const uint32_t below_key = (uint32_t)__shfl_up((int)kl, 1u, 64);
    uint64_t carry = lane > 0u && below_key == kf ? below : 0ull;
    if ( lane == 63u ) {
	wave_run[wave] = run;
	wave_last[wave] = kl;
    }
    if ( lane == 0u )
	wave_first[wave] = kf;
    __syncthreads();
    if ( kf == wave_first[wave] )				// the thread's first window reaches the wave's start
	for ( uint32_t w = 0; w < wave; w++ )
	    if ( wave_last[w] == kf )
		carry += wave_run[w];
    // the element that ends a window's run in the tile stores the window's sum
    uint64_t *pieces = A.pieces + ( (size_t)s * A.ntiles + blockIdx.x ) * 2u;
    uint64_t *inner = A.inner + (size_t)s * A.wcap + jbase;
#pragma unroll
    for ( uint32_t u = 0; u < kSqPer; u++ ) {
	const bool ends = key[u + 1u] != key[u] || ( u == kSqPer - 1u && tid == kSqThreads - 1u );
	if ( ends ) {
	    const uint32_t k = key[u];
	    const uint64_t sum = e[u] + ( k == kf ? carry : 0ull );
	    if ( k == 0u )
		pieces[0] = sum;
	    else if ( k == klast )
		pieces[1] = sum;
	    else
		inner[k] = sum;					// (jbase + k is below the row's count of windows)
	}
    }
}

// ---------------------------------------------------------------------------
// 2. one wave per row: the windows' energies, the gate, the spans, the state
// ---------------------------------------------------------------------------
// the sum over the call's elements [lo, hi) of row s (lo < hi <= W), which are those of its window j
__device__ __forceinline__ uint64_t sq_join( const SquelchArgs &A, uint32_t s, uint64_t j, uint64_t lo, uint64_t hi, uint64_t W )
{
    const uint64_t *pieces = A.pieces + (size_t)s * A.ntiles * 2u;
    uint64_t E = 0ull;
    for ( uint64_t t = lo / kSqTile; t <= ( hi - 1u ) / kSqTile; t++ ) {
	const uint64_t a = t * kSqTile, b = a + kSqTile < W ? a + kSqTile : W;	// the tile's elements [a, b)
	if ( lo <= a )
	    E += pieces[2u * t];					// the tile's first window
	else if ( hi >= b )
	    E += pieces[2u * t + 1u];					// its last
	else
	    E += A.inner[(size_t)s * A.wcap + j];			// inside it
    }
    return E;
}

__global__ __launch_bounds__(256)
void squelch_gate_kernel( const SquelchArgs A )
{
    const uint32_t s = blockIdx.x * kSqWaves + ( threadIdx.x >> 6 ), lane = threadIdx.x & 63u;
    if ( s >= A.nrows )
	return;							// (whole waves)
    const uint64_t W = A.in.len(s);
    mifsk_fm_squelch_state st = {};
    if ( A.state )
	st = A.state[s];
    const uint32_t B = A.B;
    const uint64_t w0 = st.seen / B, r0 = st.seen % B;
    const uint64_t nw = ( r0 + W ) / B;				// windows completed: 2^32 - 1 at most
    const bool open_in = st.open != 0u;
    const uint64_t need = (uint64_t)A.hang + 1ull;		// low windows in a row that close the gate
    bool open = open_in;					// the gate, the run of low windows behind it and
    uint64_t low = open ? (uint64_t)st.low : 0ull;		// ... the count of spans before the round
    uint64_t span_first = st.span_first;
    uint32_t nspans = 0u;
    uint8_t *applied = A.applied ? A.applied + (size_t)s * ( A.wcap + 1u ) : nullptr;
    mifsk_fm_squelch_span *spans = A.spans ? A.spans + (size_t)s * A.span_cap : nullptr;
    if ( applied && lane == 0u )
	applied[0] = (uint8_t)open_in;
    const uint64_t upto = ( 2ull << lane ) - 1ull, under = ( 1ull << lane ) - 1ull;	// lanes <= and < this one

    for ( uint64_t j0 = 0; j0 < nw; j0 += 64u ) {
	const uint64_t j = j0 + lane;
	const bool valid = j < nw;
	uint64_t E = 0ull;
	if ( valid ) {
	    const uint64_t lo = j == 0u ? 0ull : j * B - r0, hi = ( j + 1u ) * B - r0;
	    E = sq_join(A, s, j, lo, hi, W) + ( j == 0u ? st.acc : 0ull );
	}
	const bool is_high = valid && E >= A.open_level, is_low = valid && E < A.close_level;
	const uint64_t m_high = __ballot(is_high), m_other = __ballot(!is_low);
	// the run of low windows that ends here: back to the last window that is not low, or into `low`
	const uint64_t stop = m_other & upto;
	const uint64_t run = !is_low ? 0ull : stop ? (uint64_t)( lane - ( 63u - (uint32_t)__clzll((long long)stop) ) )
						   : low + lane + 1ull;
	const uint64_t m_close = __ballot(is_low && run >= need);
	// open: the last high window lies behind the last closing one; with neither, as before the round
	const uint64_t mh = m_high & upto, mc = m_close & upto;
	const bool g = mh > mc || ( ( mh | mc ) == 0ull && open );
	const uint64_t m_gate = __ballot(g);
	// spans: a run of open windows begins where the window before was closed (before the call's first
	// window: by definition) and ends in front of the first closed one
	const bool before = lane == 0u ? ( j0 != 0u && open ) : ( ( m_gate >> ( lane - 1u ) ) & 1ull ) != 0ull;
	const bool starts = valid && g && !before, ends = valid && !g && before;
	const uint64_t m_start = __ballot(starts);
	const uint32_t idx = nspans + (uint32_t)__popcll(m_start & under);	// runs begun before this window
	if ( spans && starts && idx < A.span_cap )
	    spans[idx].first_window = j == 0u && open_in ? st.span_first : w0 + j;
	if ( spans && ends && idx - 1u < A.span_cap )
	    spans[idx - 1u].end_window = w0 + j;
	if ( valid ) {
	    if ( A.energy )
		A.energy[(size_t)s * A.win_stride + j] = E;
	    if ( A.gate )
		A.gate[(size_t)s * A.win_stride + j] = (uint8_t)g;
	    if ( applied )
		applied[j + 1u] = (uint8_t)g;
	}
	// the round's last window hands on
	if ( m_start ) {
	    const uint64_t jl = j0 + ( 63u - (uint32_t)__clzll((long long)m_start) );
	    if ( !( jl == 0u && open_in ) )			// (the gate went from closed to open)
		span_first = w0 + jl;
	}
	nspans += (uint32_t)__popcll(m_start);
	const uint32_t last = nw - j0 < 64u ? (uint32_t)( nw - j0 ) - 1u : 63u;
	open = ( ( m_gate >> last ) & 1ull ) != 0ull;
	low = (uint64_t)__shfl((unsigned long long)run, (int)last, 64);
    }

    if ( lane == 0u ) {
	// the window that is not yet complete
	const uint64_t lo = nw == 0u ? 0ull : nw * B - r0;
	uint64_t acc = nw == 0u ? st.acc : 0ull;
	if ( lo < W )
	    acc += sq_join(A, s, nw, lo, W, W);
	A.nwindows[s] = (uint32_t)nw;
	if ( A.nspans )
	    A.nspans[s] = nspans;
	if ( spans && open && nspans != 0u && nspans - 1u < A.span_cap )
	    spans[nspans - 1u].end_window = w0 + nw;		// still open
	if ( A.state_out ) {
	    mifsk_fm_squelch_state out;
	    out.seen = st.seen + W;
	    out.acc = acc;
	    out.span_first = span_first;
	    out.open = open ? 1u : 0u;
	    out.low = open ? (uint32_t)low : 0u;
	    A.state_out[s] = out;
	}
	if ( A.rem )
	    A.rem[s] = (uint32_t)r0;
    }
}

// ---------------------------------------------------------------------------
// 3. zeros over the audio where the gate of that moment is closed
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void squelch_mute_kernel( const SquelchArgs A )
{
    const uint32_t s = A.s0 + blockIdx.y;
    const uint64_t i0 = ( (uint64_t)blockIdx.x * kSqThreads + threadIdx.x ) * kSqMutePer, W = A.in.len(s);
    if ( i0 >= W )
	return;
    const uint32_t B = A.B;
    const uint64_t x = (uint64_t)A.rem[s] + i0;
    uint64_t q = x / B;						// the call's window of element i0: nw at most
    uint32_t r = (uint32_t)( x % B );
    const uint8_t *applied = A.applied + (size_t)s * ( A.wcap + 1u );
    bool shut[kSqMutePer];
    uint8_t g = 0;
#pragma unroll
    for ( uint32_t u = 0; u < kSqMutePer; u++ ) {
	shut[u] = false;
	if ( i0 + u < W ) {
	    if ( u == 0u || r == 0u )
		g = applied[q];
	    shut[u] = g == 0;
	}
	if ( ++r == B ) {
	    r = 0u;
	    q++;
	}
    }
    float *row = A.audio + (size_t)s * A.audio_stride + i0;
    if ( shut[0] && shut[1] && shut[2] && shut[3] && ( A.audio_stride & 3u ) == 0u ) {
	*reinterpret_cast<float4 *>(row) = float4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
#pragma unroll
	for ( uint32_t u = 0; u < kSqMutePer; u++ )
	    if ( shut[u] )
		row[u] = 0.0f;
    }
}

} // namespace mifsk

extern "C" uint64_t mifsk_fm_squelch_level( double dbfs, uint32_t window )
{
    if ( window == 0u )
	return 0ull;
    const double top = (double)window * 0x1p48;
    const double v = rint(pow(10.0, dbfs / 10.0) * 0x1p40 * (double)window);
    if ( !( v >= 1.0 ) )
	return 1ull;
    return v >= top ? (uint64_t)window << 48 : (uint64_t)v;
}

extern "C" int mifsk_fm_squelch_batch( mifsk_ctx *ctx, const mifsk_fm_squelch_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !io || !io->d_samples || !io->d_nwindows )
	return -EINVAL;
    if ( io->nstreams <= 0 )
	return -EINVAL;
    if ( int rc = kind_check(io->kind) )
	return rc;
    if ( io->flags != 0u )
	return -EINVAL;
    const bool s16 = io->kind == MIFSK_FEED_S16;
    if ( !rows_aligned(io->d_samples, io->stream_stride, rows_vec(true, s16)) )
	return -EINVAL;
    if ( io->window < 1u || io->window > 32768u )
	return -EINVAL;
    if ( io->close_level > io->open_level )
	return -EINVAL;
    if ( io->hang > 0x80000000u )
	return -EINVAL;
    const uint64_t kmax = stream_kmax(io), wcap = kmax / io->window + 1u;
    if ( ( io->d_energy || io->d_gate ) && io->win_stride < wcap )
	return -EINVAL;
    if ( io->d_spans && !io->d_nspans )
	return -EINVAL;
    if ( io->d_audio && ( io->audio_stride < kmax || ( (uintptr_t)io->d_audio & 15u ) != 0 ) )
	return -EINVAL;

    SquelchArgs A = {};
    A.in = rows_in(io);
    A.nrows = (uint32_t)io->nstreams;
    A.ntiles = (uint32_t)( ( kmax + kSqTile - 1u ) / kSqTile );
    A.B = io->window;
    A.hang = io->hang;
    A.span_cap = io->span_cap;
    A.wcap = wcap;
    A.open_level = io->open_level;
    A.close_level = io->close_level;
    A.state = io->d_state;
    A.state_out = io->d_state_out;
    A.energy = io->d_energy;
    A.gate = io->d_gate;
    A.win_stride = io->win_stride;
    A.nwindows = io->d_nwindows;
    A.spans = io->d_spans;
    A.nspans = io->d_nspans;
    A.audio = io->d_audio;
    A.audio_stride = io->audio_stride;

    // the scratch, each part whole 16 bytes: pieces, inner, and for the mute launch applied and rem
    const unsigned __int128 n = A.nrows;
    const unsigned __int128 b_pieces = n * A.ntiles * 16u, b_inner = ( n * wcap * 8u + 15u ) / 16u * 16u;
    const unsigned __int128 b_applied = io->d_audio ? ( n * ( wcap + 1u ) + 15u ) / 16u * 16u : 0u;
    const unsigned __int128 b_rem = io->d_audio ? ( n * 4u + 15u ) / 16u * 16u : 0u;
    const unsigned __int128 bytes = b_pieces + b_inner + b_applied + b_rem;
    if ( bytes > ( (unsigned __int128)1 << 46 ) )
	return -ENOMEM;

    if ( hipSetDevice(ctx->device) != hipSuccess )
	return -EIO;
    const hipStream_t st = (hipStream_t)stream;
    StreamMem scratch(st);					// freed in the stream's order, behind the launches
    if ( int rc = scratch.alloc((size_t)bytes) )
	return rc;
    char *base = reinterpret_cast<char *>(scratch.p);
    A.pieces = reinterpret_cast<uint64_t *>(base);
    A.inner = reinterpret_cast<uint64_t *>(base + (size_t)b_pieces);
    if ( io->d_audio ) {
	A.applied = reinterpret_cast<uint8_t *>(base + (size_t)( b_pieces + b_inner ));
	A.rem = reinterpret_cast<uint32_t *>(base + (size_t)( b_pieces + b_inner + b_applied ));
    }

    if ( A.ntiles != 0u )
	if ( int rc = for_row_blocks(A.nrows, [&]( uint32_t s0, uint32_t rows ) {
		A.s0 = s0;
		return dispatch_kind(true, s16, [&]( auto, auto in16 ) {
		    hipLaunchKernelGGL(( squelch_energy_kernel<decltype(in16)::value> ), dim3(A.ntiles, rows, 1), dim3(kSqThreads),
				       0, st, A);
		    return 0;
		});
	    }) )
	    return rc;
    A.s0 = 0u;
    hipLaunchKernelGGL(squelch_gate_kernel, dim3(( A.nrows + kSqWaves - 1u ) / kSqWaves), dim3(kSqThreads), 0, st, A);
    if ( !io->d_audio || kmax == 0u )
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
    const uint32_t nblocks = (uint32_t)( ( kmax + kSqThreads * kSqMutePer - 1u ) / ( kSqThreads * kSqMutePer ) );
    return for_row_blocks(A.nrows, [&]( uint32_t s0, uint32_t rows ) {
	A.s0 = s0;
	hipLaunchKernelGGL(squelch_mute_kernel, dim3(nblocks, rows, 1), dim3(kSqThreads), 0, st, A);
	return 0;
    });
}
