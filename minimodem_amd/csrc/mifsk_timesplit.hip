// mifsk_timesplit.hip -- long recordings across the whole chip: one (mifsk_demod_long) or a small
// batch of them (mifsk_demod_long_batch), the same code.
//
// The receive loop is serial in its state (minimodem.c:1137-1463), so one stream runs on one
// wavefront.  A long recording is cut in time instead: chunk k starts at s_k = k * L, and
//   pass A  runs [s_k, s_k + W) from a zeroed state (a guess at the loop's state there) and
//           keeps only the paused state X_k;
//   pass B  runs [s_k, s_{k+1} + W) from X_k and keeps the outputs and the paused state S_k.
// Row k-1 of pass B and row k of pass A pause by the same rule at the same absolute sample, so
// when the CONTROL fields of X_k equal those of S_{k-1} (translated by L; DESIGN.md "cutting a
// stream in time") everything row k decodes is what one call decodes there.  A rejected chunk
// is run again from S_{k-1}: a round re-runs every row whose starting state disagrees with its
// predecessor's current pause (settled or not) in one batch, and the consistent prefix is settled.
// The stitch kernels below turn the per-row outputs into one stream's outputs, fixing up the
// BOOKKEEPING fields (counts, frame indices, episode totals) that the rows cannot know.  The loop
// kernels themselves are the existing ones, called through mifsk_demod_slab.
//
// Here: the kernels and the driver, a Job whose phases run() calls in order -- uncut(), or gather(),
// pass_a(), pass_b(), rounds(), tails(), stitch().  What the host decides between the launches (the
// planner, the row table, which rows a round settles, drops or runs again, where the tails go) is
// plain C++ in mifsk_timesplit_plan.cpp (mifsk_timesplit.h), checked on a CPU by
// tools/timesplit_rounds.cpp.
//
// Field classification of mifsk_stream_state (both engines):
//   control      base, rp (relative), advance, flags, noconfidence (saturating: every value
//                above FSK_MAX_NOCONFIDENCE_BITS acts alike), track_amplitude,
//                peak_confidence, carrier_band, b_mark
//   bookkeeping  carrier_nsamples, nframes_total, confidence_total, amplitude_total,
//                nframes_decoded, ep_first, ep_b_mark (== b_mark while a carrier is held),
//                first_band, nbytes_total, nepisodes_total, status
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <vector>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"
#include "mifsk_outputs.h"
#include "mifsk_timesplit.h"

using mifsk::StreamMem;

using namespace mifsk::timesplit;

namespace {

__device__ inline bool same_control( const mifsk_stream_state &p, const mifsk_stream_state &x,
	uint64_t L )
{
    return p.base == x.base + L && p.rp == x.rp + L && p.advance == x.advance
	&& p.flags == x.flags
	&& min(p.noconfidence, kNoconfSat) == min(x.noconfidence, kNoconfSat)
	&& __float_as_uint(p.track_amplitude) == __float_as_uint(x.track_amplitude)
	&& __float_as_uint(p.peak_confidence) == __float_as_uint(x.peak_confidence)
	&& p.carrier_band == x.carrier_band && p.b_mark == x.b_mark;
}

// One PCM16 sample as a float: the expression of ingest_s16_kernel (mifsk_ingest.hip), so that a
// row gathered from PCM16 is bit for bit the row gathered from mifsk_ingest_s16's floats.
__device__ inline float s16_sample( int v, float dc )
{
    return mifsk::sample_from_s16(v, dc);
}

__device__ inline float4 s16_pair( int lo, int hi, float dc )
{
    return make_float4(s16_sample((int16_t)( lo & 0xFFFF ), dc), s16_sample((int16_t)( (uint32_t)lo >> 16 ), dc),
		       s16_sample((int16_t)( hi & 0xFFFF ), dc), s16_sample((int16_t)( (uint32_t)hi >> 16 ), dc));
}

// dst[i] = x[s0 + i] for i < 4 * nvec, 0.0 behind the stream's end n.  A float source is copied as
// it is (x + s0 is 16-byte aligned; dc is not used).  A PCM16 source (T = int16_t) is converted on
// the way, x[i] / 32768 + dc: 2 B read and 4 B written per sample, the recording never exists as
// floats.  Its row start is s0 = k * L with L a multiple of 4, not of 8, so x + s0 is 8-byte
// aligned and only sometimes 16-byte aligned: 16-byte loads of 8 samples per thread where it is,
// 8-byte loads of 4 samples where it is not; 16-byte stores always.  The vector that straddles the
// stream's end is done per element.
template <typename T>
__device__ inline void copy_row( const T *__restrict__ x, uint64_t n, uint64_t s0,
	float *__restrict__ dst, uint64_t nvec, float dc )
{
    float4 *d4 = reinterpret_cast<float4 *>(dst);
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    if constexpr ( sizeof(T) == sizeof(float) ) {
	for ( uint64_t v = t0; v < nvec; v += nt ) {
	    const uint64_t i = s0 + v * 4u;
	    float4 f;
	    if ( i + 4u <= n ) {
		f = reinterpret_cast<const float4 *>(x + s0)[v];
	    } else {
		f.x = i < n ? x[i] : 0.0f;
		f.y = i + 1u < n ? x[i + 1u] : 0.0f;
		f.z = i + 2u < n ? x[i + 2u] : 0.0f;
		f.w = i + 3u < n ? x[i + 3u] : 0.0f;
	    }
	    d4[v] = f;
	}
    } else if ( ( s0 & 7u ) == 0u ) {
	for ( uint64_t p = t0; p * 2u < nvec; p += nt ) {		// 8 samples: float4s 2p and 2p + 1
	    const uint64_t i = s0 + p * 8u;
	    float4 f, g;
	    if ( i + 8u <= n ) {
		const int4 raw = reinterpret_cast<const int4 *>(x + s0)[p];
		f = s16_pair(raw.x, raw.y, dc);
		g = s16_pair(raw.z, raw.w, dc);
	    } else {
		float e[8];
#pragma unroll
		for ( uint32_t j = 0; j < 8u; j++ )
		    e[j] = i + j < n ? s16_sample(x[i + j], dc) : 0.0f;
		f = make_float4(e[0], e[1], e[2], e[3]);
		g = make_float4(e[4], e[5], e[6], e[7]);
	    }
	    d4[p * 2u] = f;
	    if ( p * 2u + 1u < nvec )
		d4[p * 2u + 1u] = g;
	}
    } else {
	for ( uint64_t v = t0; v < nvec; v += nt ) {
	    const uint64_t i = s0 + v * 4u;
	    float4 f;
	    if ( i + 4u <= n ) {
		const int2 raw = reinterpret_cast<const int2 *>(x + s0)[v];
		f = s16_pair(raw.x, raw.y, dc);
	    } else {
		f.x = i < n ? s16_sample(x[i], dc) : 0.0f;
		f.y = i + 1u < n ? s16_sample(x[i + 1u], dc) : 0.0f;
		f.z = i + 2u < n ? s16_sample(x[i + 2u], dc) : 0.0f;
		f.w = i + 3u < n ? s16_sample(x[i + 3u], dc) : 0.0f;
	    }
	    d4[v] = f;
	}
    }
}

// rows[r][i] = x_m[k * L + i] for row r = (m, k) of the row table (the loop kernels take no row
// longer than the batch stride, so the overlapping chunks are laid out apart)
template <typename T>
__global__ void ts_gather_rows( const T *__restrict__ x, uint64_t xstride,
	const StreamRef *__restrict__ streams, const RowRef *__restrict__ rowref,
	float *__restrict__ rows, uint64_t stride, uint64_t L, int nrows, float dc )
{
    for ( int r = blockIdx.y; r < nrows; r += gridDim.y ) {
	const RowRef ref = rowref[r];
	copy_row(x + (uint64_t)ref.m * xstride, streams[ref.m].n, (uint64_t)ref.k * L,
		 rows + (uint64_t)r * stride, stride / 4u, dc);
    }
}

// the streams' tails do not sit at one stride in the rows: tails[m][i] = x_m[tail_off_m + i]
// (tail_off is a multiple of 4, or the stream's length where the tail is dropped: nothing of the
// source is read then)
template <typename T>
__global__ void ts_gather_tails( const T *__restrict__ x, uint64_t xstride,
	const StreamRef *__restrict__ streams, float *__restrict__ tails, uint64_t stride, int nstreams,
	float dc )
{
    for ( int m = blockIdx.y; m < nstreams; m += gridDim.y )
	copy_row(x + (uint64_t)m * xstride, streams[m].n, streams[m].tail_off,
		 tails + (uint64_t)m * stride, stride / 4u, dc);
}

// pass A's starting states: zero, but a stream's row 0 needs no guess (a finished state: the
// loop skips the row)
__global__ void ts_guess_init( mifsk_stream_state *X, const RowRef *__restrict__ rowref, int R )
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if ( r >= R )
	return;
    mifsk_stream_state s = {};
    if ( rowref[r].k == 0u )
	s.flags = MIFSK_STATE_STARTED | MIFSK_STATE_FINISHED;
    X[r] = s;
}

// pass B's starting states: a stream's row 0 starts from zero, row k from X_k with the
// bookkeeping zeroed
__global__ void ts_prepare( const mifsk_stream_state *__restrict__ X, mifsk_stream_state *I,
	mifsk_stream_state *S, const RowRef *__restrict__ rowref, int R )
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if ( r >= R )
	return;
    mifsk_stream_state s = {};
    if ( rowref[r].k > 0u )
	s = reset_book(X[r], 0);
    I[r] = s;
    S[r] = s;
}

// code[r] of row r = (m, k >= 1): 1 = the state the row started from (X_k, or S_{k-1} of a
// re-run) agrees with S_{k-1} of its own stream in every control field, 2 = S_{k-1} finished the
// stream (--rx-one, an aborted loop): the stream's rows behind it decode nothing
__global__ void ts_verify( const mifsk_stream_state *__restrict__ X,
	const mifsk_stream_state *__restrict__ S, const RowRef *__restrict__ rowref, uint32_t *code,
	int R, uint64_t L, int reject_all )
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if ( r >= R || rowref[r].k == 0u )
	return;
    const mifsk_stream_state p = S[r - 1];
    uint32_t c = 0;
    if ( p.flags & MIFSK_STATE_FINISHED )
	c = 2u;
    else if ( !reject_all && same_control(p, X[r], L) )
	c = 1u;
    code[r] = c;
}

// one round of re-runs over rows lo..hi (of any streams): the marked rows start from S_{k-1} of
// their stream, moved into their own coordinates; the others are skipped by the loop (a finished
// state)
__global__ void ts_seed( const mifsk_stream_state *__restrict__ S, const uint8_t *__restrict__ mark,
	const RowRef *__restrict__ rowref, mifsk_stream_state *R, mifsk_stream_state *I, int lo, int hi,
	uint64_t L )
{
    const int r = lo + (int)( blockIdx.x * blockDim.x + threadIdx.x );
    if ( r > hi )
	return;
    mifsk_stream_state s = {};
    if ( mark[r] && rowref[r].k > 0u ) {
	s = reset_book(S[r - 1], L);
	I[r] = s;
    } else {
	s.flags = MIFSK_STATE_STARTED | MIFSK_STATE_FINISHED;
    }
    R[r] = s;
}

// ... and what they made replaces pass B's (counts: nframes, nbytes, nepisodes, status)
__global__ void ts_merge( const mifsk_stream_state *__restrict__ R, const uint8_t *__restrict__ mark,
	const uint32_t *__restrict__ rcnt, mifsk_stream_state *S, uint32_t *cnt, int lo, int hi,
	int nrows )
{
    const int k = lo + (int)( blockIdx.x * blockDim.x + threadIdx.x );
    if ( k > hi || !mark[k] )
	return;
    S[k] = R[k];
    for ( int j = 0; j < 4; j++ )
	cnt[j * nrows + k] = rcnt[j * nrows + k];
}

// last[m] = the paused state of stream m's last chunk, which its tail starts from
__global__ void ts_last_states( const mifsk_stream_state *__restrict__ S,
	const StreamRef *__restrict__ streams, mifsk_stream_state *last, int nstreams )
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if ( m < nstreams )
	last[m] = S[streams[m].rowbase + streams[m].K - 1u];
}

// ---- stitch ---------------------------------------------------------------------------------

// The prefix of a stream's rows 0..k-1: output counts, and the episode that is open behind them
// (its true carrier_nsamples, nframes_decoded and first frame).  A row either carries the open
// episode through (a = 1: its running values are deltas) or sets it anew (a = 0).
struct Agg {
    uint64_t	nf, nb, ne, cn, ep;
    uint32_t	nd, a, status;
    int32_t	band;
};

__device__ inline Agg agg_identity()
{
    Agg r;
    r.nf = r.nb = r.ne = r.cn = r.ep = 0;
    r.nd = 0;
    r.a = 1;
    r.status = 0;
    r.band = -1;
    return r;
}

// x, then y
__device__ inline Agg agg_combine( const Agg &x, const Agg &y )
{
    Agg r;
    r.nf = x.nf + y.nf;
    r.nb = x.nb + y.nb;
    r.ne = x.ne + y.ne;
    r.a = x.a & y.a;
    r.cn = y.a ? x.cn + y.cn : y.cn;
    r.nd = y.a ? x.nd + y.nd : y.nd;
    r.ep = y.a ? x.ep : x.nf + y.ep;
    r.status = x.status | y.status;
    r.band = x.band >= 0 ? x.band : y.band;
    return r;
}

struct StitchArgs {
    const mifsk_stream_state	*I, *S;
    const uint32_t		*cnt;		// [4][nrows]: nframes, nbytes, nepisodes, status
    const uint8_t		*drop;		// [nrows]
    const StreamRef		*streams;	// [nstreams]
    const RowRef		*rowref;	// [nrows]
    int				nrows, R;	// R chunk rows, then the nstreams tails
    const mifsk_frame		*rframes;	// [nrows][fcap]
    const uint8_t		*rbytes;	// [nrows][fcap] or NULL
    const mifsk_episode		*reps;		// [nrows][ecap]
    size_t			fcap, ecap;
    uint64_t			L;		// chunk k of a stream starts at k * L, its tail at tail_off
    Agg				*pref;		// per stream K + 2: exclusive prefixes of its K + 1 rows, the total
    mifsk_demod_io		out;
    int				autodetect;
};

// the row of stream m's j-th piece (its K chunks, then its tail) ...
__device__ inline int piece_row( const StitchArgs &a, const StreamRef &sr, int m, int j )
{
    return j < (int)sr.K ? (int)sr.rowbase + j : a.R + m;
}

// ... and the stream's prefixes: pref[j] is what lies before piece j
__device__ inline Agg *stream_pref( const StitchArgs &a, const StreamRef &sr, int m )
{
    return a.pref + sr.rowbase + 2 * (size_t)m;
}

__device__ inline Agg row_agg( const StitchArgs &a, int k )
{
    if ( a.drop[k] )
	return agg_identity();
    const mifsk_stream_state &s = a.S[k];
    Agg r;
    r.nf = a.cnt[k];
    r.nb = a.cnt[a.nrows + k];
    r.ne = a.cnt[2 * a.nrows + k];
    r.status = a.cnt[3 * a.nrows + k];
    r.a = ( a.I[k].flags & MIFSK_STATE_CARRIER ) && ( s.flags & MIFSK_STATE_CARRIER )
	&& s.ep_first == kSentinel;
    r.cn = s.carrier_nsamples;
    r.nd = s.nframes_decoded;
    r.ep = r.a ? 0u : s.ep_first;
    r.band = s.first_band;
    return r;
}

constexpr int kScanThreads = 1024;

// one workgroup per stream (K is in the thousands): the stream's counts, status and band go to
// index blockIdx.x of the caller's arrays
__global__ __launch_bounds__(kScanThreads) void ts_scan( StitchArgs a )
{
    __shared__ Agg lds[kScanThreads];
    const int t = threadIdx.x, m = blockIdx.x;
    const StreamRef sr = a.streams[m];
    Agg *pref = stream_pref(a, sr, m);
    const int np = (int)sr.K + 1;
    const int per = ( np + kScanThreads - 1 ) / kScanThreads;
    const int lo = min(np, t * per), hi = min(np, lo + per);
    Agg mine = agg_identity();
    for ( int j = lo; j < hi; j++ )
	mine = agg_combine(mine, row_agg(a, piece_row(a, sr, m, j)));
    lds[t] = mine;
    __syncthreads();
    for ( int d = 1; d < kScanThreads; d <<= 1 ) {		// inclusive scan of the threads' parts
	Agg v = lds[t];
	if ( t >= d )
	    v = agg_combine(lds[t - d], v);
	__syncthreads();
	lds[t] = v;
	__syncthreads();
    }
    Agg run = t ? lds[t - 1] : agg_identity();
    for ( int j = lo; j < hi; j++ ) {
	pref[j] = run;
	run = agg_combine(run, row_agg(a, piece_row(a, sr, m, j)));
    }
    if ( t == kScanThreads - 1 ) {
	const Agg tot = lds[t];
	pref[np] = tot;
	uint32_t status = tot.status & ~( MIFSK_STREAM_FRAMES_TRUNCATED | MIFSK_STREAM_EPISODES_TRUNCATED );
	if ( tot.nf > a.out.frames_cap && ( a.out.d_frames || a.out.d_bits || a.out.d_bytes ) )
	    status |= MIFSK_STREAM_FRAMES_TRUNCATED;
	if ( tot.ne > a.out.episodes_cap && a.out.d_episodes )
	    status |= MIFSK_STREAM_EPISODES_TRUNCATED;
	if ( a.out.d_nframes ) a.out.d_nframes[m] = (uint32_t)tot.nf;
	if ( a.out.d_nbytes ) a.out.d_nbytes[m] = (uint32_t)tot.nb;
	if ( a.out.d_nepisodes ) a.out.d_nepisodes[m] = (uint32_t)tot.ne;
	if ( a.out.d_status ) a.out.d_status[m] = status;
	if ( a.out.d_carrier_band && a.autodetect ) a.out.d_carrier_band[m] = tot.band;
    }
}

// frames, bits and bytes of row blockIdx.x to their places in its stream's arrays
__global__ void ts_scatter( StitchArgs a )
{
    const int r = blockIdx.x;
    const RowRef ref = a.rowref[r];
    const StreamRef sr = a.streams[ref.m];
    const Agg *pref = stream_pref(a, sr, ref.m) + ref.k;
    // (a row holds at most fcap frames: mifsk_max_frames of the longest row)
    const uint64_t f0 = pref[0].nf, nf = min(pref[1].nf - f0, (uint64_t)a.fcap);
    const uint64_t b0 = pref[0].nb, nb = min(pref[1].nb - b0, (uint64_t)a.fcap);
    const uint64_t off = ref.k == sr.K ? sr.tail_off : (uint64_t)ref.k * a.L;
    const size_t o0 = (size_t)ref.m * a.out.frames_cap;
    const mifsk_frame *src = a.rframes + (size_t)r * a.fcap;
    for ( uint64_t i = threadIdx.x; i < nf && f0 + i < a.out.frames_cap; i += blockDim.x ) {
	mifsk_frame f = src[i];
	f.start += off;
	if ( a.out.d_frames )
	    a.out.d_frames[o0 + f0 + i] = f;
	if ( a.out.d_bits )
	    a.out.d_bits[o0 + f0 + i] = f.bits;
    }
    if ( a.out.d_bytes && a.rbytes ) {
	const uint8_t *bs = a.rbytes + (size_t)r * a.fcap;
	for ( uint64_t i = threadIdx.x; i < nb && b0 + i < a.out.frames_cap; i += blockDim.x )
	    a.out.d_bytes[o0 + b0 + i] = bs[i];
    }
}

// episodes of row blockIdx.x; the one that began before the row gets its true count, length,
// first frame and totals -- the float totals summed again over its frames in loop order, as
// the loop sums them (minimodem.c:1397-1398).  Only the row's own stream is searched.
__global__ void ts_episodes( StitchArgs a )
{
    const int r = blockIdx.x;
    const RowRef ref = a.rowref[r];
    const int m = (int)ref.m, k = (int)ref.k;
    const StreamRef sr = a.streams[m];
    const Agg *pref = stream_pref(a, sr, m);
    const uint64_t e0 = pref[k].ne, ne = min(pref[k + 1].ne - e0, (uint64_t)a.ecap);
    const uint64_t f0 = pref[k].nf;
    mifsk_episode *dst = a.out.d_episodes + (size_t)m * a.out.episodes_cap;
    for ( uint64_t j = threadIdx.x; j < ne && e0 + j < a.out.episodes_cap; j += blockDim.x ) {
	mifsk_episode e = a.reps[(size_t)r * a.ecap + j];
	if ( j == 0 && ( a.I[r].flags & MIFSK_STATE_CARRIER ) ) {
	    const Agg &p = pref[k];
	    const uint64_t g0 = p.ep;
	    const uint64_t count = (uint64_t)p.nd + e.nframes;
	    e.carrier_nsamples += p.cn;
	    e.nframes = (uint32_t)count;
	    e.first_frame = (uint32_t)g0;
	    // the piece that holds frame g0: the last one whose prefix does not pass it
	    int lo = 0, hi = k;
	    while ( lo < hi ) {
		const int mid = ( lo + hi + 1 ) / 2;
		if ( pref[mid].nf <= g0 )
		    lo = mid;
		else
		    hi = mid - 1;
	    }
	    float ct = 0.0f, at = 0.0f;
	    uint64_t left = count, i = g0 - pref[lo].nf;
	    for ( int q = lo; q <= k && left; q++ ) {
		const uint64_t nr = min(pref[q + 1].nf - pref[q].nf, (uint64_t)a.fcap);
		const mifsk_frame *fr = a.rframes + (size_t)piece_row(a, sr, m, q) * a.fcap;
		for ( ; i < nr && left; i++, left-- ) {
		    ct += fr[i].confidence;
		    at += fr[i].amplitude;
		}
		i = 0;
	    }
	    e.confidence_total = ct;
	    e.amplitude_total = at;
	} else {
	    e.first_frame = (uint32_t)( f0 + e.first_frame );
	}
	dst[e0 + j] = e;
    }
}

unsigned blocks_for( uint64_t stride )
{
    return (unsigned)std::min<uint64_t>(64, std::max<uint64_t>(1, ( stride / 4 + 255 ) / 256));
}

// Where the recordings are: float rows (`dc` is not used: --Xrxnoise is applied to floats in
// place, before the call) or PCM16 rows, converted as they are gathered.
struct Src {
    const void	*p;		// device, 16-byte aligned
    size_t	stride;		// elements between the streams' rows
    bool	s16;		// int16_t elements (else float)
    float	dc;		// s16: the --Xrxnoise term, added to every sample
};

void gather_rows( const Src &src, dim3 grid, hipStream_t st, const StreamRef *streams, const RowRef *rowref,
	float *rows, uint64_t stride, uint64_t L, int nrows )
{
    if ( src.s16 )
	hipLaunchKernelGGL(ts_gather_rows<int16_t>, grid, dim3(256), 0, st, (const int16_t *)src.p,
			   (uint64_t)src.stride, streams, rowref, rows, stride, L, nrows, src.dc);
    else
	hipLaunchKernelGGL(ts_gather_rows<float>, grid, dim3(256), 0, st, (const float *)src.p,
			   (uint64_t)src.stride, streams, rowref, rows, stride, L, nrows, 0.0f);
}

void gather_tails( const Src &src, dim3 grid, hipStream_t st, const StreamRef *streams, float *tails,
	uint64_t stride, int nstreams )
{
    if ( src.s16 )
	hipLaunchKernelGGL(ts_gather_tails<int16_t>, grid, dim3(256), 0, st, (const int16_t *)src.p,
			   (uint64_t)src.stride, streams, tails, stride, nstreams, src.dc);
    else
	hipLaunchKernelGGL(ts_gather_tails<float>, grid, dim3(256), 0, st, (const float *)src.p,
			   (uint64_t)src.stride, streams, tails, stride, nstreams, 0.0f);
}

// Rows [lo, lo + count) of `b`, the batch of all rows from row 0 on: their samples and lengths,
// their part of the per-row result buffers, and their four counts, which lie nrows apart in `cnt`.
mifsk_demod_io rows_of( mifsk_demod_io b, uint32_t *cnt, int nrows, int lo, int count )
{
    b.d_samples += (size_t)lo * b.stream_stride;
    b.d_nsamples += lo;
    b.nstreams = count;
    mifsk::outputs_advance(b, (size_t)lo);
    b.d_nframes = cnt + lo;
    b.d_nbytes = cnt + nrows + lo;
    b.d_nepisodes = cnt + 2 * nrows + lo;
    b.d_status = cnt + 3 * nrows + lo;
    return b;
}

// a per-call device array of T, allocated and freed in the order of the call's stream
template <class T>
struct Buf : StreamMem {
    using StreamMem::StreamMem;
    T *d() const { return (T *)p; }
    int make( size_t n ) { return alloc(n * sizeof(T)); }
};

// One call from its plan to its outputs: the arguments, the row layout, every host array that a
// copy on the stream reads or writes (all of them live to the end of the call) and the device
// buffers.  run() calls the phases in order: uncut(), or gather(), pass_a(), pass_b(), rounds(),
// tails(), stitch().
struct Job {
    mifsk_ctx			*ctx;
    const mifsk_rx_config	*cfg;
    const Src			src;
    const float			rxnoise;
    const uint64_t		*nsamples;
    const mifsk_demod_io	*io_out;
    void			*stream;
    const hipStream_t		st;
    const unsigned		flags, engine;
    std::vector<mifsk_time_split_stats> ps;	// the plan, then the call's statistics
    RowLayout			lay;

    // host
    std::vector<uint32_t>	hn;		// uncut: the rows' lengths
    struct { StreamRef s; RowRef r; } one;	// uncut: the table of a lone row that is gathered
    RowFlags			f{lay};
    std::vector<uint32_t>	hcode;		// [nrows] ts_verify's codes of a round
    std::vector<mifsk_stream_state> last;	// [M] the last chunks' pauses, then the tails' starts
    mifsk_demod_io		b;		// pass B's batch of all R rows: re-runs and tails are rows_of it

    // device (the uncut batch uses the first two only)
    Buf<float>			pad{st};	// uncut: the rows as floats, every row defined up to its stride
    StreamMem			table{st};	// uncut: the rows' lengths, or `one`
    Buf<float>			rows{st};	// [R][rstride]: the chunks, laid out apart
    // [nrows] each: pass A's runs from zero to their pauses, the guesses at the chunks' entry states;
    // the state a row's kept outputs started from; the state that run paused in (a tail's: finished);
    // a round's re-runs, from start to pause ([R + m]: stream m's last pause, on its way to the host)
    Buf<mifsk_stream_state>	guess{st}, start{st}, pause{st}, rerun{st};
    // [4][nrows]: nframes, nbytes, nepisodes, status of the kept runs, and of a round's re-runs
    Buf<uint32_t>		counts{st}, rerun_counts{st};
    Buf<uint32_t>		code{st};	// [nrows] ts_verify
    // [nrows] bytes with two tenants and one hand-over: a round's marks (d_mark) from gather() to
    // the end of rounds(), the drop flags (d_drop) from the end of tails() on, which copies them over
    Buf<uint8_t>		row_flags{st};
    uint8_t			*d_mark = nullptr;
    const uint8_t		*d_drop = nullptr;
    Buf<mifsk_frame>		rframes{st};	// [nrows][fcap]
    Buf<uint8_t>		rbytes{st};	// [nrows][fcap], where the caller wants bytes
    Buf<mifsk_episode>		reps{st};	// [nrows][ecap]
    Buf<Agg>			pref{st};	// [nrows + M] ts_scan
    Buf<uint32_t>		ns{st};		// [nrows] lay.hns
    Buf<StreamRef>		streams{st};	// [M] lay.hs
    Buf<RowRef>			rowref{st};	// [nrows] lay.hrow
    Buf<float>			tail_rows{st};	// [M][tstride]

    static constexpr unsigned	tb = 256;	// the small per-row kernels' block
    unsigned blocks( int n ) const { return (unsigned)( ( n + tb - 1 ) / tb ); }

    Job( mifsk_ctx *ctx_, const mifsk_rx_config *cfg_, const Src &src_, float rxnoise_, const uint64_t *nsamples_,
	    unsigned flags_, const mifsk_demod_io *io_out_, void *stream_, std::vector<mifsk_time_split_stats> plan_ )
	: ctx(ctx_), cfg(cfg_), src(src_), rxnoise(rxnoise_), nsamples(nsamples_), io_out(io_out_), stream(stream_),
	  st((hipStream_t)stream_), flags(flags_), engine(flags_ & ( MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE )),
	  ps(std::move(plan_)), lay(cfg_, nsamples_, ps), hcode(lay.nrows, 0), last(lay.M)
    {
    }

    int uncut(), gather(), pass_a(), pass_b(), rounds(), tails(), stitch();
};

// No stream is cut: the existing call over the batch.  A batch of floats is taken where it is, and
// so is a lone row of whole float4s (no allocation, no copy); any other lone row goes over a padded
// copy, its stride being its length in whole float4s; PCM16 becomes floats through
// mifsk_ingest_s16, as the host pipeline makes them (every row defined up to its stride)
int Job::uncut()
{
    const int M = lay.M;
    int rc;
    const bool lone = M == 1;
    const uint64_t stride = lone ? std::max<uint64_t>(4, ( nsamples[0] + 3u ) & ~3ull) : src.stride;
    mifsk_demod_io io = *io_out;
    io.d_samples = (const float *)src.p;
    if ( src.s16 || !lone ) {		// the lengths: for mifsk_ingest_s16, and of a batch's rows
	hn.resize(M);
	for ( int m = 0; m < M; m++ )
	    hn[m] = (uint32_t)nsamples[m];
	if ( ( rc = table.alloc(M * sizeof(uint32_t)) ) )
	    return rc;
	HIP_OK(hipMemcpyAsync(table.p, hn.data(), M * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
    }
    if ( src.s16 ) {
	if ( ( rc = pad.make((size_t)M * stride) ) )
	    return rc;
	if ( !src.p )
	    HIP_OK(hipMemsetAsync(pad.p, 0, (size_t)M * stride * sizeof(float), st));
	else if ( ( rc = mifsk_ingest_s16(ctx, (const int16_t *)src.p, src.stride, pad.d(), stride,
					  (const uint32_t *)table.p, 0, M, rxnoise, stream) ) )
	    return rc;
	io.d_samples = pad.d();
    } else if ( lone && nsamples[0] % 4u ) {
	if ( ( rc = pad.make(stride) ) )
	    return rc;
	one = { { nsamples[0], 0, 0, 1 }, { 0, 0 } };
	if ( ( rc = table.alloc(sizeof(one)) ) )
	    return rc;
	HIP_OK(hipMemcpyAsync(table.p, &one, sizeof(one), hipMemcpyHostToDevice, st));
	HIP_OK(hipStreamSynchronize(st));
	gather_rows(src, dim3(64, 1), st, (const StreamRef *)table.p,
		    (const RowRef *)( (char *)table.p + sizeof(StreamRef) ), pad.d(), stride, 0, 1);
	io.d_samples = pad.d();
    }
    io.stream_stride = stride;
    io.d_nsamples = lone ? nullptr : (const uint32_t *)table.p;
    io.nsamples = (uint32_t)( lone ? nsamples[0] : std::min<uint64_t>(stride, 0xFFFFFFFFull) );
    io.nstreams = M;
    io.d_counters = nullptr;
    io.flags = engine;
    io.reserved = 0;
    if ( ( rc = mifsk_demod_batch(ctx, cfg, &io, stream) ) )
	return rc;
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

// everything the call holds on the device but the tails' samples; the tables go up and the chunks
// are copied apart
int Job::gather()
{
    const size_t M = lay.M, R = lay.R, nrows = lay.nrows;
    int rc;
    if ( ( rc = rows.make(R * lay.rstride) )
	    || ( rc = guess.make(nrows) ) || ( rc = start.make(nrows) )
	    || ( rc = pause.make(nrows) ) || ( rc = rerun.make(nrows) )
	    || ( rc = counts.make(4 * nrows) )
	    || ( rc = rerun_counts.make(4 * nrows) )
	    || ( rc = code.make(nrows) )
	    || ( rc = row_flags.make(nrows) )
	    || ( rc = rframes.make(nrows * lay.fcap) )
	    || ( io_out->d_bytes && ( rc = rbytes.make(nrows * lay.fcap) ) )
	    || ( rc = reps.make(nrows * lay.ecap) )
	    || ( rc = pref.make(nrows + M) )
	    || ( rc = ns.make(nrows) )
	    || ( rc = streams.make(M) )
	    || ( rc = rowref.make(nrows) ) )
	return rc;
    d_mark = row_flags.d();
    HIP_OK(hipMemsetAsync(counts.p, 0, 4 * nrows * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(d_mark, 0, nrows, st));
    HIP_OK(hipMemcpyAsync(streams.p, lay.hs.data(), M * sizeof(StreamRef), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(rowref.p, lay.hrow.data(), nrows * sizeof(RowRef), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(ns.p, lay.hns.data(), nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    gather_rows(src, dim3(blocks_for(lay.rstride), (unsigned)std::min(lay.R, 65535)), st, streams.d(), rowref.d(),
		rows.d(), lay.rstride, lay.L, lay.R);
    return 0;
}

// pass A: rows 1 .. R-1, W samples each, from a zeroed state (a stream's row 0 is skipped); then
// pass B's starting states
int Job::pass_a()
{
    const unsigned gb = blocks(lay.nrows);
    hipLaunchKernelGGL(ts_guess_init, dim3(gb), dim3(tb), 0, st, guess.d(), rowref.d(), lay.R);
    mifsk_demod_io a;
    std::memset(&a, 0, sizeof(a));
    a.flags = engine;
    a.d_samples = rows.d() + lay.rstride;
    a.stream_stride = lay.rstride;
    a.nsamples = (uint32_t)lay.W;
    a.nstreams = lay.R - 1;
    if ( const int rc = mifsk_demod_slab(ctx, cfg, &a, guess.d() + 1, nullptr, 0, stream) )
	return rc;
    hipLaunchKernelGGL(ts_prepare, dim3(gb), dim3(tb), 0, st, guess.d(), start.d(), pause.d(), rowref.d(), lay.R);
    return 0;
}

// pass B: every row up to W samples into its stream's next chunk (a stream's last one to the
// end; it stays a non-final slab: the tail finishes it)
int Job::pass_b()
{
    std::memset(&b, 0, sizeof(b));
    b.flags = engine;
    b.d_samples = rows.d();
    b.stream_stride = lay.rstride;
    b.d_nsamples = ns.d();
    b.nsamples = (uint32_t)( lay.L + lay.W );
    b.d_frames = rframes.d();
    b.d_bytes = rbytes.d();
    b.frames_cap = lay.fcap;
    b.d_episodes = reps.d();
    b.episodes_cap = lay.ecap;
    b = rows_of(b, counts.d(), lay.nrows, 0, lay.R);
    return mifsk_demod_slab(ctx, cfg, &b, pause.d(), nullptr, 0, stream);
}

// Verify, and re-run what was rejected, in rounds.  Row k of a stream is CONSISTENT when the
// state it started from agrees in control with the state row k-1 of that stream paused in;
// a stream's settled rows are its consistent prefix.  A round re-runs every inconsistent row
// of every stream at once from its predecessor's current state (settled or not: a row whose
// predecessor changes again is simply inconsistent again), so the rounds follow the longest
// run of rejections in any one stream, not their number and not the sum over the streams.
int Job::rounds()
{
    const int R = lay.R, nrows = lay.nrows;
    for ( uint32_t round = 0;; round++ ) {
	// (MIFSK_TIME_SPLIT_REJECT_ALL: every guess of pass A is rejected)
	const int reject = round == 0 && ( flags & MIFSK_TIME_SPLIT_REJECT_ALL );
	hipLaunchKernelGGL(ts_verify, dim3(blocks(nrows)), dim3(tb), 0, st, (const mifsk_stream_state *)start.d(),
			   (const mifsk_stream_state *)pause.d(), rowref.d(), code.d(), R, lay.L, reject);
	HIP_OK(hipMemcpyAsync(hcode.data(), code.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	const RowSpan span = settle_round(hcode, lay, f, ps);
	if ( span.lo < 0 )
	    return 0;
	HIP_OK(hipMemcpyAsync(d_mark, f.mark.data(), nrows, hipMemcpyHostToDevice, st));
	const int lo = span.lo, hi = span.hi, nr = hi - lo + 1;
	hipLaunchKernelGGL(ts_seed, dim3(blocks(nr)), dim3(tb), 0, st, pause.d(), (const uint8_t *)d_mark, rowref.d(),
			   rerun.d(), start.d(), lo, hi, lay.L);
	const mifsk_demod_io r = rows_of(b, rerun_counts.d(), nrows, lo, nr);
	if ( const int rc = mifsk_demod_slab(ctx, cfg, &r, rerun.d() + lo, nullptr, 0, stream) )
	    return rc;
	hipLaunchKernelGGL(ts_merge, dim3(blocks(nr)), dim3(tb), 0, st, (const mifsk_stream_state *)rerun.d(),
			   (const uint8_t *)d_mark, (const uint32_t *)rerun_counts.d(), pause.d(), counts.d(), lo, hi,
			   nrows);
    }
}

// the tails: every stream's last chunk finished as a final slab from its paused state, all of
// them one batch over a small buffer of their own (they do not sit at one stride in the rows);
// then the drop flags take the marks' place
int Job::tails()
{
    const int M = lay.M, R = lay.R;
    const size_t stsz = sizeof(mifsk_stream_state);
    hipLaunchKernelGGL(ts_last_states, dim3(blocks(M)), dim3(tb), 0, st, (const mifsk_stream_state *)pause.d(),
		       streams.d(), rerun.d() + R, M);
    HIP_OK(hipMemcpyAsync(last.data(), rerun.d() + R, M * stsz, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const Tails t = place_tails(lay, last, f.drop);
    HIP_OK(hipMemcpyAsync(streams.p, lay.hs.data(), M * sizeof(StreamRef), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(start.d() + R, last.data(), M * stsz, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(pause.d() + R, last.data(), M * stsz, hipMemcpyHostToDevice, st));
    if ( t.live ) {
	const uint64_t tstride = std::max<uint64_t>(4, ( t.longest + 3u ) & ~3ull);
	if ( const int rc = tail_rows.make((size_t)M * tstride) )
	    return rc;
	HIP_OK(hipMemcpyAsync(ns.d() + R, lay.hns.data() + R, M * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	gather_tails(src, dim3(blocks_for(tstride), (unsigned)std::min(M, 65535)), st, streams.d(), tail_rows.d(),
		     tstride, M);
	mifsk_demod_io tio = rows_of(b, counts.d(), lay.nrows, R, M);
	tio.d_samples = tail_rows.d();
	tio.stream_stride = tstride;
	tio.nsamples = (uint32_t)t.longest;
	if ( const int rc = mifsk_demod_slab(ctx, cfg, &tio, pause.d() + R, nullptr, 1, stream) )
	    return rc;
    }
    HIP_OK(hipMemcpyAsync(row_flags.p, f.drop.data(), lay.nrows, hipMemcpyHostToDevice, st));
    d_mark = nullptr;
    d_drop = row_flags.d();
    return 0;
}

int Job::stitch()
{
    // (in the order of StitchArgs' fields)
    const StitchArgs sa = { start.d(), pause.d(), counts.d(), d_drop, streams.d(), rowref.d(), lay.nrows, lay.R,
			    b.d_frames, b.d_bytes, b.d_episodes, lay.fcap, lay.ecap, lay.L, pref.d(), *io_out,
			    cfg->auto_carrier_threshold > 0.0f };
    hipLaunchKernelGGL(ts_scan, dim3(lay.M), dim3(kScanThreads), 0, st, sa);
    if ( io_out->d_frames || io_out->d_bits || io_out->d_bytes )
	hipLaunchKernelGGL(ts_scatter, dim3(lay.nrows), dim3(256), 0, st, sa);
    if ( io_out->d_episodes )
	hipLaunchKernelGGL(ts_episodes, dim3(lay.nrows), dim3(64), 0, st, sa);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

// The entry points (which have checked the rows against the source's stride); mifsk_demod_long is
// the nstreams == 1 case of a float source, whose one row holds just nsamples[0] floats (the
// stride is not used then)
int run( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const Src &src, float rxnoise,
	const uint64_t *nsamples, int nstreams, const mifsk_time_split *params,
	const mifsk_demod_io *io_out, mifsk_time_split_stats *stats, void *stream )
{
    if ( !ctx || !io_out || !nsamples || nstreams <= 0 || mifsk_check_cfg(cfg)
	    || ( (uintptr_t)src.p & 15u ) )
	return -EINVAL;
    int rc;
    for ( int m = 0; m < nstreams; m++ )
	if ( nsamples[m] && !src.p )
	    return -EINVAL;
    if ( ( ( io_out->d_bytes || io_out->d_bits || io_out->d_frames ) && io_out->frames_cap == 0 )
	    || ( io_out->d_episodes && io_out->episodes_cap == 0 ) )
	return -EINVAL;
    const unsigned flags = params ? params->flags : 0u;
    if ( ( flags & MIFSK_IO_ENGINE_WORKGROUP ) && cfg->auto_carrier_threshold > 0.0f )
	return -EINVAL;
    if ( ( rc = mifsk::time_split_check_params(cfg, params) ) )
	return rc;		// (before any HIP call)
    HIP_OK(hipSetDevice(ctx->device));

    // the chip's worth of chunks for this engine
    uint32_t hint = 0;
    mifsk_launch_info li;
    if ( mifsk_demod_plan_ex(ctx, cfg, 1, 0xFFFFFFFFu, flags & ~MIFSK_TIME_SPLIT_REJECT_ALL, &li) == 0 )
	hint = li.compute_units * kChunksPerCu;
    std::vector<mifsk_time_split_stats> ps(nstreams);
    if ( ( rc = plan(cfg, nsamples, nstreams, params, hint, ps.data()) ) )
	return rc;

    Job j(ctx, cfg, src, rxnoise, nsamples, flags, io_out, stream, std::move(ps));
    if ( j.lay.R == nstreams )
	rc = j.uncut();
    else
	( rc = j.gather() ) || ( rc = j.pass_a() ) || ( rc = j.pass_b() ) || ( rc = j.rounds() )
	    || ( rc = j.tails() ) || ( rc = j.stitch() );
    if ( rc )
	return rc;
    if ( stats )
	std::copy(j.ps.begin(), j.ps.end(), stats);
    return 0;
}

} // namespace

extern "C" int mifsk_demod_long( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const float *d_samples,
	uint64_t nsamples, const mifsk_time_split *params, const mifsk_demod_io *io_out,
	mifsk_time_split_stats *stats, void *stream )
{
    const Src src = { d_samples, 0, false, 0.0f };
    return run(ctx, cfg, src, 0.0f, &nsamples, 1, params, io_out, stats, stream);
}

extern "C" int mifsk_demod_long_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const float *d_samples, size_t stream_stride, const uint64_t *nsamples, int nstreams,
	const mifsk_time_split *params, const mifsk_demod_io *io_out, mifsk_time_split_stats *stats,
	void *stream )
{
    if ( stream_stride % 4u || !nsamples || nstreams <= 0 )
	return -EINVAL;
    for ( int m = 0; m < nstreams; m++ )
	if ( nsamples[m] > stream_stride )
	    return -EINVAL;
    const Src src = { d_samples, stream_stride, false, 0.0f };
    return run(ctx, cfg, src, 0.0f, nsamples, nstreams, params, io_out, stats, stream);
}

extern "C" int mifsk_demod_long_batch_s16( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const int16_t *d_pcm, size_t pcm_stride, const uint64_t *nsamples, int nstreams, float rxnoise,
	const mifsk_time_split *params, const mifsk_demod_io *io_out, mifsk_time_split_stats *stats,
	void *stream )
{
    if ( !ctx || !cfg || !io_out || !nsamples )
	return -EINVAL;
    if ( nstreams <= 0 )
	return -EINVAL;
    if ( ( (uintptr_t)d_pcm & 15u ) || pcm_stride % 8u )
	return -EINVAL;
    for ( int m = 0; m < nstreams; m++ )
	if ( nsamples[m] > pcm_stride )
	    return -EINVAL;
    const Src src = { d_pcm, pcm_stride, true, mifsk::rxnoise_term(rxnoise) };
    return run(ctx, cfg, src, rxnoise, nsamples, nstreams, params, io_out, stats, stream);
}
