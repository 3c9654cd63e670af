// mifsk_timesplit.hip -- one long recording across the whole chip (mifsk_demod_long).
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
// predecessor's current pause (settled or not) in one batch, and the consistent prefix is settled.  The stitch kernels below turn the per-row outputs into one stream's outputs,
// fixing up the BOOKKEEPING fields (counts, frame indices, episode totals) that the rows cannot
// know.  The loop kernels themselves are the existing ones, called through mifsk_demod_slab.
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

namespace {

constexpr uint32_t kSentinel = 0xFFFFFFFFu;	// ep_first of an episode that began before the row
constexpr uint32_t kNoconfSat = 21u;		// FSK_MAX_NOCONFIDENCE_BITS + 1 (minimodem.c:1294)
constexpr double kDefaultWarmupSeconds = 10.0;	// DESIGN.md "cutting a stream in time"
constexpr uint32_t kChunksPerCu = 4;
// The rows are laid out apart, so the copy holds the recording plus (K - 1) * W samples of
// warm-up overlap; the library's choice of K keeps that overlap within this many bytes.
constexpr uint64_t kOverlapBudget = 4ull << 30;

// A row's starting state with the bookkeeping zeroed: the row's outputs then count from 0 and
// its running episode values are deltas against the state it starts from.  `shift` moves the
// state into the coordinates of a row that starts `shift` samples later.
__host__ __device__ inline mifsk_stream_state reset_book( mifsk_stream_state s, uint64_t shift )
{
    s.base -= shift;
    s.rp -= shift;
    s.carrier_nsamples = 0;
    s.nframes_total = 0;
    s.confidence_total = 0.0f;
    s.amplitude_total = 0.0f;
    s.nframes_decoded = 0;
    s.first_band = -1;
    s.ep_first = ( s.flags & MIFSK_STATE_CARRIER ) ? kSentinel : 0u;
    s.nbytes_total = 0;
    s.nepisodes_total = 0;
    s.status = 0;
    return s;
}

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

// rows[k][i] = x[k * L + i] for i < row_len, 0.0 behind the recording's end (the loop kernels
// take no row longer than the batch stride, so the overlapping chunks are laid out apart)
__global__ void ts_gather_rows( const float *__restrict__ x, uint64_t n, float *__restrict__ rows,
	uint64_t stride, uint64_t L, int nrows )
{
    const int k = blockIdx.y;
    if ( k >= nrows )
	return;
    const uint64_t s0 = (uint64_t)k * L;
    float4 *dst = reinterpret_cast<float4 *>(rows + (uint64_t)k * stride);
    const uint64_t nvec = stride / 4u;
    for ( uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec;
	  v += (uint64_t)gridDim.x * blockDim.x ) {
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
	dst[v] = f;
    }
}

// pass B's starting states: I_0 = 0, I_k = X_k with the bookkeeping zeroed
__global__ void ts_prepare( const mifsk_stream_state *__restrict__ X, mifsk_stream_state *I,
	mifsk_stream_state *S, int K )
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if ( k >= K )
	return;
    mifsk_stream_state r = {};
    if ( k > 0 )
	r = reset_book(X[k], 0);
    I[k] = r;
    S[k] = r;
}

// code[k] (k >= 1): 1 = the state row k started from (X_k, or S_{k-1} of a re-run) agrees with
// S_{k-1} in every control field, 2 = S_{k-1} finished the stream (--rx-one, an aborted loop):
// the rows behind it decode nothing
__global__ void ts_verify( const mifsk_stream_state *__restrict__ X,
	const mifsk_stream_state *__restrict__ S, uint32_t *code, int K, uint64_t L, int reject_all )
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if ( k < 1 || k >= K )
	return;
    const mifsk_stream_state p = S[k - 1];
    uint32_t c = 0;
    if ( p.flags & MIFSK_STATE_FINISHED )
	c = 2u;
    else if ( !reject_all && same_control(p, X[k], L) )
	c = 1u;
    code[k] = c;
}

// one round of re-runs over rows lo..hi: the marked rows start from S_{k-1}, moved into their
// own coordinates; the others are skipped by the loop (a finished state)
__global__ void ts_seed( const mifsk_stream_state *__restrict__ S, const uint8_t *__restrict__ mark,
	mifsk_stream_state *R, mifsk_stream_state *I, int lo, int hi, uint64_t L )
{
    const int k = lo + (int)( blockIdx.x * blockDim.x + threadIdx.x );
    if ( k > hi )
	return;
    mifsk_stream_state r = {};
    if ( mark[k] ) {
	r = reset_book(S[k - 1], L);
	I[k] = r;
    } else {
	r.flags = MIFSK_STATE_STARTED | MIFSK_STATE_FINISHED;
    }
    R[k] = r;
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

// ---- stitch ---------------------------------------------------------------------------------

// The prefix of rows 0..k-1: output counts, and the episode that is open behind them (its true
// carrier_nsamples, nframes_decoded and first frame).  A row either carries the open episode
// through (a = 1: its running values are deltas) or sets it anew (a = 0).
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
    int				nrows;
    const mifsk_frame		*rframes;	// [nrows][fcap]
    const uint8_t		*rbytes;	// [nrows][fcap] or NULL
    const mifsk_episode		*reps;		// [nrows][ecap]
    size_t			fcap, ecap;
    uint64_t			L, tail_off;	// row k < nrows - 1 starts at k * L, the last at tail_off
    Agg				*pref;		// [nrows + 1] exclusive prefixes, [nrows] = total
    mifsk_demod_io		out;
    int				autodetect;
};

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

// one workgroup: K is in the thousands
__global__ __launch_bounds__(kScanThreads) void ts_scan( StitchArgs a )
{
    __shared__ Agg lds[kScanThreads];
    const int t = threadIdx.x;
    const int per = ( a.nrows + kScanThreads - 1 ) / kScanThreads;
    const int lo = min(a.nrows, t * per), hi = min(a.nrows, lo + per);
    Agg mine = agg_identity();
    for ( int k = lo; k < hi; k++ )
	mine = agg_combine(mine, row_agg(a, k));
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
    for ( int k = lo; k < hi; k++ ) {
	a.pref[k] = run;
	run = agg_combine(run, row_agg(a, k));
    }
    if ( t == kScanThreads - 1 ) {
	const Agg tot = lds[t];
	a.pref[a.nrows] = tot;
	uint32_t status = tot.status & ~( MIFSK_STREAM_FRAMES_TRUNCATED | MIFSK_STREAM_EPISODES_TRUNCATED );
	if ( tot.nf > a.out.frames_cap && ( a.out.d_frames || a.out.d_bits || a.out.d_bytes ) )
	    status |= MIFSK_STREAM_FRAMES_TRUNCATED;
	if ( tot.ne > a.out.episodes_cap && a.out.d_episodes )
	    status |= MIFSK_STREAM_EPISODES_TRUNCATED;
	if ( a.out.d_nframes ) a.out.d_nframes[0] = (uint32_t)tot.nf;
	if ( a.out.d_nbytes ) a.out.d_nbytes[0] = (uint32_t)tot.nb;
	if ( a.out.d_nepisodes ) a.out.d_nepisodes[0] = (uint32_t)tot.ne;
	if ( a.out.d_status ) a.out.d_status[0] = status;
	if ( a.out.d_carrier_band && a.autodetect ) a.out.d_carrier_band[0] = tot.band;
    }
}

// frames, bits and bytes of row blockIdx.x to their places in the stream's arrays
__global__ void ts_scatter( StitchArgs a )
{
    const int k = blockIdx.x;
    // (a row holds at most fcap frames: mifsk_max_frames of the longest row)
    const uint64_t f0 = a.pref[k].nf, nf = min(a.pref[k + 1].nf - f0, (uint64_t)a.fcap);
    const uint64_t b0 = a.pref[k].nb, nb = min(a.pref[k + 1].nb - b0, (uint64_t)a.fcap);
    const uint64_t off = k == a.nrows - 1 ? a.tail_off : (uint64_t)k * a.L;
    const mifsk_frame *src = a.rframes + (size_t)k * a.fcap;
    for ( uint64_t i = threadIdx.x; i < nf && f0 + i < a.out.frames_cap; i += blockDim.x ) {
	mifsk_frame f = src[i];
	f.start += off;
	if ( a.out.d_frames )
	    a.out.d_frames[f0 + i] = f;
	if ( a.out.d_bits )
	    a.out.d_bits[f0 + i] = f.bits;
    }
    if ( a.out.d_bytes && a.rbytes ) {
	const uint8_t *bs = a.rbytes + (size_t)k * a.fcap;
	for ( uint64_t i = threadIdx.x; i < nb && b0 + i < a.out.frames_cap; i += blockDim.x )
	    a.out.d_bytes[b0 + i] = bs[i];
    }
}

// episodes of row blockIdx.x; the one that began before the row gets its true count, length,
// first frame and totals -- the float totals summed again over its frames in loop order, as
// the loop sums them (minimodem.c:1397-1398)
__global__ void ts_episodes( StitchArgs a )
{
    const int k = blockIdx.x;
    const uint64_t e0 = a.pref[k].ne, ne = min(a.pref[k + 1].ne - e0, (uint64_t)a.ecap);
    const uint64_t f0 = a.pref[k].nf;
    for ( uint64_t j = threadIdx.x; j < ne && e0 + j < a.out.episodes_cap; j += blockDim.x ) {
	mifsk_episode e = a.reps[(size_t)k * a.ecap + j];
	if ( j == 0 && ( a.I[k].flags & MIFSK_STATE_CARRIER ) ) {
	    const Agg &p = a.pref[k];
	    const uint64_t g0 = p.ep;
	    const uint64_t count = (uint64_t)p.nd + e.nframes;
	    e.carrier_nsamples += p.cn;
	    e.nframes = (uint32_t)count;
	    e.first_frame = (uint32_t)g0;
	    // the row that holds frame g0: the last one whose prefix does not pass it
	    int lo = 0, hi = k;
	    while ( lo < hi ) {
		const int mid = ( lo + hi + 1 ) / 2;
		if ( a.pref[mid].nf <= g0 )
		    lo = mid;
		else
		    hi = mid - 1;
	    }
	    float ct = 0.0f, at = 0.0f;
	    uint64_t left = count, i = g0 - a.pref[lo].nf;
	    for ( int r = lo; r <= k && left; r++ ) {
		const uint64_t nr = min(a.pref[r + 1].nf - a.pref[r].nf, (uint64_t)a.fcap);
		const mifsk_frame *fr = a.rframes + (size_t)r * a.fcap;
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
	a.out.d_episodes[e0 + j] = e;
    }
}

uint64_t gcd64( uint64_t a, uint64_t b )
{
    while ( b ) {
	const uint64_t t = a % b;
	a = b;
	b = t;
    }
    return a;
}

const unsigned kKnownFlags = MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE
			   | MIFSK_TIME_SPLIT_REJECT_ALL;

// the planner; chunks_hint: the chunk count that fills the chip (0: params->chunks or the
// default of a host-only call)
int plan( const mifsk_rx_config *cfg, uint64_t n, const mifsk_time_split *params,
	uint32_t chunks_hint, mifsk_time_split_stats *out )
{
    if ( !cfg || !out || mifsk_check_cfg(cfg) )
	return -EINVAL;
    mifsk_time_split p;
    std::memset(&p, 0, sizeof(p));
    if ( params )
	p = *params;
    if ( p.flags & ~kKnownFlags )
	return -EINVAL;
    if ( ( p.flags & MIFSK_IO_ENGINE_WORKGROUP ) && ( p.flags & MIFSK_IO_ENGINE_WAVE ) )
	return -EINVAL;
    if ( p.flags & MIFSK_IO_RING_EXACT )
	return -ENOTSUP;
    if ( cfg->samplebuf_size < 2u )
	return -EINVAL;
    const uint64_t half = cfg->samplebuf_size / 2u;
    const uint64_t lattice = half / gcd64(half, 4) * 4;		// lcm(samplebuf_size / 2, 4)
    const uint64_t wmin = 2ull * cfg->samplebuf_size;
    if ( p.warmup && p.warmup < wmin )
	return -EINVAL;
    if ( p.chunk && ( p.chunk % lattice || p.chunk >= 0x7FFFFFF0ull ) )
	return -EINVAL;
    if ( p.warmup >= 0x7FFFFFF0ull || n >= ( 1ull << 62 ) )
	return -EINVAL;		// (rows are uint32 lengths; keeps the arithmetic below exact)
    uint64_t W = p.warmup;
    if ( !W ) {
	W = (uint64_t)( kDefaultWarmupSeconds * cfg->sample_rate );
	W = std::max(W, wmin);
    }
    std::memset(out, 0, sizeof(*out));
    out->nsamples = n;
    out->warmup = W;
    out->lattice = lattice;
    uint64_t L = p.chunk;
    uint64_t K = 1;
    if ( n > W ) {
	if ( !L ) {
	    uint64_t target = p.chunks ? p.chunks : ( chunks_hint ? chunks_hint : 1024u );
	    target = std::min(target, std::max<uint64_t>(2, kOverlapBudget / ( W * sizeof(float) )));
	    L = ( n - W + target - 1 ) / target;
	    L = std::max(lattice, ( L + lattice - 1 ) / lattice * lattice);
	}
	K = ( n - W ) / L + 1;
	// the library's choice: a split pays when a row (about L + 2 W) is well short of the whole
	if ( !p.chunk && !p.warmup && 4 * W > n )
	    K = 1;
    }
    if ( K < 2 ) {
	K = 1;
	L = n;
    }
    if ( K > 1 && ( L + W >= 0x7FFFFFF0ull || K > 0x7FFFFFFull ) )
	return -EINVAL;
    if ( K == 1 && n > 0xFFFFFFF0ull )
	return -EINVAL;
    out->nchunks = (uint32_t)K;
    out->chunk = L;
    out->samples_speculative = K > 1 ? ( K - 1 ) * W + ( K - 1 ) * W : 0;
    return 0;
}

struct DevBuf {
    void *p = nullptr;
    hipStream_t st = nullptr;
    ~DevBuf() { if ( p ) (void)hipFreeAsync(p, st); }
};

int alloc( DevBuf &b, size_t bytes, hipStream_t st )
{
    b.st = st;
    return hipMallocAsync(&b.p, bytes ? bytes : 16, st) == hipSuccess ? 0 : -ENOMEM;
}

} // namespace

extern "C" int mifsk_time_split_plan_get( const mifsk_rx_config *cfg, uint64_t nsamples,
	const mifsk_time_split *params, mifsk_time_split_stats *out )
{
    return plan(cfg, nsamples, params, 0, out);
}

extern "C" int mifsk_demod_long( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const float *d_samples,
	uint64_t nsamples, const mifsk_time_split *params, const mifsk_demod_io *io_out,
	mifsk_time_split_stats *stats, void *stream )
{
    if ( !ctx || !io_out || mifsk_check_cfg(cfg) || ( nsamples && !d_samples )
	    || ( (uintptr_t)d_samples & 15u ) )
	return -EINVAL;
    if ( ( io_out->d_bytes || io_out->d_bits || io_out->d_frames ) && io_out->frames_cap == 0 )
	return -EINVAL;
    if ( io_out->d_episodes && io_out->episodes_cap == 0 )
	return -EINVAL;
    const unsigned flags = params ? params->flags : 0u;
    const unsigned engine = flags & ( MIFSK_IO_ENGINE_WORKGROUP | MIFSK_IO_ENGINE_WAVE );
    if ( ( flags & MIFSK_IO_ENGINE_WORKGROUP ) && cfg->auto_carrier_threshold > 0.0f )
	return -EINVAL;
    HIP_OK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;

    // the chip's worth of chunks for this engine
    uint32_t hint = 0;
    {
	mifsk_launch_info li;
	if ( mifsk_demod_plan_ex(ctx, cfg, 1, 0xFFFFFFFFu, flags & ~MIFSK_TIME_SPLIT_REJECT_ALL, &li) == 0 )
	    hint = li.compute_units * kChunksPerCu;
    }
    mifsk_time_split_stats ps;
    int rc = plan(cfg, nsamples, params, hint, &ps);
    if ( rc )
	return rc;
    const uint64_t K = ps.nchunks, L = ps.chunk, W = ps.warmup;

    mifsk_demod_io base;
    std::memset(&base, 0, sizeof(base));
    base.flags = engine;

    if ( K == 1 ) {
	// the existing single call (over a padded copy unless the row is whole float4s already)
	DevBuf pad;
	const float *x = d_samples;
	const uint64_t stride = ( nsamples + 3u ) & ~3ull;
	if ( stride != nsamples ) {
	    if ( ( rc = alloc(pad, stride * sizeof(float), st) ) )
		return rc;
	    hipLaunchKernelGGL(ts_gather_rows, dim3(64, 1), dim3(256), 0, st, d_samples, nsamples,
			       (float *)pad.p, stride, (uint64_t)0, 1);
	    x = (const float *)pad.p;
	}
	mifsk_demod_io io = *io_out;
	io.d_samples = x;
	io.stream_stride = stride ? stride : 4;
	io.d_nsamples = nullptr;
	io.nsamples = (uint32_t)nsamples;
	io.nstreams = 1;
	io.d_counters = nullptr;
	io.flags = engine;
	io.reserved = 0;
	rc = mifsk_demod_batch(ctx, cfg, &io, stream);
	if ( rc )
	    return rc;
	HIP_OK(hipStreamSynchronize(st));
	if ( stats ) {
	    *stats = ps;
	    stats->accepted = 0;
	}
	return 0;
    }

    const int nrows = (int)K + 1;			// the K chunks and the final tail
    const uint64_t rstride = ( L + W + 3u ) & ~3ull;
    const size_t fcap = mifsk_max_frames(cfg, L + W);
    const size_t ecap = mifsk_max_episodes(cfg, L + W) + 1;
    const bool want_bytes = io_out->d_bytes != nullptr;
    DevBuf rows, X, I, S, R, cnt, rcnt, code, mark, rframes, rbytes, reps, pref, ns;
    const size_t stsz = sizeof(mifsk_stream_state);
    if ( ( rc = alloc(rows, K * rstride * sizeof(float), st) )
	    || ( rc = alloc(X, nrows * stsz, st) ) || ( rc = alloc(I, nrows * stsz, st) )
	    || ( rc = alloc(S, nrows * stsz, st) ) || ( rc = alloc(R, nrows * stsz, st) )
	    || ( rc = alloc(cnt, 4 * nrows * sizeof(uint32_t), st) )
	    || ( rc = alloc(rcnt, 4 * nrows * sizeof(uint32_t), st) )
	    || ( rc = alloc(code, nrows * sizeof(uint32_t), st) )
	    || ( rc = alloc(mark, nrows, st) )
	    || ( rc = alloc(rframes, nrows * fcap * sizeof(mifsk_frame), st) )
	    || ( want_bytes && ( rc = alloc(rbytes, nrows * fcap, st) ) )
	    || ( rc = alloc(reps, nrows * ecap * sizeof(mifsk_episode), st) )
	    || ( rc = alloc(pref, ( nrows + 1 ) * sizeof(Agg), st) )
	    || ( rc = alloc(ns, nrows * sizeof(uint32_t), st) ) )
	return rc;
    auto *dX = (mifsk_stream_state *)X.p, *dI = (mifsk_stream_state *)I.p;
    auto *dS = (mifsk_stream_state *)S.p, *dR = (mifsk_stream_state *)R.p;
    auto *dcnt = (uint32_t *)cnt.p, *drcnt = (uint32_t *)rcnt.p;
    auto *dframes = (mifsk_frame *)rframes.p;
    auto *deps = (mifsk_episode *)reps.p;
    float *drows = (float *)rows.p;

    HIP_OK(hipMemsetAsync(X.p, 0, nrows * stsz, st));
    HIP_OK(hipMemsetAsync(cnt.p, 0, 4 * nrows * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(mark.p, 0, nrows, st));
    {
	const unsigned bx = (unsigned)std::min<uint64_t>(64, ( rstride / 4 + 255 ) / 256);
	hipLaunchKernelGGL(ts_gather_rows, dim3(bx, (unsigned)K), dim3(256), 0, st, d_samples,
			   nsamples, drows, rstride, L, (int)K);
    }
    std::vector<uint32_t> hns(nrows, 0);
    for ( uint64_t k = 0; k < K; k++ )
	hns[k] = (uint32_t)( k + 1 < K ? L + W : nsamples - k * L );
    HIP_OK(hipMemcpyAsync(ns.p, hns.data(), nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));

    // pass A: rows 1 .. K-1, W samples each, from a zeroed state
    mifsk_demod_io a = base;
    a.d_samples = drows + rstride;
    a.stream_stride = rstride;
    a.nsamples = (uint32_t)W;
    a.nstreams = (int)K - 1;
    if ( ( rc = mifsk_demod_slab(ctx, cfg, &a, dX + 1, nullptr, 0, stream) ) )
	return rc;
    const unsigned tb = 256, gb = (unsigned)( ( nrows + tb - 1 ) / tb );
    hipLaunchKernelGGL(ts_prepare, dim3(gb), dim3(tb), 0, st, dX, dI, dS, (int)K);

    // pass B: rows 0 .. K-1 up to W samples into the next chunk (the last one to the end; it
    // stays a non-final slab: the tail below finishes it)
    mifsk_demod_io b = base;
    b.d_samples = drows;
    b.stream_stride = rstride;
    b.d_nsamples = (const uint32_t *)ns.p;
    b.nsamples = (uint32_t)( L + W );
    b.nstreams = (int)K;
    b.d_frames = dframes;
    b.d_bytes = (uint8_t *)rbytes.p;
    b.frames_cap = fcap;
    b.d_episodes = deps;
    b.episodes_cap = ecap;
    b.d_nframes = dcnt;
    b.d_nbytes = dcnt + nrows;
    b.d_nepisodes = dcnt + 2 * nrows;
    b.d_status = dcnt + 3 * nrows;
    if ( ( rc = mifsk_demod_slab(ctx, cfg, &b, dS, nullptr, 0, stream) ) )
	return rc;

    // Verify, and re-run what was rejected, in rounds.  Row k is CONSISTENT when the state it
    // started from agrees in control with the state row k-1 paused in; the settled rows are the
    // consistent prefix.  A round re-runs every inconsistent row at once from its predecessor's
    // current state (settled or not: a row whose predecessor changes again is simply
    // inconsistent again), so the rounds follow the longest run of rejections, not their number.
    std::vector<uint8_t> settled(nrows, 0), drop(nrows, 0), hmark(nrows, 0), ran(nrows, 0);
    std::vector<uint32_t> hcode(nrows, 0);
    settled[0] = 1;
    uint32_t accepted = 0, rerun = 0, rounds = 0;
    uint64_t rerun_samples = 0;
    for ( ;; ) {
	// (MIFSK_TIME_SPLIT_REJECT_ALL: every guess of pass A is rejected)
	const int reject = rounds == 0 && ( flags & MIFSK_TIME_SPLIT_REJECT_ALL );
	hipLaunchKernelGGL(ts_verify, dim3(gb), dim3(tb), 0, st, (const mifsk_stream_state *)dI,
			   (const mifsk_stream_state *)dS, (uint32_t *)code.p, (int)K, L, reject);
	HIP_OK(hipMemcpyAsync(hcode.data(), code.p, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	for ( uint64_t k = 1; k < K; k++ ) {
	    if ( settled[k] )
		continue;
	    if ( !settled[k - 1] )
		break;
	    if ( drop[k - 1] || ( hcode[k] & 2u ) ) {
		drop[k] = settled[k] = 1;
	    } else if ( hcode[k] & 1u ) {
		settled[k] = 1;
		accepted += !ran[k];
	    } else {
		break;
	    }
	}
	int lo = -1, hi = -1;
	std::fill(hmark.begin(), hmark.end(), 0);
	for ( uint64_t k = 1; k < K; k++ )
	    if ( !settled[k] && hcode[k] == 0u ) {	// (behind a finished row: wait for it to settle)
		hmark[k] = 1;
		if ( lo < 0 )
		    lo = (int)k;
		hi = (int)k;
	    }
	if ( lo < 0 )
	    break;
	HIP_OK(hipMemcpyAsync(mark.p, hmark.data(), nrows, hipMemcpyHostToDevice, st));
	const int m = hi - lo + 1;
	const unsigned gm = (unsigned)( ( m + tb - 1 ) / tb );
	hipLaunchKernelGGL(ts_seed, dim3(gm), dim3(tb), 0, st, dS, (const uint8_t *)mark.p, dR, dI,
			   lo, hi, L);
	mifsk_demod_io r = b;
	r.d_samples = drows + (size_t)lo * rstride;
	r.d_nsamples = (const uint32_t *)ns.p + lo;
	r.nstreams = m;
	r.d_frames = dframes + (size_t)lo * fcap;
	r.d_bytes = rbytes.p ? (uint8_t *)rbytes.p + (size_t)lo * fcap : nullptr;
	r.d_episodes = deps + (size_t)lo * ecap;
	r.d_nframes = drcnt + lo;
	r.d_nbytes = drcnt + nrows + lo;
	r.d_nepisodes = drcnt + 2 * nrows + lo;
	r.d_status = drcnt + 3 * nrows + lo;
	if ( ( rc = mifsk_demod_slab(ctx, cfg, &r, dR + lo, nullptr, 0, stream) ) )
	    return rc;
	hipLaunchKernelGGL(ts_merge, dim3(gm), dim3(tb), 0, st, (const mifsk_stream_state *)dR,
			   (const uint8_t *)mark.p, (const uint32_t *)drcnt, dS, dcnt, lo, hi, nrows);
	for ( int k = lo; k <= hi; k++ )
	    if ( hmark[k] ) {
		ran[k] = 1;
		rerun++;
		rerun_samples += hns[k];
	    }
	rounds++;
    }

    // the tail: the last chunk's loop finished as a final slab, from its paused state
    uint64_t tail_off = 0;
    mifsk_stream_state last;
    HIP_OK(hipMemcpyAsync(&last, dS + ( K - 1 ), stsz, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if ( drop[K - 1] || ( last.flags & MIFSK_STATE_FINISHED ) ) {
	drop[K] = 1;
    } else {
	const uint64_t rel = last.base & ~3ull;	// (rows start 16-byte aligned)
	tail_off = ( K - 1 ) * L + rel;
	const mifsk_stream_state it = reset_book(last, rel);
	HIP_OK(hipMemcpyAsync(dI + K, &it, stsz, hipMemcpyHostToDevice, st));
	HIP_OK(hipMemcpyAsync(dS + K, &it, stsz, hipMemcpyHostToDevice, st));
	const uint64_t nt = nsamples - tail_off;
	mifsk_demod_io t = b;
	t.d_samples = drows + ( K - 1 ) * rstride + rel;
	t.stream_stride = ( nt + 3u ) & ~3ull;
	t.d_nsamples = nullptr;
	t.nsamples = (uint32_t)nt;
	t.nstreams = 1;
	t.d_frames = dframes + K * fcap;
	t.d_bytes = rbytes.p ? (uint8_t *)rbytes.p + K * fcap : nullptr;
	t.d_episodes = deps + K * ecap;
	t.d_nframes = dcnt + K;
	t.d_nbytes = dcnt + nrows + K;
	t.d_nepisodes = dcnt + 2 * nrows + K;
	t.d_status = dcnt + 3 * nrows + K;
	if ( ( rc = mifsk_demod_slab(ctx, cfg, &t, dS + K, nullptr, 1, stream) ) )
	    return rc;
    }
    HIP_OK(hipMemcpyAsync(mark.p, drop.data(), nrows, hipMemcpyHostToDevice, st));

    // stitch
    StitchArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.I = dI;
    sa.S = dS;
    sa.cnt = dcnt;
    sa.drop = (const uint8_t *)mark.p;
    sa.nrows = nrows;
    sa.rframes = dframes;
    sa.rbytes = (const uint8_t *)rbytes.p;
    sa.reps = deps;
    sa.fcap = fcap;
    sa.ecap = ecap;
    sa.L = L;
    sa.tail_off = tail_off;
    sa.pref = (Agg *)pref.p;
    sa.out = *io_out;
    sa.autodetect = cfg->auto_carrier_threshold > 0.0f;
    hipLaunchKernelGGL(ts_scan, dim3(1), dim3(kScanThreads), 0, st, sa);
    if ( io_out->d_frames || io_out->d_bits || io_out->d_bytes )
	hipLaunchKernelGGL(ts_scatter, dim3(nrows), dim3(256), 0, st, sa);
    if ( io_out->d_episodes )
	hipLaunchKernelGGL(ts_episodes, dim3(nrows), dim3(64), 0, st, sa);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    if ( stats ) {
	*stats = ps;
	stats->accepted = accepted;
	stats->rerun = rerun;
	stats->rounds = rounds;
	stats->samples_rerun = rerun_samples;
    }
    return 0;
}
