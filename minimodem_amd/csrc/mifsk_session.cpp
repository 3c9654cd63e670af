// mifsk_session.cpp -- a batch of streams that arrive in pieces, fed from host memory
// (include/mifsk.h "streams fed in pieces from host memory").
//
// The reference reads its one stream half a samplebuf at a time and never holds more
// (src/minimodem.c:1144-1174): a recording longer than memory, or live audio, is its normal case.
// mifsk_demod_slab is that for a batch on the device -- state in, state out -- but leaves its
// caller the bookkeeping: which samples the loop has not passed yet, where each row starts in its
// stream, output arrays of the right size, the copies.  A session owns all of that: feed() takes
// each stream's NEW samples (any amount, also none), puts them behind the stream's unconsumed
// tail, runs the loop as far as the data allows and hands back what that made.  Whatever the
// cuts, the concatenated results are those of one call over the whole streams, bit for bit
// (tests/test_gpu_session.py).
//
// Two kinds.  The host-tail session (the default) keeps each stream's unconsumed samples in host
// memory and uploads all of them with every feed.  The resident session (MIFSK_SESSION_RESIDENT)
// keeps them on the device in one of two row buffers: a feed uploads the new samples only -- as
// PCM16 when they are PCM16 -- or takes them from device memory, session_append_kernel
// (mifsk_ingest.hip) builds every row in the other buffer, and the host keeps integers.  Both are
// one driver, feed(): the integers and every check that needs no device are the book's
// (mifsk_session_book.cpp), and only how the rows get to the device has two bodies.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"
#include "mifsk_outputs.h"
#include "mifsk_session_book.h"

using mifsk::DevMem;
using mifsk::PinMem;
using mifsk::kNumOutArrays;
using mifsk::kOutArrays;

namespace {

constexpr size_t out_index( size_t member )
{
    size_t i = 0;
    while ( kOutArrays[i].member != member )
	i++;
    return i;
}

// where a per-stream count is in the packed block of them: behind the table's counts before it
constexpr size_t count_slot( size_t member )
{
    size_t slot = 0;
    for ( size_t i = 0; i < out_index(member); i++ )
	slot += kOutArrays[i].per == mifsk::kOne;
    return slot;
}

// The result arrays by name, for the fill of mifsk_session_result (run_slab) and the two that are
// special: the frame records are optional, the carrier band starts as -1.
constexpr size_t kBytes = out_index(offsetof(mifsk_demod_io, d_bytes)), kBits = out_index(offsetof(mifsk_demod_io, d_bits)),
		 kFrames = out_index(offsetof(mifsk_demod_io, d_frames)), kEpisodes = out_index(offsetof(mifsk_demod_io, d_episodes));
constexpr size_t kNBytes = count_slot(offsetof(mifsk_demod_io, d_nbytes)), kNFrames = count_slot(offsetof(mifsk_demod_io, d_nframes)),
		 kNEpisodes = count_slot(offsetof(mifsk_demod_io, d_nepisodes)), kStatus = count_slot(offsetof(mifsk_demod_io, d_status)),
		 kCarrierBand = count_slot(offsetof(mifsk_demod_io, d_carrier_band));
constexpr size_t kNumCounts = kCarrierBand + 1;		// (the last: one fill of zeros in front of it)

} // namespace

struct mifsk_session {
    mifsk_ctx		*ctx = nullptr;
    mifsk_rx_config	cfg;
    int			n;
    unsigned		flags = 0;
    bool		want_frames = false, ring = false, resident;
    // per stream: where what is held starts in the stream, how much is held, who is done
    mifsk::SessionBook	book;
    mifsk::FeedPlan	plan;				// (of the feed that runs)
    std::vector<uint64_t>	base;			// the loop's cursors and FINISHED flags, for the book
    std::vector<uint8_t>	fin;
    std::vector<std::vector<float>>	tail;		// host-tail: the samples held
    // device: loop state, RING cells, the rows of a feed and its outputs
    DevMem<mifsk_stream_state>	d_state;
    DevMem<float>		d_ring;
    DevMem<float>		d_rows;
    DevMem<uint32_t>		d_lens, d_counts;	// counts: the table's per-stream counts, one block
    DevMem<uint64_t>		d_origin;
    DevMem<uint8_t>		d_out[kNumOutArrays];	// the table's other arrays
    // host (page-locked): staging of the rows, the results of the last feed
    PinMem<float>		h_rows;
    PinMem<uint32_t>		h_lens, h_counts;
    PinMem<uint64_t>		h_origin;
    PinMem<uint8_t>		h_out[kNumOutArrays];
    PinMem<mifsk_stream_state>	h_state;
    std::vector<mifsk_session_result>	results;
    // what info_get reports
    uint32_t			feeds = 0;
    uint64_t			h2d_last = 0, h2d_total = 0;
    // MIFSK_SESSION_RESIDENT
    DevMem<float>		rows[2];		// [n][row_cap] each; rows[cur] holds the tails
    size_t			row_cap = 0;
    int				cur = 0;
    PinMem<uint8_t>		h_stage;		// a feed's table, then its new pieces
    DevMem<uint8_t>		d_stage;
    mifsk::HipEvent		ev_producer;		// feed_device: the producer's stream at the call
    // (the last member: synchronised and destroyed before any buffer above is freed)
    mifsk::HipStream		stream;

    mifsk_session( int n_, bool resident_ )		// (may throw std::bad_alloc)
	: n(n_), resident(resident_), book((size_t)n_, resident_ ? mifsk::kResidentPolicy : mifsk::kHostTailPolicy),
	  base((size_t)n_), fin((size_t)n_), tail(resident_ ? 0 : (size_t)n_), results((size_t)n_) {}
};

namespace {

bool wanted( const mifsk_session *s, size_t i )
{
    return kOutArrays[i].per != mifsk::kCounters && ( i != kFrames || s->want_frames );
}

// The arrays a feed of `width` samples per row needs behind the rows, and `io` with the capacities
// and the result pointers: the counts into their block, the others to arrays of their own.
int fit_outputs( mifsk_session *s, size_t width, mifsk_demod_io &io )
{
    const size_t n = (size_t)s->n;
    std::memset(&io, 0, sizeof(io));
    io.frames_cap = mifsk_max_frames(&s->cfg, width);
    io.episodes_cap = mifsk_max_episodes(&s->cfg, width);
    int rc = 0;
    if ( ( rc = s->d_lens.fit(n) ) || ( rc = s->d_origin.fit(n) ) || ( rc = s->h_state.fit(n) )
	    || ( rc = s->h_counts.fit(kNumCounts * n) ) || ( rc = s->d_counts.fit(kNumCounts * n) ) )
	return rc;
    size_t slot = 0;
    for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	if ( !wanted(s, i) )
	    continue;
	if ( kOutArrays[i].per == mifsk::kOne ) {
	    mifsk::out_set(io, kOutArrays[i], s->d_counts.p + n * slot++);
	    continue;
	}
	const size_t bytes = n * mifsk::out_row_bytes(io, kOutArrays[i]);
	if ( ( rc = s->d_out[i].fit(bytes) ) || ( rc = s->h_out[i].fit(bytes) ) )
	    return rc;
	mifsk::out_set(io, kOutArrays[i], s->d_out[i].p);
    }
    return 0;
}

// Everything behind the rows, for both kinds of session: the loop over d_rows ([n][stride], the
// first `width` of each row, lengths in d_lens, origins in d_origin -- all enqueued on the
// session's stream before) into the arrays of `io` (fit_outputs), the copy back, the results.
// h_state holds the loop's state after.
int run_slab( mifsk_session *s, mifsk_demod_io &io, const float *d_rows, size_t stride, size_t width, int final )
{
    const size_t n = (size_t)s->n, fc = io.frames_cap, ec = io.episodes_cap;
    hipStream_t st = s->stream;
    HIP_OK(hipMemsetAsync(s->d_counts.p, 0, kCarrierBand * n * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(s->d_counts.p + kCarrierBand * n, 0xFF, n * sizeof(uint32_t), st));	// carrier_band: -1
    io.d_samples = d_rows;
    io.stream_stride = stride;
    io.d_nsamples = s->d_lens.p;
    io.nsamples = (uint32_t)width;
    io.nstreams = s->n;
    io.flags = s->flags | ( s->ring ? MIFSK_IO_RING_EXACT : 0u );
    const int rc = s->ring ? mifsk_demod_slab_ring(s->ctx, &s->cfg, &io, s->d_state.p, s->d_origin.p, s->d_ring.p, final ? 1 : 0, st)
			   : mifsk_demod_slab(s->ctx, &s->cfg, &io, s->d_state.p, s->d_origin.p, final ? 1 : 0, st);
    if ( rc != 0 )
	return rc;
    HIP_OK(hipMemcpyAsync(s->h_counts.p, s->d_counts.p, kNumCounts * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(s->h_state.p, s->d_state.p, n * sizeof(mifsk_stream_state), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    size_t most[mifsk::kCounters + 1] = {};		// per PerRow: the columns that hold something
    const uint32_t *cnt = s->h_counts.p;
    for ( size_t i = 0; i < n; i++ ) {
	mifsk_session_result &r = s->results[i];
	std::memset(&r, 0, sizeof(r));
	r.nframes = cnt[kNFrames * n + i];
	r.nbytes = cnt[kNBytes * n + i];
	r.nepisodes = cnt[kNEpisodes * n + i];
	r.status = cnt[kStatus * n + i];
	r.carrier_band = (int32_t)cnt[kCarrierBand * n + i];
	most[mifsk::kFramesCap] = std::max<size_t>(most[mifsk::kFramesCap], std::max(r.nframes, r.nbytes));
	most[mifsk::kEpisodesCap] = std::max<size_t>(most[mifsk::kEpisodesCap], r.nepisodes);
	if ( r.nframes > fc ) r.nframes = (uint32_t)fc;		// (what the arrays hold; status says it was cut:
	if ( r.nbytes > fc ) r.nbytes = (uint32_t)fc;		// the counts keep counting past the capacity)
	if ( r.nepisodes > ec ) r.nepisodes = (uint32_t)ec;
	r.bits = reinterpret_cast<const uint64_t *>(s->h_out[kBits].p) + i * fc;
	r.bytes = s->h_out[kBytes].p + i * fc;
	r.frames = s->want_frames ? reinterpret_cast<const mifsk_frame *>(s->h_out[kFrames].p) + i * fc : nullptr;
	r.episodes = reinterpret_cast<const mifsk_episode *>(s->h_out[kEpisodes].p) + i * ec;
	const mifsk_stream_state &ss = s->h_state.p[i];
	r.consumed = s->base[i] = ss.base;
	r.finished = s->fin[i] = ( ss.flags & MIFSK_STATE_FINISHED ) ? 1u : 0u;
    }
    most[mifsk::kFramesCap] = std::min(most[mifsk::kFramesCap], fc);
    most[mifsk::kEpisodesCap] = std::min(most[mifsk::kEpisodesCap], ec);
    for ( size_t i = 0; i < kNumOutArrays; i++ ) {
	const size_t row = mifsk::out_row_bytes(io, kOutArrays[i]), cols = most[kOutArrays[i].per] * kOutArrays[i].esz;
	if ( wanted(s, i) && cols )
	    HIP_OK(hipMemcpy2DAsync(s->h_out[i].p, row, s->d_out[i].p, row, cols, n, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

// A pair of row buffers a feed grows into.  The feed's kernels read the old pair and write this
// one, so whichever pair loses is freed only behind the stream: here when the feed fails, by the
// feed itself when it has synchronised.
struct GrownRows {
    hipStream_t	st;
    DevMem<float>	p[2];
    explicit GrownRows( hipStream_t st_ ) : st(st_) {}
    int alloc( size_t floats )
    {
	if ( const int rc = p[0].alloc(floats) )
	    return rc;
	return p[1].alloc(floats);
    }
    ~GrownRows()
    {
	if ( p[0].p || p[1].p )
	    (void)hipStreamSynchronize(st);	// (then the members free)
    }
};

// what the caller passes beside the samples' place (mifsk_session_feed_ex, _feed_device)
struct FeedExtras {
    float	rxnoise = 0.0f;
    void	*producer = nullptr;
};

// Build rows, host-tail: kept floats and new floats into the pinned rows, then the upload.
int rows_host_tail( mifsk_session *s, const mifsk::FeedSource &src, uint64_t &h2d )
{
    const size_t n = (size_t)s->n, width = (size_t)s->plan.width;
    for ( size_t i = 0; i < n; i++ ) {
	const mifsk::FeedRow &r = s->plan.rows[i];
	float *row = s->h_rows.p + i * width;
	if ( r.keep )
	    std::memcpy(row, s->tail[i].data() + r.drop, r.keep * sizeof(float));
	if ( r.k )
	    std::memcpy(row + r.keep, src.host[i], r.k * sizeof(float));
	std::memset(row + r.keep + r.k, 0, ( width - r.keep - r.k ) * sizeof(float));
	s->h_lens.p[i] = r.keep + r.k;
	s->h_origin.p[i] = s->book.origin(i);
    }
    hipStream_t st = s->stream;
    HIP_OK(hipMemcpyAsync(s->d_rows.p, s->h_rows.p, n * width * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->d_lens.p, s->h_lens.p, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->d_origin.p, s->h_origin.p, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    h2d = n * ( width * sizeof(float) + sizeof(uint32_t) + sizeof(uint64_t) );
    return 0;
}

// Build rows, resident: the table and (host pieces, packed in their own element type) the new
// samples in one upload, then session_append_kernel from rows[cur] into `dst`.
int rows_resident( mifsk_session *s, const mifsk::FeedSource &src, const FeedExtras &ex, float *dst, size_t dst_cap,
	uint64_t &h2d )
{
    const size_t n = (size_t)s->n, table_bytes = n * sizeof(mifsk::SessionRow);	// (a multiple of 16)
    const mifsk::FeedPlan &plan = s->plan;
    mifsk::SessionRow *table = reinterpret_cast<mifsk::SessionRow *>(s->h_stage.p);
    uint8_t *pieces = s->h_stage.p + table_bytes;
    for ( size_t i = 0; i < n; i++ ) {
	const mifsk::FeedRow &r = plan.rows[i];
	table[i] = mifsk::SessionRow{src.on_device ? (uint64_t)i * src.stride : r.off / plan.esz, s->book.origin(i),
				     r.drop, r.keep, r.k, 0u};
	if ( r.k && !src.on_device )
	    std::memcpy(pieces + r.off, src.host[i], r.k * plan.esz);
    }
    hipStream_t st = s->stream;
    h2d = src.on_device ? table_bytes : table_bytes + plan.piece_bytes;
    HIP_OK(hipMemcpyAsync(s->d_stage.p, s->h_stage.p, h2d, hipMemcpyHostToDevice, st));
    if ( src.on_device && ex.producer != MIFSK_PIPELINE_NO_PRODUCER ) {
	// the samples were written on the caller's stream: wait for the point it has reached
	HIP_OK(hipEventRecord(s->ev_producer, (hipStream_t)ex.producer));
	HIP_OK(hipStreamWaitEvent(st, s->ev_producer, 0));
    }
    return mifsk::launch_session_append(s->rows[s->cur].p, s->row_cap, dst, dst_cap, (uint32_t)plan.width,
					src.on_device ? src.device : (const void *)( s->d_stage.p + table_bytes ),
					src.kind == MIFSK_FEED_S16, reinterpret_cast<const mifsk::SessionRow *>(s->d_stage.p),
					s->d_lens.p, s->d_origin.p, s->n, mifsk::rxnoise_term(ex.rxnoise), st);
}

// A feed, of either kind of session and from any source.  Everything that can fail comes before
// the commit: a feed that fails or is refused leaves the session as it was.
int feed( mifsk_session *s, const mifsk::FeedSource &src, const FeedExtras &ex, int final )
{
    // 1. plan
    int rc = s->book.plan(src, s->plan);
    if ( rc != 0 )
	return rc;
    const size_t n = (size_t)s->n, width = (size_t)s->plan.width;
    HIP_OK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->stream;
    // 2. fit
    mifsk_demod_io io;
    if ( ( rc = fit_outputs(s, width, io) ) )
	return rc;
    GrownRows grown(st);
    size_t new_cap = s->row_cap;
    if ( s->resident ) {
	const size_t up_bytes = n * sizeof(mifsk::SessionRow) + ( src.on_device ? 0 : (size_t)s->plan.piece_bytes );
	if ( ( rc = s->h_stage.fit(up_bytes) ) || ( rc = s->d_stage.fit(up_bytes) ) )
	    return rc;
	if ( width > s->row_cap ) {
	    new_cap = ( width + width / 4 + 3 ) & ~(size_t)3;	// (DevMem::fit's head-room)
	    if ( ( rc = grown.alloc(n * new_cap) ) )
		return rc;
	}
    } else {
	if ( ( rc = s->h_rows.fit(n * width) ) || ( rc = s->d_rows.fit(n * width) )
		|| ( rc = s->h_lens.fit(n) ) || ( rc = s->h_origin.fit(n) ) )
	    return rc;
	try {
	    for ( size_t i = 0; i < n; i++ )		// (phase 5 puts the row back within this)
		s->tail[i].reserve((size_t)s->plan.rows[i].keep + s->plan.rows[i].k);
	} catch ( const std::bad_alloc & ) {
	    return -ENOMEM;
	}
    }
    // 3. build rows
    float *d_rows = !s->resident ? s->d_rows.p : grown.p[0].p ? grown.p[0].p : s->rows[s->cur ^ 1].p;
    const size_t stride = s->resident ? new_cap : width;
    uint64_t h2d = 0;
    rc = s->resident ? rows_resident(s, src, ex, d_rows, stride, h2d) : rows_host_tail(s, src, h2d);
    // 4. the loop
    if ( rc == 0 )
	rc = run_slab(s, io, d_rows, stride, width, final);
    if ( rc != 0 ) {
	(void)hipStreamSynchronize(st);		// (the buffers and the caller's samples are read until here)
	return rc;
    }
    // 5. commit.  The stream has synchronised: a resident session's rows are in the other buffer,
    // of the new pair if it grew; a host-tail session's are what the loop left of its pinned rows.
    (void)s->book.commit(s->plan, s->base.data(), s->fin.data(), final != 0);	// (this feed's plan: it is taken)
    if ( grown.p[0].p ) {
	for ( int b = 0; b < 2; b++ )
	    s->rows[b] = std::move(grown.p[b]);
	s->row_cap = new_cap;
	s->cur = 0;
    } else if ( s->resident ) {
	s->cur ^= 1;
    }
    for ( size_t i = 0; i < s->tail.size(); i++ ) {
	const float *end = s->h_rows.p + i * width + s->plan.rows[i].keep + s->plan.rows[i].k;
	s->tail[i].assign(end - s->book.held(i), end);
    }
    s->feeds++;
    s->h2d_last = h2d;
    s->h2d_total += h2d;
    return 0;
}

} // namespace

extern "C" void mifsk_session_destroy( mifsk_session *s )
{
    if ( !s )
	return;
    if ( s->ctx )
	(void)hipSetDevice(s->ctx->device);
    delete s;					// (the stream first, then the buffers: they free themselves)
}

extern "C" int mifsk_session_create( mifsk_session **out, mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	int nstreams, unsigned flags )
{
    if ( !out )
	return -EINVAL;
    *out = nullptr;
    if ( !ctx || !cfg || nstreams <= 0 )
	return -EINVAL;
    if ( flags & ~( MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP | MIFSK_SESSION_WANT_FRAMES
		   | MIFSK_SESSION_RESIDENT ) )
	return -EINVAL;
    if ( ( flags & MIFSK_IO_ENGINE_WAVE ) && ( flags & MIFSK_IO_ENGINE_WORKGROUP ) )
	return -EINVAL;
    if ( ( flags & MIFSK_IO_RING_EXACT ) && ( flags & MIFSK_IO_ENGINE_WORKGROUP ) )
	return -EINVAL;				// (RING addressing is the wavefront engine's)
    int rc = mifsk_check_cfg(cfg);
    if ( rc != 0 )
	return rc;
    mifsk_session *s = nullptr;
    try {
	s = new mifsk_session(nstreams, ( flags & MIFSK_SESSION_RESIDENT ) != 0);
    } catch ( const std::bad_alloc & ) {
	return -ENOMEM;
    }
    s->ctx = ctx;
    s->cfg = *cfg;
    s->flags = flags & ( MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP );
    s->want_frames = ( flags & MIFSK_SESSION_WANT_FRAMES ) != 0;
    s->ring = ( flags & MIFSK_IO_RING_EXACT ) != 0;
    rc = -EIO;
    if ( hipSetDevice(ctx->device) == hipSuccess
	    && s->stream.make() == 0 ) {
	rc = s->d_state.fit((size_t)nstreams);
	if ( rc == 0 && hipMemsetAsync(s->d_state.p, 0, (size_t)nstreams * sizeof(mifsk_stream_state), s->stream) != hipSuccess )
	    rc = -EIO;				// (all zero: a new stream)
	if ( rc == 0 && s->ring ) {
	    const size_t nf = mifsk_ring_floats(cfg) * (size_t)nstreams;
	    rc = s->d_ring.fit(nf);
	    if ( rc == 0 && hipMemsetAsync(s->d_ring.p, 0, nf * sizeof(float), s->stream) != hipSuccess )
		rc = -EIO;
	}
	if ( rc == 0 && s->resident )
	    rc = s->ev_producer.make();
    }
    if ( rc != 0 ) {
	mifsk_session_destroy(s);
	return rc;
    }
    *out = s;
    return 0;
}

// The four feeds: how each one's arguments say where the new samples are.

extern "C" int mifsk_session_feed( mifsk_session *s, const float *const *samples, const uint32_t *nsamples, int final )
{
    if ( !s )
	return -EINVAL;
    mifsk::FeedSource src;
    src.nsamples = nsamples;
    src.host = reinterpret_cast<const void *const *>(samples);
    return feed(s, src, FeedExtras{}, final);
}

extern "C" int mifsk_session_feed_ex( mifsk_session *s, const void *const *samples, const uint32_t *nsamples,
	unsigned kind, float rxnoise, int final )
{
    if ( !s || !s->resident )
	return -EINVAL;
    mifsk::FeedSource src;
    src.nsamples = nsamples;
    src.host = samples;
    src.kind = kind;
    return feed(s, src, FeedExtras{rxnoise, nullptr}, final);
}

extern "C" int mifsk_session_feed_device( mifsk_session *s, const void *d_samples, size_t stride,
	const uint32_t *nsamples, unsigned kind, float rxnoise, int final, void *producer )
{
    if ( !s || !s->resident )
	return -EINVAL;
    mifsk::FeedSource src;
    src.nsamples = nsamples;
    src.device = d_samples;
    src.stride = stride;
    src.on_device = true;
    src.kind = kind;
    return feed(s, src, FeedExtras{rxnoise, producer}, final);
}

extern "C" int mifsk_session_info_get( const mifsk_session *s, mifsk_session_info *info )
{
    if ( !s || !info )
	return -EINVAL;
    std::memset(info, 0, sizeof(*info));
    info->resident = s->resident ? 1u : 0u;
    info->feeds = s->feeds;
    info->row_capacity = s->row_cap;
    info->device_bytes = 2 * (uint64_t)s->n * s->row_cap * sizeof(float) + s->d_stage.cap
	+ s->d_state.cap * sizeof(mifsk_stream_state) + ( s->d_ring.cap + s->d_rows.cap ) * sizeof(float)
	+ ( s->d_lens.cap + s->d_counts.cap ) * sizeof(uint32_t) + s->d_origin.cap * sizeof(uint64_t);
    for ( const DevMem<uint8_t> &m : s->d_out )
	info->device_bytes += m.cap;
    info->h2d_bytes_last = s->h2d_last;
    info->h2d_bytes_total = s->h2d_total;
    return 0;
}

extern "C" const mifsk_session_result *mifsk_session_get( const mifsk_session *s, int stream )
{
    if ( !s || stream < 0 || stream >= s->n )
	return nullptr;
    return &s->results[(size_t)stream];
}

extern "C" size_t mifsk_session_pending( const mifsk_session *s, int stream )
{
    if ( !s || stream < 0 || stream >= s->n )
	return 0;
    return s->book.held((size_t)stream);
}
