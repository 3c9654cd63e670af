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
// (mifsk_ingest.hip) builds every row in the other buffer, and the host keeps integers.  Behind
// the rows both kinds run the same code: run_slab().
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

using mifsk::DevMem;
using mifsk::PinMem;

struct mifsk_session {
    mifsk_ctx		*ctx = nullptr;
    mifsk_rx_config	cfg;
    int			n = 0;
    unsigned		flags = 0;
    bool		want_frames = false, ring = false, finished = false;
    hipStream_t		stream = nullptr;
    // per stream: what the loop has not passed yet, and where that starts in the stream
    std::vector<std::vector<float>>	tail;
    std::vector<uint64_t>		origin;
    // device: loop state, RING cells, the rows of a feed and its outputs
    DevMem<mifsk_stream_state>	d_state;
    DevMem<float>		d_ring;
    DevMem<float>		d_rows;
    DevMem<uint32_t>		d_lens, d_counts;	// counts: nframes | nbytes | nepisodes | status | carrier_band
    DevMem<uint64_t>		d_origin, d_bits;
    DevMem<uint8_t>		d_bytes;
    DevMem<mifsk_frame>		d_frames;
    DevMem<mifsk_episode>	d_eps;
    // host (page-locked): staging of the rows, the results of the last feed
    PinMem<float>		h_rows;
    PinMem<uint32_t>		h_lens, h_counts;
    PinMem<uint64_t>		h_origin, h_bits;
    PinMem<uint8_t>		h_bytes;
    PinMem<mifsk_frame>		h_frames;
    PinMem<mifsk_episode>	h_eps;
    PinMem<mifsk_stream_state>	h_state;
    size_t			fc = 0, ec = 0;		// capacities of the last feed's arrays
    std::vector<mifsk_session_result>	results;
    // what info_get reports
    uint32_t			feeds = 0;
    uint64_t			h2d_last = 0, h2d_total = 0;
    // MIFSK_SESSION_RESIDENT.  The host's mirror of a stream is integers: `origin` above, the
    // samples held and where they start in the row (what the loop passed in the feed before is
    // still in front of them until the next feed compacts the row), and whether the loop is done
    // with the stream
    struct Held { uint32_t len, skip; bool done; };
    bool			resident = false;
    std::vector<Held>		held;
    DevMem<float>		rows[2];		// [n][row_cap] each; rows[cur] holds the tails
    size_t			row_cap = 0;
    int				cur = 0;
    PinMem<uint8_t>		h_stage;		// a feed's table, then its new pieces
    DevMem<uint8_t>		d_stage;
    hipEvent_t			ev_producer = nullptr;	// feed_device: the producer's stream at the call
};

namespace {

constexpr uint64_t kMaxRow = 0xFFFFF000ull;	// samples a row may hold (the kernels index rows in 32 bits)

inline size_t up16( size_t v ) { return ( v + 15 ) & ~(size_t)15; }

void note_h2d( mifsk_session *s, uint64_t bytes )
{
    s->feeds++;
    s->h2d_last = bytes;
    s->h2d_total += bytes;
}

// the arrays a feed of `width` samples per row needs behind the rows; fc / ec: their capacities
int fit_outputs( mifsk_session *s, size_t width, size_t &fc, size_t &ec )
{
    const size_t n = (size_t)s->n;
    fc = mifsk_max_frames(&s->cfg, width);
    ec = mifsk_max_episodes(&s->cfg, width);
    int rc = 0;
    if ( ( rc = s->d_lens.fit(n) ) || ( rc = s->d_origin.fit(n) )
	    || ( rc = s->h_counts.fit(5 * n) ) || ( rc = s->d_counts.fit(5 * n) )
	    || ( rc = s->h_state.fit(n) )
	    || ( rc = s->d_bits.fit(n * fc) ) || ( rc = s->h_bits.fit(n * fc) )
	    || ( rc = s->d_bytes.fit(n * fc) ) || ( rc = s->h_bytes.fit(n * fc) )
	    || ( rc = s->d_eps.fit(n * ec) ) || ( rc = s->h_eps.fit(n * ec) ) )
	return rc;
    if ( s->want_frames && ( ( rc = s->d_frames.fit(n * fc) ) || ( rc = s->h_frames.fit(n * fc) ) ) )
	return rc;
    return 0;
}

// Everything behind the rows, for both kinds of session: the loop over d_rows ([n][stride], the
// first `width` of each row, lengths in d_lens, origins in d_origin -- all enqueued on the
// session's stream before), the copy back, the results.  h_state holds the loop's state after.
int run_slab( mifsk_session *s, const float *d_rows, size_t stride, size_t width, size_t fc, size_t ec, int final )
{
    const size_t n = (size_t)s->n;
    hipStream_t st = s->stream;
    HIP_OK(hipMemsetAsync(s->d_counts.p, 0, 4 * n * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(s->d_counts.p + 4 * n, 0xFF, n * sizeof(uint32_t), st));	// carrier_band: -1

    mifsk_demod_io io;
    std::memset(&io, 0, sizeof(io));
    io.d_samples = d_rows;
    io.stream_stride = stride;
    io.d_nsamples = s->d_lens.p;
    io.nsamples = (uint32_t)width;
    io.nstreams = s->n;
    io.d_bytes = s->d_bytes.p;
    io.d_bits = s->d_bits.p;
    io.d_frames = s->want_frames ? s->d_frames.p : nullptr;
    io.frames_cap = fc;
    io.d_episodes = s->d_eps.p;
    io.episodes_cap = ec;
    io.d_nframes = s->d_counts.p;
    io.d_nbytes = s->d_counts.p + n;
    io.d_nepisodes = s->d_counts.p + 2 * n;
    io.d_status = s->d_counts.p + 3 * n;
    io.d_carrier_band = reinterpret_cast<int32_t *>(s->d_counts.p + 4 * n);
    io.flags = s->flags | ( s->ring ? MIFSK_IO_RING_EXACT : 0u );
    const int rc = s->ring ? mifsk_demod_slab_ring(s->ctx, &s->cfg, &io, s->d_state.p, s->d_origin.p, s->d_ring.p, final ? 1 : 0, st)
			   : mifsk_demod_slab(s->ctx, &s->cfg, &io, s->d_state.p, s->d_origin.p, final ? 1 : 0, st);
    if ( rc != 0 )
	return rc;
    HIP_OK(hipMemcpyAsync(s->h_counts.p, s->d_counts.p, 5 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(s->h_state.p, s->d_state.p, n * sizeof(mifsk_stream_state), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // the columns that hold something (counts keep counting past the capacity)
    size_t mf = 0, mb = 0, me = 0;
    for ( size_t i = 0; i < n; i++ ) {
	const size_t nf = s->h_counts.p[i], nb = s->h_counts.p[n + i], ne = s->h_counts.p[2 * n + i];
	mf = nf > mf ? nf : mf;
	mb = nb > mb ? nb : mb;
	me = ne > me ? ne : me;
    }
    mf = mf < fc ? mf : fc;
    mb = mb < fc ? mb : fc;
    me = me < ec ? me : ec;
    if ( mf )
	HIP_OK(hipMemcpy2DAsync(s->h_bits.p, fc * sizeof(uint64_t), s->d_bits.p, fc * sizeof(uint64_t),
				mf * sizeof(uint64_t), n, hipMemcpyDeviceToHost, st));
    if ( mf && s->want_frames )
	HIP_OK(hipMemcpy2DAsync(s->h_frames.p, fc * sizeof(mifsk_frame), s->d_frames.p, fc * sizeof(mifsk_frame),
				mf * sizeof(mifsk_frame), n, hipMemcpyDeviceToHost, st));
    if ( mb )
	HIP_OK(hipMemcpy2DAsync(s->h_bytes.p, fc, s->d_bytes.p, fc, mb, n, hipMemcpyDeviceToHost, st));
    if ( me )
	HIP_OK(hipMemcpy2DAsync(s->h_eps.p, ec * sizeof(mifsk_episode), s->d_eps.p, ec * sizeof(mifsk_episode),
				me * sizeof(mifsk_episode), n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    s->fc = fc;
    s->ec = ec;
    for ( size_t i = 0; i < n; i++ ) {
	mifsk_session_result &r = s->results[i];
	std::memset(&r, 0, sizeof(r));
	r.nframes = s->h_counts.p[i];
	r.nbytes = s->h_counts.p[n + i];
	r.nepisodes = s->h_counts.p[2 * n + i];
	r.status = s->h_counts.p[3 * n + i];
	r.carrier_band = (int32_t)s->h_counts.p[4 * n + i];
	if ( r.nframes > fc ) r.nframes = (uint32_t)fc;		// (what the arrays hold; status says it was cut)
	if ( r.nbytes > fc ) r.nbytes = (uint32_t)fc;
	if ( r.nepisodes > ec ) r.nepisodes = (uint32_t)ec;
	r.bits = s->h_bits.p + i * fc;
	r.bytes = s->h_bytes.p + i * fc;
	r.frames = s->want_frames ? s->h_frames.p + i * fc : nullptr;
	r.episodes = s->h_eps.p + i * ec;
	const mifsk_stream_state &ss = s->h_state.p[i];
	r.consumed = ss.base;
	r.finished = ( ss.flags & MIFSK_STATE_FINISHED ) ? 1u : 0u;
    }
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

// A feed of a resident session: the new samples are host pieces (`host`, packed into the pinned
// staging buffer and uploaded in their own element type) or rows of one device array (`d_fresh`,
// `stride` elements apart).  Nothing of the session changes before the loop has run.
int feed_resident( mifsk_session *s, const void *const *host, const void *d_fresh, size_t stride, bool device,
	const uint32_t *nsamples, unsigned kind, float rxnoise, int final, void *producer )
{
    if ( !s->resident || s->finished )
	return -EINVAL;				// (finished: the final piece has been fed)
    if ( kind != MIFSK_FEED_F32 && kind != MIFSK_FEED_S16 )
	return -EINVAL;
    const size_t n = (size_t)s->n;
    const size_t esz = kind == MIFSK_FEED_S16 ? sizeof(int16_t) : sizeof(float);
    const size_t table_bytes = n * sizeof(mifsk::SessionRow);	// (a multiple of 16)
    size_t width = 4, piece_bytes = 0;
    for ( size_t i = 0; i < n; i++ ) {
	const uint32_t k = nsamples ? nsamples[i] : 0u;
	if ( k && ( device ? ( !d_fresh || k > stride ) : ( !host || !host[i] ) ) )
	    return -EINVAL;
	if ( s->held[i].done )
	    continue;				// a finished stream: later samples are ignored
	const uint64_t len = (uint64_t)s->held[i].len + k;
	if ( len > kMaxRow )
	    return -EOVERFLOW;
	width = len > width ? (size_t)len : width;
	piece_bytes = up16(piece_bytes) + k * esz;
    }
    width = ( width + 3 ) & ~(size_t)3;
    HIP_OK(hipSetDevice(s->ctx->device));
    hipStream_t st = s->stream;
    const size_t up_bytes = device ? table_bytes : table_bytes + up16(piece_bytes);
    size_t fc = 0, ec = 0;
    int rc = 0;
    if ( ( rc = s->h_stage.fit(up_bytes) ) || ( rc = s->d_stage.fit(up_bytes) ) || ( rc = fit_outputs(s, width, fc, ec) ) )
	return rc;
    GrownRows grown(st);
    size_t new_cap = s->row_cap;
    if ( width > s->row_cap ) {
	new_cap = ( width + width / 4 + 3 ) & ~(size_t)3;	// (DevMem::fit's head-room)
	if ( ( rc = grown.alloc(n * new_cap) ) )
	    return rc;
    }
    float *dst = grown.p[0].p ? grown.p[0].p : s->rows[s->cur ^ 1].p;

    mifsk::SessionRow *table = reinterpret_cast<mifsk::SessionRow *>(s->h_stage.p);
    uint8_t *pieces = s->h_stage.p + table_bytes;
    size_t off = 0;
    for ( size_t i = 0; i < n; i++ ) {
	const mifsk_session::Held &h = s->held[i];
	const uint32_t k = nsamples && !h.done ? nsamples[i] : 0u;
	mifsk::SessionRow &r = table[i];
	off = up16(off);
	r.src_off = device ? (uint64_t)i * stride : (uint64_t)( off / esz );
	r.origin = s->origin[i];
	r.drop = h.skip;
	r.keep = h.len;
	r.k = k;
	r.reserved = 0;
	if ( k && !device )
	    std::memcpy(pieces + off, host[i], k * esz);
	off += k * esz;
    }
    HIP_OK(hipMemcpyAsync(s->d_stage.p, s->h_stage.p, up_bytes, hipMemcpyHostToDevice, st));
    if ( device && producer != MIFSK_PIPELINE_NO_PRODUCER ) {
	// the samples were written on the caller's stream: wait for the point it has reached
	HIP_OK(hipEventRecord(s->ev_producer, (hipStream_t)producer));
	HIP_OK(hipStreamWaitEvent(st, s->ev_producer, 0));
    }
    rc = mifsk::launch_session_append(s->rows[s->cur].p, s->row_cap, dst, new_cap, (uint32_t)width,
				      device ? d_fresh : (const void *)( s->d_stage.p + table_bytes ),
				      kind == MIFSK_FEED_S16, reinterpret_cast<const mifsk::SessionRow *>(s->d_stage.p),
				      s->d_lens.p, s->d_origin.p, s->n, mifsk::rxnoise_term(rxnoise), st);
    if ( rc == 0 )
	rc = run_slab(s, dst, new_cap, width, fc, ec, final);
    if ( rc != 0 ) {
	(void)hipStreamSynchronize(st);		// (the buffers and the caller's samples are read until here)
	return rc;
    }
    // the stream has synchronised: the rows are in the other buffer, of the new pair if it grew
    if ( grown.p[0].p ) {
	for ( int b = 0; b < 2; b++ )
	    s->rows[b] = std::move(grown.p[b]);
	s->row_cap = new_cap;
	s->cur = 0;
    } else {
	s->cur ^= 1;
    }
    for ( size_t i = 0; i < n; i++ ) {
	mifsk_session::Held &h = s->held[i];
	const mifsk_stream_state &ss = s->h_state.p[i];
	h.len = table[i].keep + table[i].k;
	h.skip = 0;
	// everything before the cursor has been passed for good; the next feed drops it
	if ( ss.base > s->origin[i] ) {
	    const uint64_t passed = ss.base - s->origin[i];
	    h.skip = passed < h.len ? (uint32_t)passed : h.len;
	    h.len -= h.skip;
	    s->origin[i] += h.skip;
	}
	if ( ss.flags & MIFSK_STATE_FINISHED ) {
	    h.len = h.skip = 0;			// --rx-one, an aborted loop, the final feed: nothing is held
	    h.done = true;
	}
    }
    note_h2d(s, up_bytes);
    if ( final )
	s->finished = true;
    return 0;
}

} // namespace

extern "C" void mifsk_session_destroy( mifsk_session *s )
{
    if ( !s )
	return;
    if ( s->ctx )
	(void)hipSetDevice(s->ctx->device);
    if ( s->stream ) {
	(void)hipStreamSynchronize(s->stream);
	(void)hipStreamDestroy(s->stream);
    }
    if ( s->ev_producer ) (void)hipEventDestroy(s->ev_producer);
    delete s;					// (its buffers free themselves)
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
    mifsk_session *s = new (std::nothrow) mifsk_session;
    if ( !s )
	return -ENOMEM;
    s->ctx = ctx;
    s->cfg = *cfg;
    s->n = nstreams;
    s->flags = flags & ( MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP );
    s->want_frames = ( flags & MIFSK_SESSION_WANT_FRAMES ) != 0;
    s->ring = ( flags & MIFSK_IO_RING_EXACT ) != 0;
    s->resident = ( flags & MIFSK_SESSION_RESIDENT ) != 0;
    try {
	s->tail.resize((size_t)nstreams);
	s->origin.assign((size_t)nstreams, 0);
	s->results.resize((size_t)nstreams);
	if ( s->resident )
	    s->held.assign((size_t)nstreams, mifsk_session::Held{0u, 0u, false});
    } catch ( const std::bad_alloc & ) {
	delete s;
	return -ENOMEM;
    }
    rc = -EIO;
    if ( hipSetDevice(ctx->device) == hipSuccess
	    && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess ) {
	rc = s->d_state.fit((size_t)nstreams);
	if ( rc == 0 && hipMemsetAsync(s->d_state.p, 0, (size_t)nstreams * sizeof(mifsk_stream_state), s->stream) != hipSuccess )
	    rc = -EIO;				// (all zero: a new stream)
	if ( rc == 0 && s->ring ) {
	    const size_t nf = mifsk_ring_floats(cfg) * (size_t)nstreams;
	    rc = s->d_ring.fit(nf);
	    if ( rc == 0 && hipMemsetAsync(s->d_ring.p, 0, nf * sizeof(float), s->stream) != hipSuccess )
		rc = -EIO;
	}
	if ( rc == 0 && s->resident
		&& hipEventCreateWithFlags(&s->ev_producer, hipEventDisableTiming) != hipSuccess )
	    rc = -EIO;
    }
    if ( rc != 0 ) {
	mifsk_session_destroy(s);
	return rc;
    }
    *out = s;
    return 0;
}

extern "C" int mifsk_session_feed( mifsk_session *s, const float *const *samples, const uint32_t *nsamples, int final )
{
    if ( !s )
	return -EINVAL;
    if ( s->resident )
	return feed_resident(s, reinterpret_cast<const void *const *>(samples), nullptr, 0, false, nsamples,
			     MIFSK_FEED_F32, 0.0f, final, nullptr);
    if ( s->finished )
	return -EINVAL;				// the final piece has been fed
    const size_t n = (size_t)s->n;
    HIP_OK(hipSetDevice(s->ctx->device));
    size_t width = 4;
    try {
	for ( size_t i = 0; i < n; i++ ) {
	    const uint32_t k = nsamples ? nsamples[i] : 0u;
	    if ( k && ( !samples || !samples[i] ) )
		return -EINVAL;
	    if ( k )
		s->tail[i].insert(s->tail[i].end(), samples[i], samples[i] + k);
	    if ( s->tail[i].size() > 0xFFFFFFF0ull )
		return -EOVERFLOW;
	    width = s->tail[i].size() > width ? s->tail[i].size() : width;
	}
    } catch ( const std::bad_alloc & ) {
	return -ENOMEM;
    }
    width = ( width + 3 ) & ~(size_t)3;
    size_t fc = 0, ec = 0;
    int rc = 0;
    if ( ( rc = s->h_rows.fit(n * width) ) || ( rc = s->d_rows.fit(n * width) )
	    || ( rc = s->h_lens.fit(n) ) || ( rc = s->h_origin.fit(n) ) || ( rc = fit_outputs(s, width, fc, ec) ) )
	return rc;
    for ( size_t i = 0; i < n; i++ ) {
	float *row = s->h_rows.p + i * width;
	const size_t k = s->tail[i].size();
	if ( k )
	    std::memcpy(row, s->tail[i].data(), k * sizeof(float));
	std::memset(row + k, 0, ( width - k ) * sizeof(float));
	s->h_lens.p[i] = (uint32_t)k;
	s->h_origin.p[i] = s->origin[i];
    }
    hipStream_t st = s->stream;
    HIP_OK(hipMemcpyAsync(s->d_rows.p, s->h_rows.p, n * width * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->d_lens.p, s->h_lens.p, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s->d_origin.p, s->h_origin.p, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if ( ( rc = run_slab(s, s->d_rows.p, width, width, fc, ec, final) ) )
	return rc;
    note_h2d(s, n * ( width * sizeof(float) + sizeof(uint32_t) + sizeof(uint64_t) ));
    for ( size_t i = 0; i < n; i++ ) {
	const mifsk_stream_state &ss = s->h_state.p[i];
	// everything before the cursor has been passed for good
	if ( ss.base > s->origin[i] ) {
	    size_t drop = (size_t)( ss.base - s->origin[i] );
	    if ( drop > s->tail[i].size() )
		drop = s->tail[i].size();
	    s->tail[i].erase(s->tail[i].begin(), s->tail[i].begin() + (long)drop);
	    s->origin[i] += drop;
	}
    }
    if ( final )
	s->finished = true;
    return 0;
}

extern "C" int mifsk_session_feed_ex( mifsk_session *s, const void *const *samples, const uint32_t *nsamples,
	unsigned kind, float rxnoise, int final )
{
    if ( !s )
	return -EINVAL;
    return feed_resident(s, samples, nullptr, 0, false, nsamples, kind, rxnoise, final, nullptr);
}

extern "C" int mifsk_session_feed_device( mifsk_session *s, const void *d_samples, size_t stride,
	const uint32_t *nsamples, unsigned kind, float rxnoise, int final, void *producer )
{
    if ( !s )
	return -EINVAL;
    return feed_resident(s, nullptr, d_samples, stride, true, nsamples, kind, rxnoise, final, producer);
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
	+ ( s->d_lens.cap + s->d_counts.cap ) * sizeof(uint32_t) + ( s->d_origin.cap + s->d_bits.cap ) * sizeof(uint64_t)
	+ s->d_bytes.cap + s->d_frames.cap * sizeof(mifsk_frame) + s->d_eps.cap * sizeof(mifsk_episode);
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
    return s->resident ? s->held[(size_t)stream].len : s->tail[(size_t)stream].size();
}
