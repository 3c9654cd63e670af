// mifsk_mux_stream.hip -- the multiplexer fed in pieces (include/mifsk/mux_stream.h):
// mifsk_mux_stream_create / _destroy / _feed / _seek / _seen and the host's mifsk_mux_stream_drain.  A feed
// launches multiplex_kernel with STREAM = true (mifsk_mux_kernel.h, which says what a stream keeps and
// what the kernel does with it); the host logic that needs no device is in mifsk_mux_stream_check.h.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk/mux_stream.h"
#include "mifsk_mux_kernel.h"
#include "mifsk_mux_plan.h"
#include "mifsk_mux_stream_check.h"

struct mifsk_mux_stream {
    const mifsk_mux_plan			*plan;
    int						nstreams;
    bool					iq;		// input rows are (I, Q) pairs
    uint32_t					tail_cap;	// elements per row and side
    uint32_t					esz;		// bytes of an element
    unsigned					parity;		// the side the next feed reads
    mifsk::DevMem<mifsk::MuxStreamRecord>	rec;		// [2][nstreams]
    mifsk::DevMem<char>				tails;		// [2][nstreams * K][tail_cap] elements
};

extern "C" uint32_t mifsk_mux_stream_drain( uint32_t ntaps, uint32_t interp )
{
    return mifsk::mux_stream_drain(ntaps, interp);
}

extern "C" int mifsk_mux_stream_create( const mifsk_mux_plan *plan, int nstreams, uint32_t flags, mifsk_mux_stream **out )
{
    using namespace mifsk;
    if ( !plan || !out || nstreams <= 0 || ( flags & ~MIFSK_MUX_STREAM_IQ ) )
	return -EINVAL;
    std::unique_ptr<mifsk_mux_stream> ms(new (std::nothrow) mifsk_mux_stream);
    if ( !ms )
	return -ENOMEM;
    ms->plan = plan;
    ms->nstreams = nstreams;
    ms->iq = ( flags & MIFSK_MUX_STREAM_IQ ) != 0u;
    ms->esz = ms->iq ? 8u : 4u;
    ms->tail_cap = mux_stream_tail_cap(mux_stream_drain(plan->T, plan->L), ms->esz);
    ms->parity = 0u;
    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    if ( int rc = ms->rec.alloc(2u * (size_t)nstreams, 0, true) )
	return rc;
    if ( int rc = ms->tails.alloc(2u * (size_t)nstreams * plan->K * ms->tail_cap * ms->esz, 0, true) )
	return rc;
    *out = ms.release();
    return 0;
}

extern "C" void mifsk_mux_stream_destroy( mifsk_mux_stream *ms )
{
    if ( !ms )
	return;
    (void)hipSetDevice(ms->plan->device);
    (void)hipDeviceSynchronize();		// no kernel reads the tails any more
    delete ms;
}

extern "C" int mifsk_mux_stream_feed( mifsk_mux_stream *ms, const mifsk_mux_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ms || !io )
	return -EINVAL;
    const mifsk_mux_plan *plan = ms->plan;
    if ( int rc = mux_stream_feed_check(MuxStreamShape{plan->cx, plan->s16, ms->iq, plan->L, plan->K, ms->nstreams}, io) )
	return rc;

    MuxGeometry geo = {};
    MuxStreamArgs S = {mux_args(*plan, io, geo)};
    const size_t n = (size_t)ms->nstreams, side = n * plan->K * ms->tail_cap * ms->esz;
    S.rec_in = ms->rec.p + ms->parity * n;
    S.rec_out = ms->rec.p + ( ms->parity ^ 1u ) * n;
    S.tail_in = ms->tails.p + ms->parity * side;
    S.tail_out = ms->tails.p + ( ms->parity ^ 1u ) * side;
    S.tail_cap = ms->tail_cap;

    const int rc = mux_launch(*plan, geo, io->nstreams, S, ms->iq, (hipStream_t)stream);
    // (a feed that did not go out whole leaves the side it read as the current one)
    if ( rc == 0 )
	ms->parity ^= 1u;
    return rc;
}

extern "C" int mifsk_mux_stream_seek( mifsk_mux_stream *ms, const uint64_t *seen, void *stream )
{
    using namespace mifsk;
    if ( !ms )
	return -EINVAL;
    const size_t n = (size_t)ms->nstreams;
    const std::unique_ptr<MuxStreamRecord[]> rec(new (std::nothrow) MuxStreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    for ( size_t s = 0; s < n; s++ ) {
	if ( seen && seen[s] > kMuxStreamMaxSeen )
	    return -EINVAL;
	rec[s] = mux_stream_record_at(seen ? seen[s] : 0u);
    }
    // behind the feeds queued on `stream`; the records are there when this returns
    if ( hipSetDevice(ms->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    return hipMemcpy(ms->rec.p + ms->parity * n, rec.get(), n * sizeof(MuxStreamRecord), hipMemcpyHostToDevice) == hipSuccess
	? 0 : -EIO;
}

extern "C" int mifsk_mux_stream_seen( mifsk_mux_stream *ms, uint64_t *seen_out, void *stream )
{
    using namespace mifsk;
    if ( !ms || !seen_out )
	return -EINVAL;
    const size_t n = (size_t)ms->nstreams;
    const std::unique_ptr<MuxStreamRecord[]> rec(new (std::nothrow) MuxStreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    if ( hipSetDevice(ms->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    if ( hipMemcpy(rec.get(), ms->rec.p + ms->parity * n, n * sizeof(MuxStreamRecord), hipMemcpyDeviceToHost) != hipSuccess )
	return -EIO;
    for ( size_t s = 0; s < n; s++ )
	seen_out[s] = rec[s].seen;
    return 0;
}
