// mifsk_mux_stream.hip -- the multiplexer fed in pieces (include/mifsk/mux_stream.h):
// mifsk_mux_stream_create / _destroy / _feed / _seek / _seen and the host's mifsk_mux_stream_drain.  A feed
// launches multiplex_kernel with STREAM = true (mifsk_mux_kernel.h, which says what a stream keeps and
// what the kernel does with it); records and tails have their owner in mifsk_stream_state.h, and the host
// logic that needs no device is in mifsk_mux_stream_check.h.  gfx950 only.
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
#include "mifsk_stream_state.h"

struct mifsk_mux_stream {
    const mifsk_mux_plan			*plan;
    bool					iq;	// input rows are (I, Q) pairs
    mifsk::StreamState<mifsk::MuxStreamRecord>	st;	// K rows per stream, H elements of tail
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
    ms->iq = ( flags & MIFSK_MUX_STREAM_IQ ) != 0u;
    const uint32_t esz = ms->iq ? 8u : 4u;
    if ( int rc = ms->st.alloc(plan->device, nstreams, plan->K, stream_tail_room(mux_stream_drain(plan->T, plan->L), esz), esz) )
	return rc;
    *out = ms.release();
    return 0;
}

extern "C" void mifsk_mux_stream_destroy( mifsk_mux_stream *ms )
{
    if ( !ms )
	return;
    ms->st.quiesce();
    delete ms;
}

extern "C" int mifsk_mux_stream_feed( mifsk_mux_stream *ms, const mifsk_mux_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ms || !io )
	return -EINVAL;
    const mifsk_mux_plan *plan = ms->plan;
    if ( int rc = mux_stream_feed_check(MuxStreamShape{plan->cx, plan->s16, ms->iq, plan->L, plan->K, ms->st.nstreams}, io) )
	return rc;

    MuxGeometry geo = {};
    MuxStreamArgs S = {mux_args(*plan, io, geo), ms->st.sides()};
    const int rc = mux_launch(*plan, geo, io->nstreams, S, ms->iq, (hipStream_t)stream);
    if ( rc == 0 )
	ms->st.commit();
    return rc;
}

extern "C" int mifsk_mux_stream_seek( mifsk_mux_stream *ms, const uint64_t *seen, void *stream )
{
    using namespace mifsk;
    if ( !ms )
	return -EINVAL;
    return ms->st.seek(seen, kMuxStreamMaxSeen, mux_stream_record_at, (hipStream_t)stream);
}

extern "C" int mifsk_mux_stream_seen( mifsk_mux_stream *ms, uint64_t *seen_out, void *stream )
{
    if ( !ms || !seen_out )
	return -EINVAL;
    return ms->st.seen(seen_out, (hipStream_t)stream);
}
