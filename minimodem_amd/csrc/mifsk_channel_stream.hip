// mifsk_channel_stream.hip -- the channelizer fed in pieces (include/mifsk/channel_stream.h):
// mifsk_channel_stream_create / _destroy / _feed / _seek / _seen and the host's
// mifsk_channel_stream_outputs.  A feed launches channelize_kernel with STREAM = true
// (mifsk_channel_kernel.h, which says what a stream keeps and what the kernel does with it); records and
// tails have their owner in mifsk_stream_state.h, and the host logic that needs no device is in
// mifsk_channel_stream_check.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk/channel_stream.h"
#include "mifsk_channel_kernel.h"
#include "mifsk_channel_plan.h"
#include "mifsk_channel_stream_check.h"
#include "mifsk_stream_state.h"

struct mifsk_channel_stream {
    const mifsk_channel_plan			*plan;
    mifsk::StreamState<mifsk::StreamRecord>	st;	// one row per stream, T - 1 elements of tail
};

extern "C" uint64_t mifsk_channel_stream_outputs( uint32_t ntaps, uint32_t decim, uint64_t seen, uint64_t k )
{
    return mifsk::stream_outputs(ntaps, decim, seen, k);
}

extern "C" int mifsk_channel_stream_create( const mifsk_channel_plan *plan, int nstreams, mifsk_channel_stream **out )
{
    using namespace mifsk;
    if ( !plan || !out || nstreams <= 0 )
	return -EINVAL;
    std::unique_ptr<mifsk_channel_stream> cs(new (std::nothrow) mifsk_channel_stream);
    if ( !cs )
	return -ENOMEM;
    cs->plan = plan;
    const uint32_t esz = ( plan->s16 ? 2u : 4u ) * ( plan->cx ? 2u : 1u );
    if ( int rc = cs->st.alloc(plan->device, nstreams, 1u, stream_tail_room(plan->T - 1u, esz), esz) )
	return rc;
    *out = cs.release();
    return 0;
}

extern "C" void mifsk_channel_stream_destroy( mifsk_channel_stream *cs )
{
    if ( !cs )
	return;
    cs->st.quiesce();
    delete cs;
}

extern "C" int mifsk_channel_stream_feed( mifsk_channel_stream *cs, const mifsk_channel_io *io, uint32_t flags, void *stream )
{
    using namespace mifsk;
    if ( !cs || !io )
	return -EINVAL;
    const mifsk_channel_plan *plan = cs->plan;
    if ( int rc = stream_feed_check(StreamShape{plan->cx, plan->s16, plan->D, plan->K, cs->st.nstreams}, io, flags) )
	return rc;
    const bool iq = ( flags & MIFSK_CHANNEL_STREAM_IQ ) != 0u;

    const ChannelGeometry g = channel_geometry(*plan);
    ChannelStreamArgs S = {channel_args(*plan, io, g), cs->st.sides()};
    const int rc = channel_launch(*plan, g, io->out_stride, io->nstreams, S, iq, (hipStream_t)stream);
    if ( rc == 0 )
	cs->st.commit();
    return rc;
}

extern "C" int mifsk_channel_stream_seek( mifsk_channel_stream *cs, const uint64_t *seen, void *stream )
{
    using namespace mifsk;
    if ( !cs )
	return -EINVAL;
    const uint32_t D = cs->plan->D;
    return cs->st.seek(seen, kStreamMaxSeen, [D]( uint64_t n0 ) { return stream_record_at(D, n0); }, (hipStream_t)stream);
}

extern "C" int mifsk_channel_stream_seen( mifsk_channel_stream *cs, uint64_t *seen_out, void *stream )
{
    if ( !cs || !seen_out )
	return -EINVAL;
    return cs->st.seen(seen_out, (hipStream_t)stream);
}
