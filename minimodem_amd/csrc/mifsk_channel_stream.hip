// mifsk_channel_stream.hip -- the channelizer fed in pieces (include/mifsk/channel_stream.h):
// mifsk_channel_stream_create / _destroy / _feed / _seek / _seen and the host's
// mifsk_channel_stream_outputs.  A feed launches channelize_kernel with STREAM = true
// (mifsk_channel_kernel.h, which says what a stream keeps and what the kernel does with it); the host
// logic that needs no device is in mifsk_channel_stream_check.h.  gfx950 only.
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

struct mifsk_channel_stream {
    const mifsk_channel_plan		*plan;
    int					nstreams;
    uint32_t				tail_cap;	// elements per stream and side
    uint32_t				esz;		// bytes of an element
    unsigned				parity;		// the side the next feed reads
    mifsk::DevMem<mifsk::StreamRecord>	rec;		// [2][nstreams]
    mifsk::DevMem<char>			tails;		// [2][nstreams][tail_cap] elements
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
    cs->nstreams = nstreams;
    cs->esz = ( plan->s16 ? 2u : 4u ) * ( plan->cx ? 2u : 1u );
    cs->tail_cap = stream_tail_cap(plan->T, cs->esz);
    cs->parity = 0u;
    if ( hipSetDevice(plan->device) != hipSuccess )
	return -EIO;
    if ( int rc = cs->rec.alloc(2u * (size_t)nstreams, 0, true) )
	return rc;
    if ( int rc = cs->tails.alloc(2u * (size_t)nstreams * cs->tail_cap * cs->esz, 0, true) )
	return rc;
    *out = cs.release();
    return 0;
}

extern "C" void mifsk_channel_stream_destroy( mifsk_channel_stream *cs )
{
    if ( !cs )
	return;
    (void)hipSetDevice(cs->plan->device);
    (void)hipDeviceSynchronize();		// no kernel reads the tails any more
    delete cs;
}

extern "C" int mifsk_channel_stream_feed( mifsk_channel_stream *cs, const mifsk_channel_io *io, uint32_t flags, void *stream )
{
    using namespace mifsk;
    if ( !cs || !io )
	return -EINVAL;
    const mifsk_channel_plan *plan = cs->plan;
    if ( int rc = stream_feed_check(StreamShape{plan->cx, plan->s16, plan->D, plan->K, cs->nstreams}, io, flags) )
	return rc;
    const bool iq = ( flags & MIFSK_CHANNEL_STREAM_IQ ) != 0u;

    const ChannelGeometry g = channel_geometry(*plan);
    ChannelStreamArgs S = {channel_args(*plan, io, g)};
    const size_t n = (size_t)cs->nstreams, side = n * cs->tail_cap * cs->esz;
    S.rec_in = cs->rec.p + cs->parity * n;
    S.rec_out = cs->rec.p + ( cs->parity ^ 1u ) * n;
    S.tail_in = cs->tails.p + cs->parity * side;
    S.tail_out = cs->tails.p + ( cs->parity ^ 1u ) * side;
    S.tail_cap = cs->tail_cap;

    const int rc = channel_launch(*plan, g, io->out_stride, io->nstreams, S, iq, (hipStream_t)stream);
    // (a feed that did not go out whole leaves the side it read as the current one)
    if ( rc == 0 )
	cs->parity ^= 1u;
    return rc;
}

extern "C" int mifsk_channel_stream_seek( mifsk_channel_stream *cs, const uint64_t *seen, void *stream )
{
    using namespace mifsk;
    if ( !cs )
	return -EINVAL;
    const size_t n = (size_t)cs->nstreams;
    const std::unique_ptr<StreamRecord[]> rec(new (std::nothrow) StreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    for ( size_t s = 0; s < n; s++ ) {
	if ( seen && seen[s] > kStreamMaxSeen )
	    return -EINVAL;
	rec[s] = stream_record_at(cs->plan->D, seen ? seen[s] : 0u);
    }
    // behind the feeds queued on `stream`; the records are there when this returns
    if ( hipSetDevice(cs->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    return hipMemcpy(cs->rec.p + cs->parity * n, rec.get(), n * sizeof(StreamRecord), hipMemcpyHostToDevice) == hipSuccess
	? 0 : -EIO;
}

extern "C" int mifsk_channel_stream_seen( mifsk_channel_stream *cs, uint64_t *seen_out, void *stream )
{
    using namespace mifsk;
    if ( !cs || !seen_out )
	return -EINVAL;
    const size_t n = (size_t)cs->nstreams;
    const std::unique_ptr<StreamRecord[]> rec(new (std::nothrow) StreamRecord[n]);
    if ( !rec )
	return -ENOMEM;
    if ( hipSetDevice(cs->plan->device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess )
	return -EIO;
    if ( hipMemcpy(rec.get(), cs->rec.p + cs->parity * n, n * sizeof(StreamRecord), hipMemcpyDeviceToHost) != hipSuccess )
	return -EIO;
    for ( size_t s = 0; s < n; s++ )
	seen_out[s] = rec[s].seen;
    return 0;
}
