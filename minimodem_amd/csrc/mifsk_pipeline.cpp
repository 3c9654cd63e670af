// mifsk_pipeline.cpp -- several batches in flight behind the C ABI (include/mifsk.h "passes in
// flight").
//
// A launch of mifsk_demod_batch ends well after its mean stream: the streams of a batch are
// serial chains of unequal length, and while the last ones finish most of the chip is idle
// (DESIGN.md section 6).  Nothing in the reference's call site -- one file after another,
// src/minimodem.c:1265,1373 through integration/minimodem-rx-batch.patch -- says batch i + 1 must
// wait for the last stream of batch i.  A pipeline owns what keeping P batches in flight needs:
// P lanes, each a device context (a context owns its launch scratch), a HIP stream and a
// completion event, and optionally P sets of output arrays; pass t runs on lane t mod P.
//
// HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the
// variable says otherwise; read when the runtime starts) and the null stream takes one of them:
// lanes beyond that share a queue and run one after the other -- measured slower than fewer lanes
// (profiles/r05_history.md section 6) -- so the depth is clamped to what the queues carry, and
// the clamp is reported.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_outputs.h"

namespace {

struct Lane {
    mifsk_ctx	*ctx = nullptr;
    mifsk::HipStream	stream;
    mifsk::HipEvent	done;		// behind the last pass submitted on this lane
    mifsk::HipEvent	after;		// the producer's stream at submit time
    uint64_t	last = 0;		// ticket of that pass
    bool	used = false;
    mifsk::OutMirror	set;	// its output arrays (io.nstreams: the batch size they were made for)
};

} // namespace

struct mifsk_pipeline {
    int			device = 0;
    uint32_t		requested = 0, depth = 0, hw_queues = 0;
    std::vector<Lane>	lanes;
    uint64_t		next = 0;
    bool		sets = false;
    std::mutex		lock;
};

extern "C" void mifsk_pipeline_destroy( mifsk_pipeline *p )
{
    if ( !p )
	return;
    (void)hipSetDevice(p->device);
    for ( Lane &l : p->lanes ) {
	// (in this order: the stream synchronised, then the output set, then the lane's context)
	l.stream.reset();
	l.set.reset();
	if ( l.ctx ) mifsk_ctx_destroy(l.ctx);
    }
    delete p;
}

extern "C" int mifsk_pipeline_create( mifsk_pipeline **out, int device, int depth )
{
    if ( !out )
	return -EINVAL;
    *out = nullptr;
    if ( depth < 1 )
	depth = 1;
    if ( depth > MIFSK_PIPELINE_MAX_DEPTH )
	depth = MIFSK_PIPELINE_MAX_DEPTH;
    mifsk_pipeline *p = new (std::nothrow) mifsk_pipeline;
    if ( !p )
	return -ENOMEM;
    p->requested = (uint32_t)depth;
    // what the runtime read when it started (a value set later has no effect on it)
    int hwq = 4;
    if ( const char *e = std::getenv("GPU_MAX_HW_QUEUES") ) {
	const int v = std::atoi(e);
	if ( v > 0 )
	    hwq = v;
    }
    p->hw_queues = (uint32_t)hwq;
    const int carry = hwq > 1 ? hwq - 1 : 1;	// the null stream takes a queue
    p->depth = (uint32_t)( depth < carry ? depth : carry );
    p->lanes.resize(p->depth);
    int rc = 0;
    for ( uint32_t i = 0; i < p->depth && rc == 0; i++ ) {
	Lane &l = p->lanes[i];
	rc = mifsk_ctx_create(&l.ctx, device);
	if ( rc != 0 )
	    break;
	if ( i == 0 )
	    p->device = mifsk::ctx_device(l.ctx);
	device = p->device;			// (device < 0: every lane on the one the first lane got)
	if ( hipSetDevice(p->device) != hipSuccess || l.stream.make() || l.done.make() || l.after.make() )
	    rc = -EIO;
    }
    if ( rc != 0 ) {
	mifsk_pipeline_destroy(p);
	return rc;
    }
    *out = p;
    return 0;
}

extern "C" int mifsk_pipeline_info_get( const mifsk_pipeline *p, mifsk_pipeline_info *info )
{
    if ( !p || !info )
	return -EINVAL;
    info->depth_requested = p->requested;
    info->depth = p->depth;
    info->hw_queues = p->hw_queues;
    info->output_sets = p->sets ? p->depth : 0u;
    return 0;
}

extern "C" int mifsk_pipeline_outputs_alloc( mifsk_pipeline *p, int nstreams, size_t frames_cap,
	size_t episodes_cap, unsigned want )
{
    if ( !p || nstreams <= 0 || frames_cap == 0 )
	return -EINVAL;
    std::lock_guard<std::mutex> g(p->lock);
    if ( hipSetDevice(p->device) != hipSuccess )
	return -EIO;
    const mifsk_demod_io ask = mifsk::outputs_want(want, frames_cap, episodes_cap);
    int rc = 0;
    for ( Lane &l : p->lanes ) {
	if ( l.stream )
	    (void)hipStreamSynchronize(l.stream);	// nothing may still write the old set
	if ( rc != 0 || ( rc = l.set.alloc(ask, (size_t)nstreams, false) ) != 0 )
	    continue;
	// (the zero fill is the lane's own work: in the order of its stream)
	for ( const mifsk::OutArray &a : mifsk::kOutArrays )
	    if ( void *d = mifsk::out_get(l.set.io, a) )
		if ( hipMemsetAsync(d, 0, (size_t)nstreams * mifsk::out_row_bytes(ask, a), l.stream) != hipSuccess )
		    rc = -EIO;
	l.set.io.nstreams = nstreams;
    }
    if ( rc != 0 ) {
	for ( Lane &l : p->lanes )
	    l.set.reset();
	p->sets = false;
	return rc;
    }
    p->sets = true;
    return 0;
}

extern "C" int mifsk_pipeline_outputs_get( mifsk_pipeline *p, uint64_t ticket, mifsk_demod_io *io )
{
    if ( !p || !io || !p->sets )
	return -EINVAL;
    mifsk::outputs_assign(*io, p->lanes[ticket % p->depth].set.io);
    return 0;
}

extern "C" uint64_t mifsk_pipeline_next_ticket( const mifsk_pipeline *p )
{
    return p ? p->next : 0;
}

extern "C" int mifsk_pipeline_submit( mifsk_pipeline *p, const mifsk_rx_config *cfg,
	const mifsk_demod_io *io, void *after, uint64_t *ticket )
{
    if ( !p || !cfg || !io )
	return -EINVAL;
    std::lock_guard<std::mutex> g(p->lock);
    Lane &l = p->lanes[p->next % p->depth];
    if ( hipSetDevice(p->device) != hipSuccess )
	return -EIO;
    mifsk_demod_io use = *io;
    if ( p->sets && !io->d_bytes && !io->d_bits && !io->d_frames && !io->d_nframes && !io->d_nbytes ) {
	// no outputs given: the lane's own set (which must have been made for batches this size)
	if ( io->nstreams > l.set.io.nstreams )
	    return -EINVAL;
	mifsk::outputs_assign(use, l.set.io);
    }
    if ( after != MIFSK_PIPELINE_NO_PRODUCER ) {
	// the batch was produced on the caller's stream: the lane waits for the point it has reached
	if ( hipEventRecord(l.after, (hipStream_t)after) != hipSuccess
		|| hipStreamWaitEvent(l.stream, l.after, 0) != hipSuccess )
	    return -EIO;
    }
    const int rc = mifsk_demod_batch(l.ctx, cfg, &use, l.stream);
    if ( rc != 0 )
	return rc;
    if ( hipEventRecord(l.done, l.stream) != hipSuccess )
	return -EIO;
    l.last = p->next;
    l.used = true;
    if ( ticket )
	*ticket = p->next;
    p->next++;
    return 0;
}

static Lane *lane_of( mifsk_pipeline *p, uint64_t ticket )
{
    if ( !p || ticket >= p->next )
	return nullptr;
    return &p->lanes[ticket % p->depth];
}

extern "C" int mifsk_pipeline_wait( mifsk_pipeline *p, uint64_t ticket )
{
    Lane *l = lane_of(p, ticket);
    if ( !l )
	return -EINVAL;
    // (the lane's event marks its LATEST pass: waiting for it covers every earlier one)
    return hipEventSynchronize(l->done) == hipSuccess ? 0 : -EIO;
}

extern "C" int mifsk_pipeline_join( mifsk_pipeline *p, uint64_t ticket, void *stream )
{
    Lane *l = lane_of(p, ticket);
    if ( !l )
	return -EINVAL;
    return hipStreamWaitEvent((hipStream_t)stream, l->done, 0) == hipSuccess ? 0 : -EIO;
}

extern "C" int mifsk_pipeline_drain( mifsk_pipeline *p )
{
    if ( !p )
	return -EINVAL;
    int rc = 0;
    for ( Lane &l : p->lanes )
	if ( l.used && hipStreamSynchronize(l.stream) != hipSuccess )
	    rc = -EIO;
    return rc;
}

extern "C" void *mifsk_pipeline_stream( mifsk_pipeline *p, uint64_t ticket )
{
    return p ? (void *)p->lanes[ticket % p->depth].stream : nullptr;
}

extern "C" mifsk_ctx *mifsk_pipeline_ctx( mifsk_pipeline *p, uint64_t ticket )
{
    return p ? p->lanes[ticket % p->depth].ctx : nullptr;
}
