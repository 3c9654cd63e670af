// mifsk_channel.hip -- the channelizer (include/mifsk.h): mifsk_channel_plan_create / _destroy,
// mifsk_channelize_batch, the host helpers mifsk_channel_table and mifsk_channel_taps, and
// mifsk_channelize_iq_batch (include/mifsk/channel_iq.h): the same kernel with the epilogue that keeps
// both halves of the rotated sum.  The plan, the kernel's arguments and the geometry of a launch are in
// mifsk_channel_plan.h, the kernel and its launcher in mifsk_channel_kernel.h; mifsk_channel_stream.hip
// (rows fed in pieces) shares both.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk/channel_iq.h"
#include "mifsk_channel_kernel.h"
#include "mifsk_channel_plan.h"
#include "mifsk_ctx.h"

namespace mifsk {
namespace {

// what both table makers refuse of params
int channel_check_params( const mifsk_channel_params *p )
{
    if ( int rc = phase_check_params(p, MIFSK_CHANNEL_COMPLEX) )
	return rc;
    if ( p->decim == 0 || p->decim > kChMaxD )
	return -EINVAL;
    if ( (uint64_t)p->nchannels * p->ntaps > kChMaxKT )
	return -EINVAL;
    return 0;
}

// channel k's G, tap t at g[t * gstride]: the taps turned back by the channel's centre
void channel_table( const mifsk_channel_params *p, uint32_t k, double2 *g, size_t gstride )
{
    phase_rotated_taps(p->taps, p->ntaps, p->centres[k], p->phase_steps, true, g, gstride);
}

} // namespace
} // namespace mifsk

extern "C" int mifsk_channel_table( const mifsk_channel_params *params, uint32_t k, double *g_out )
{
    if ( int rc = mifsk::channel_check_params(params) )
	return rc;
    if ( k >= params->nchannels || !g_out )
	return -EINVAL;
    static_assert(sizeof(double2) == 2 * sizeof(double), "G is [ntaps][2] doubles");
    mifsk::channel_table(params, k, reinterpret_cast<double2 *>(g_out), 1);
    return 0;
}

extern "C" int mifsk_channel_taps( uint32_t ntaps, double cutoff_hz, double sample_rate, double gain, float *out )
{
    if ( ntaps == 0 || ntaps > mifsk::kPhaseMaxTaps || !out )
	return -EINVAL;
    if ( !( cutoff_hz > 0.0 ) || !( sample_rate > 0.0 ) || !std::isfinite(cutoff_hz) || !std::isfinite(sample_rate) )
	return -EINVAL;
    if ( ntaps == 1 ) {
	out[0] = (float)gain;
	return 0;
    }
    double h[mifsk::kPhaseMaxTaps];
    const double f = 2.0 * cutoff_hz / sample_rate, mid = (double)( ntaps - 1u ) / 2.0;
    double sum = 0.0;
    for ( uint32_t t = 0; t < ntaps; t++ ) {
	const double a = M_PI * ( f * ( (double)t - mid ) );
	const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
	h[t] = f * sinc * ( 0.54 - 0.46 * cos(mifsk::kTwoPi * (double)t / (double)( ntaps - 1u )) );
	sum += h[t];
    }
    for ( uint32_t t = 0; t < ntaps; t++ )
	out[t] = (float)( h[t] * ( gain / sum ) );
    return 0;
}

extern "C" int mifsk_channel_plan_create( mifsk_ctx *ctx, const mifsk_channel_params *params, mifsk_channel_plan **out )
{
    using namespace mifsk;
    if ( !ctx || !params || !out )
	return -EINVAL;
    if ( int rc = channel_check_params(params) )
	return rc;
    const uint32_t T = params->ntaps, K = params->nchannels;
    const size_t ngt = (size_t)T * K;
    const auto gt = host_array<double2>(ngt);
    const auto dq = host_array<uint32_t>(K);
    std::unique_ptr<mifsk_channel_plan> plan(new (std::nothrow) mifsk_channel_plan);
    if ( !gt || !dq || !plan )
	return -ENOMEM;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_table(params, k, gt.get() + k, K);
	dq[k] = phase_diff(params->out_centre, params->centres[k], params->phase_steps);
    }
    plan->D = params->decim;
    int rc = phase_plan_init(*plan, ctx->device, params, ( params->flags & MIFSK_CHANNEL_COMPLEX ) != 0, dq.get());
    if ( rc == 0 )
	rc = upload(plan->gt, gt.get(), ngt);
    if ( rc )
	return rc;
    *out = plan.release();
    return 0;
}

extern "C" void mifsk_channel_plan_destroy( mifsk_channel_plan *plan ) { mifsk::phase_plan_destroy(plan); }

// Both batch entries: their checks, then the one launch path.  An output element is a float, or with
// `iq` an (I, Q) pair: out_vec of them are 16 bytes, a row is out_max of them at most.
static int channelize_rows( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream, bool iq )
{
    using namespace mifsk;
    if ( !plan || !io )
	return -EINVAL;
    const OutKind ok = channel_out_kind(iq);
    if ( int rc = phase_check_io(*plan, io, io->d_rows, rows_vec(plan->cx, plan->s16), ok.vec, ok.max) )
	return rc;

    const ChannelGeometry g = channel_geometry(*plan);
    ChannelArgs A = channel_args(*plan, io, g);
    return channel_launch(*plan, g, io->out_stride, io->nstreams, A, iq, (hipStream_t)stream);
}

extern "C" int mifsk_channelize_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream )
{
    return channelize_rows(plan, io, stream, false);
}

extern "C" int mifsk_channelize_iq_batch( const mifsk_channel_plan *plan, const mifsk_channel_io *io, void *stream )
{
    return channelize_rows(plan, io, stream, true);
}
