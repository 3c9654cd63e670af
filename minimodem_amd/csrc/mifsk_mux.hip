// mifsk_mux.hip -- the multiplexer (include/mifsk.h): mifsk_mux_plan_create / _destroy,
// mifsk_multiplex_batch, and the host helper mifsk_mux_table; mifsk_multiplex_iq_batch
// (include/mifsk/mux_iq.h): the same kernel with I/Q rows in (IQIN, at the kernel).  The kernel and its
// launcher are in mifsk_mux_kernel.h (which says how it is laid out), the plan and a launch's
// arguments in mifsk_mux_plan.h: mifsk_mux_stream.hip, the rows fed in pieces, shares both.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk/mux_iq.h"
#include "mifsk_ctx.h"
#include "mifsk_mux_kernel.h"
#include "mifsk_mux_plan.h"
#include "mifsk_phase.h"
#include "mifsk_rows.h"

namespace mifsk {
namespace {

// what both table makers refuse of params
int mux_check_params( const mifsk_mux_params *p )
{
    if ( int rc = phase_check_params(p, MIFSK_MUX_COMPLEX) )
	return rc;
    if ( p->interp == 0 || p->interp > kMxMaxL )
	return -EINVAL;
    return phase_centre_ok(p->in_centre, p->phase_steps) ? 0 : -EINVAL;
}

// G: the taps turned forward by the rows' centre
void mux_table( const mifsk_mux_params *p, double2 *g )
{
    phase_rotated_taps(p->taps, p->ntaps, p->in_centre, p->phase_steps, false, g, 1);
}

} // namespace
} // namespace mifsk

extern "C" int mifsk_mux_table( const mifsk_mux_params *params, double *g_out )
{
    if ( int rc = mifsk::mux_check_params(params) )
	return rc;
    if ( !g_out )
	return -EINVAL;
    static_assert(sizeof(double2) == 2 * sizeof(double), "G is [ntaps][2] doubles");
    mifsk::mux_table(params, reinterpret_cast<double2 *>(g_out));
    return 0;
}

extern "C" int mifsk_mux_plan_create( mifsk_ctx *ctx, const mifsk_mux_params *params, mifsk_mux_plan **out )
{
    using namespace mifsk;
    if ( !ctx || !params || !out )
	return -EINVAL;
    if ( int rc = mux_check_params(params) )
	return rc;
    const uint32_t P = params->phase_steps, T = params->ntaps, K = params->nchannels, L = params->interp;
    const auto g = host_array<double2>(T);
    const auto dq = host_array<uint32_t>(K), ps = host_array<uint32_t>(K);
    std::unique_ptr<mifsk_mux_plan> plan(new (std::nothrow) mifsk_mux_plan);
    if ( !g || !dq || !ps || !plan )
	return -ENOMEM;
    mux_table(params, g.get());
    for ( uint32_t k = 0; k < K; k++ ) {
	dq[k] = phase_diff(params->centres[k], params->in_centre, P);
	ps[k] = (uint32_t)( ( (uint64_t)dq[k] * ( L % P ) ) % P );
    }
    plan->L = L;
    int rc = phase_plan_init(*plan, ctx->device, params, ( params->flags & MIFSK_MUX_COMPLEX ) != 0, dq.get());
    if ( rc == 0 ) rc = upload(plan->g, g.get(), T);
    if ( rc == 0 ) rc = upload(plan->ps, ps.get(), K);
    if ( rc == 0 && params->gains ) rc = upload(plan->gains, params->gains, K);
    if ( rc )
	return rc;
    *out = plan.release();
    return 0;
}

extern "C" void mifsk_mux_plan_destroy( mifsk_mux_plan *plan ) { mifsk::phase_plan_destroy(plan); }

// Both entries.  `iq`: the input rows are (I, Q) pairs of floats, 2 of them 16 bytes, and the kernel is
// the IQIN one; everything else is a function of the plan and the io alone.
static int multiplex_rows( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream, bool iq )
{
    using namespace mifsk;
    if ( !plan || !io )
	return -EINVAL;
    if ( int rc = phase_check_io(*plan, io, io->d_out, iq ? 2u : 4u, rows_vec(plan->cx, plan->s16), 0xFFFFFFF8ull) )
	return rc;
    MuxGeometry geo = {};
    MuxArgs A = mux_args(*plan, io, geo);
    return mux_launch(*plan, geo, io->nstreams, A, iq, (hipStream_t)stream);
}

extern "C" int mifsk_multiplex_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream )
{
    return multiplex_rows(plan, io, stream, false);
}

extern "C" int mifsk_multiplex_iq_batch( const mifsk_mux_plan *plan, const mifsk_mux_io *io, void *stream )
{
    return multiplex_rows(plan, io, stream, true);
}
