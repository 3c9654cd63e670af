// mifsk_phase.h -- what the channelizer and the multiplexer (mifsk_channel.hip, mifsk_mux.hip) share
// on the host: phases are counted in steps of 1 / P of a turn, a plan holds the unit table W[p], the
// channels' phase steps dq[k] and taps rotated to a centre.  One set of limits, one check of the
// parameters both take, THE table code, and the common part of a plan.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>

#include "mifsk.h"
#include "mifsk_batch.h"
#include "mifsk_hostmem.h"

namespace mifsk {

constexpr uint32_t kPhaseMaxSteps = 1u << 20, kPhaseMaxTaps = 4096u, kPhaseMaxChannels = 4096u;
constexpr double kTwoPi = 6.283185307179586476925286766559;

// a centre reduced to [0, P)
inline int64_t phase_reduce( int64_t q, int64_t P )
{
    q %= P;
    return q < 0 ? q + P : q;
}

// |q| < P
inline bool phase_centre_ok( int64_t q, int64_t P ) { return q < P && -q < P; }

// (to - from) mod P
inline uint32_t phase_diff( int64_t to, int64_t from, int64_t P )
{
    return (uint32_t)phase_reduce(phase_reduce(to, P) - phase_reduce(from, P), P);
}

// What both plans refuse of the fields their parameters have in common (mifsk_channel_params,
// mifsk_mux_params), before the owner's own checks and before any HIP call.  `flag_mask`: the flags
// the owner knows.
template <class Params>
int phase_check_params( const Params *p, uint32_t flag_mask )
{
    if ( !p )
	return -EINVAL;
    if ( ( p->kind != MIFSK_FEED_F32 && p->kind != MIFSK_FEED_S16 ) || ( p->flags & ~flag_mask ) )
	return -EINVAL;
    if ( p->phase_steps == 0 || p->phase_steps > kPhaseMaxSteps )
	return -EINVAL;
    if ( p->ntaps == 0 || p->ntaps > kPhaseMaxTaps || !p->taps )
	return -EINVAL;
    if ( p->nchannels == 0 || p->nchannels > kPhaseMaxChannels || !p->centres )
	return -EINVAL;
    for ( uint32_t k = 0; k < p->nchannels; k++ )
	if ( !phase_centre_ok(p->centres[k], p->phase_steps) )
	    return -EINVAL;
    return 0;
}

// THE table code, for the plans, mifsk_channel_table and mifsk_mux_table: tap t rotated by
// (q t) mod P steps at g[t * gstride], (h cos, h sin); `conj`: (h cos, -(h sin)).  The negation is a
// pass of its own over the stored products, so that it is IEEE's, of zeros and NaNs too: next to
// the product a compiler may turn -(h s) into h (-s), whose NaN has the sign of h s.
inline void phase_rotated_taps( const float *taps, uint32_t T, int64_t q, int64_t P, bool conj, double2 *g, size_t gstride )
{
    q = phase_reduce(q, P);
    for ( uint32_t t = 0; t < T; t++ ) {
	const int64_t idx = ( q * (int64_t)t ) % P;
	double s, c;
	sincos(kTwoPi * (double)idx / (double)P, &s, &c);
	const double h = (double)taps[t];
	g[(size_t)t * gstride] = double2{h * c, h * s};
    }
    if ( conj )
	for ( uint32_t t = 0; t < T; t++ )
	    g[(size_t)t * gstride].y = -g[(size_t)t * gstride].y;
}

// W[p] = (cos, sin) of p steps
inline void phase_unit_table( uint32_t P, double2 *w )
{
    for ( uint32_t p = 0; p < P; p++ ) {
	double s, c;
	sincos(kTwoPi * (double)p / (double)P, &s, &c);
	w[p] = double2{c, s};
    }
}

// n elements on the host, or nothing
template <class T>
std::unique_ptr<T[]> host_array( size_t n ) { return std::unique_ptr<T[]>(new (std::nothrow) T[n]); }

// n elements of `host` in a new block of the current device
template <class T>
int upload( DevMem<T> &d, const T *host, size_t n )
{
    if ( int rc = d.alloc(n) )
	return rc;
    return hipMemcpy(d.p, host, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? 0 : -EIO;
}

// what a plan of either kind holds; the owner derives from it and adds its G and what else it needs
struct PhasePlanCommon {
    int			device;
    bool		cx, s16;
    uint32_t		P, T, K;
    DevMem<double2>	w;		// [P]
    DevMem<uint32_t>	dq;		// [K]
};

// The common part of a plan from checked parameters: the fields, and W and dq (the owner's [K] phase
// steps) uploaded.  `device` is current when this returns 0, for the owner's own uploads.
template <class Params>
int phase_plan_init( PhasePlanCommon &plan, int device, const Params *p, bool cx, const uint32_t *dq )
{
    plan.device = device;
    plan.cx = cx;
    plan.s16 = p->kind == MIFSK_FEED_S16;
    plan.P = p->phase_steps;
    plan.T = p->ntaps;
    plan.K = p->nchannels;
    const auto w = host_array<double2>(plan.P);
    if ( !w )
	return -ENOMEM;
    phase_unit_table(plan.P, w.get());
    if ( hipSetDevice(device) != hipSuccess )
	return -EIO;
    if ( int rc = upload(plan.w, w.get(), plan.P) )
	return rc;
    return upload(plan.dq, dq, plan.K);
}

template <class Plan>
void phase_plan_destroy( Plan *plan )
{
    if ( !plan )
	return;
    (void)hipSetDevice(plan->device);
    (void)hipDeviceSynchronize();		// no kernel reads the tables any more
    delete plan;
}

// What both batch entries refuse of their rows (rows_io_check of mifsk_batch.h, K the plan's)
template <class IO>
int phase_check_io( const PhasePlanCommon &plan, const IO *io, const void *d_out, uint32_t in_vec, uint32_t out_vec,
	uint64_t out_max )
{
    return rows_io_check(plan.K, io, d_out, in_vec, out_vec, out_max);
}

} // namespace mifsk
