// mifsk_channel_plan.h -- what the channelizer's two sources share (mifsk_channel.hip: the plan and the
// batch entries; mifsk_channel_stream.hip: the channel stream of include/mifsk/channel_stream.h): the
// plan, the kernels' constants and arguments, how a row's element is widened, and the geometry of a
// launch.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mifsk.h"
#include "mifsk_phase.h"
#include "mifsk_rows.h"

struct mifsk_channel_plan : mifsk::PhasePlanCommon {
    uint32_t			D;
    mifsk::DevMem<double2>	gt;
};

namespace mifsk {

constexpr int kChO = 8;					// outputs per lane
constexpr uint32_t kChWaves = 4u;			// waves of a workgroup
constexpr uint32_t kChTile = 64u;			// taps staged at a time, at most
constexpr uint32_t kChLdsTwo = 64u * 1024u;		// two workgroups per CU up to here
constexpr uint32_t kChLdsMax = 144u * 1024u;
constexpr uint32_t kChMaxD = 65535u;
constexpr uint64_t kChMaxKT = 1ull << 22;

struct ChannelArgs {
    const double2	*gt;		// G transposed, [T][K]
    const double2	*w;		// [P]: cos, sin
    const uint32_t	*dq;		// [K]: (r - q[k]) mod P
    RowsIn		in;		// elements
    uint32_t		T, D, K, P;
    uint32_t		s0;		// first stream of this launch
    uint32_t		cwshift;	// cw = 1 << cwshift channel lanes of a wave
    uint32_t		tt;		// taps per tile, a power of two
    uint32_t		ss;		// LDS samples between neighbouring outputs: D, or tt + 1
    float		*rows;
    size_t		out_stride;
    uint32_t		nout_cap;
    uint32_t		*nout;
};

// element `at` of a row as the definition widens it
template <bool CX, bool S16>
__device__ __forceinline__ auto channel_sample( const void *row, uint64_t at )
{
    if constexpr ( CX ) {
	if constexpr ( S16 ) {
	    const short2 v = reinterpret_cast<const short2 *>(row)[at];
	    return double2{(double)rows_f32(v.x), (double)rows_f32(v.y)};
	} else {
	    const float2 v = reinterpret_cast<const float2 *>(row)[at];
	    return double2{(double)v.x, (double)v.y};
	}
    } else {
	if constexpr ( S16 )
	    return (double)rows_f32(reinterpret_cast<const int16_t *>(row)[at]);
	else
	    return (double)reinterpret_cast<const float *>(row)[at];
    }
}

// What a launch over a plan's rows looks like, whatever the rows hold: nc channels per lane, C
// channels and OB outputs per workgroup, the tile of taps and the LDS it takes.
struct ChannelGeometry {
    uint32_t	nc, cwshift, C, OB, tt, ss;
    size_t	lds;
};

inline ChannelGeometry channel_geometry( const mifsk_channel_plan &plan )
{
    ChannelGeometry g = {};
    // two channels per lane as soon as there are two; cw channel lanes, the rest of a wave's lanes
    // are groups of outputs
    g.nc = plan.K > 1u ? 2u : 1u;
    const uint32_t ncl = ( plan.K + g.nc - 1u ) / g.nc;
    while ( ( 1u << g.cwshift ) < ncl && g.cwshift < 6u )
	g.cwshift++;
    g.C = ( 1u << g.cwshift ) * g.nc;
    g.OB = kChWaves * ( 64u >> g.cwshift ) * (uint32_t)kChO;
    // the tile of taps: the largest power of two with which table and samples fit, two workgroups
    // per CU down to 16 taps
    const size_t esz = plan.cx ? 16u : 8u;
    const uint32_t D = plan.D, C = g.C, OB = g.OB;
    auto lds_of = [&]( uint32_t tt ) {
	const uint32_t ss = D < tt ? D : tt + 1u;
	return (size_t)tt * C * sizeof(double2) + ( (size_t)( OB - 1u ) * ss + tt ) * esz;
    };
    uint32_t tt = kChTile;
    while ( tt / 2u >= plan.T )
	tt /= 2u;
    uint32_t two = tt;
    while ( two > 16u && lds_of(two) > kChLdsTwo )
	two /= 2u;
    if ( lds_of(two) <= kChLdsTwo )
	tt = two;
    while ( tt > 1u && lds_of(tt) > kChLdsMax )
	tt /= 2u;
    g.tt = tt;
    g.ss = D < tt ? D : tt + 1u;
    g.lds = lds_of(tt);
    return g;
}

// the arguments every launch over `plan` and `io` begins with
inline ChannelArgs channel_args( const mifsk_channel_plan &plan, const mifsk_channel_io *io, const ChannelGeometry &g )
{
    ChannelArgs A = {};
    A.gt = plan.gt.p;
    A.w = plan.w.p;
    A.dq = plan.dq.p;
    A.in = rows_in(io);
    A.T = plan.T;
    A.D = plan.D;
    A.K = plan.K;
    A.P = plan.P;
    A.cwshift = g.cwshift;
    A.tt = g.tt;
    A.ss = g.ss;
    A.rows = io->d_rows;
    A.out_stride = io->out_stride;
    A.nout_cap = io->nout_cap;
    A.nout = io->d_nout;
    return A;
}

} // namespace mifsk
