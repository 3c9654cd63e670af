// mifsk_mux_plan.h -- what the multiplexer's two sources share (mifsk_mux.hip: the plan and the batch
// entries; mifsk_mux_stream.hip: the multiplexer stream of include/mifsk/mux_stream.h): the plan, the
// kernel's constants and arguments, and the geometry of a launch.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mifsk.h"
#include "mifsk_phase.h"
#include "mifsk_rows.h"

struct mifsk_mux_plan : mifsk::PhasePlanCommon {
    uint32_t			L;
    mifsk::DevMem<double2>	g;
    mifsk::DevMem<uint32_t>	ps;
    mifsk::DevMem<float>	gains;		// empty: no gain step
};

namespace mifsk {

constexpr int kMxO = 8;					// outputs per lane
constexpr uint32_t kMxThreads = 256u;
constexpr uint32_t kMxLdsSamples = 48u * 1024u;		// table + samples: stage channels up to here (3 workgroups per CU)
constexpr uint32_t kMxMaxL = 65535u;

struct MuxArgs {
    const double2	*g;		// [T]
    const double2	*w;		// [P]: cos, sin
    const uint32_t	*dq;		// [K]: (q[k] - r) mod P
    const uint32_t	*ps;		// [K]: (dq[k] * (L mod P)) mod P
    const float		*gains;		// [K] or NULL
    RowsIn		in;		// floats; IQIN: (I, Q) pairs of floats
    uint32_t		T, L, K, P;
    uint32_t		jmax;		// ceil(T / L): tap steps of phase 0
    uint32_t		span;		// samples staged per channel, at most
    uint32_t		spanp;		// ... and doubles between the channels' spans (padded)
    uint32_t		cb;		// channels staged at a time
    uint32_t		s0;		// first stream of this launch
    void		*out;
    size_t		out_stride;	// elements
    uint32_t		nout_cap;
    uint32_t		*nout;
};

// What a launch over a plan's rows looks like, whatever the rows hold: the workgroups of a stream
// whose output row is out_stride elements, and the LDS of one.
struct MuxGeometry {
    uint32_t	nblocks;
    size_t	lds;
};

// The arguments every launch over `plan` and `io` begins with, and its geometry.  A block's 256 slots
// touch at most 255 / L + 2 groups of 8 values of m, and jmax - 1 samples before the first; as many
// channels' spans at a time as fit beside the table, one at least.
inline MuxArgs mux_args( const mifsk_mux_plan &plan, const mifsk_mux_io *io, MuxGeometry &geo )
{
    MuxArgs A = {};
    A.g = plan.g.p;
    A.w = plan.w.p;
    A.dq = plan.dq.p;
    A.ps = plan.ps.p;
    A.gains = plan.gains.p;
    A.in = rows_in(io);
    A.T = plan.T;
    A.L = plan.L;
    A.K = plan.K;
    A.P = plan.P;
    A.out = io->d_out;
    A.out_stride = io->out_stride;
    A.nout_cap = io->nout_cap;
    A.nout = io->d_nout;

    A.jmax = ( plan.T + plan.L - 1u ) / plan.L;
    A.span = (uint32_t)kMxO * ( ( kMxThreads - 1u ) / plan.L + 2u ) + A.jmax - 1u;
    A.spanp = A.span + ( A.span >> 3 ) + 1u;
    const size_t table = (size_t)plan.T * sizeof(double2), one = (size_t)A.spanp * sizeof(double);
    A.cb = table + one < kMxLdsSamples ? (uint32_t)( ( kMxLdsSamples - table ) / one ) : 1u;
    if ( A.cb > plan.K )
	A.cb = plan.K;
    geo.lds = table + (size_t)A.cb * one;
    // slots: L per group of 8 L outputs
    const uint64_t ngroups = ( io->out_stride + (uint64_t)kMxO * plan.L - 1u ) / ( (uint64_t)kMxO * plan.L );
    geo.nblocks = (uint32_t)( ( ngroups * plan.L + kMxThreads - 1u ) / kMxThreads );
    return A;
}

} // namespace mifsk
