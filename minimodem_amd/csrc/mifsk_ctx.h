// mifsk_ctx.h -- the device context as the host-side sources of libmifsk.so share it
// (mifsk_ctx.cpp owns it: its table cache, its chain, the host-memory pipeline's work).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "mifsk.h"
#include "mifsk_device.h"
#include "mifsk_hostmem.h"
#include "mifsk_tables.h"

using mifsk::DevCfg;

#define HIP_OK(call)	do { hipError_t e_ = (call); if ( e_ != hipSuccess ) { \
	fprintf(stderr, "mifsk: %s failed: %s\n", #call, hipGetErrorString(e_)); \
	return -EIO; } } while (0)

namespace mifsk {

// what a lookup of a configuration hands back, by value: the device copy of the DevCfg and the
// shared segments' rotation tables of the four scans (mifsk_device.h WaveAuto::d_rot)
struct CfgTables {
    const DevCfg	*d_cfg = nullptr;
    const double	*d_rot[5] = {};
    uint32_t		rot_stride[5] = {};
};

// The context's device tables: the bit tables and the spectrum tables by TwKey (a spectrum table's
// key has bit_nsamples == 0: never a bit table's), and one entry per distinct kernel configuration.
// An entry owns its memory, so dropping it frees it -- a half-made one too.  Not locked: the
// context's `lock` is held around every call.
struct TableCache {
    struct Table { TwKey key; DevMem<double> d; };
    struct Config { DevCfg host; DevMem<DevCfg> dev; DevMem<double> rot[5]; uint32_t rot_stride[5]; };
    std::vector<Table>	tables;
    std::vector<Config>	configs;

    int table( const TwKey &key, const double **d_out );
    int config( const DevCfg &d, CfgTables &out );
    size_t bytes() const;		// of twiddles held: every table and rotation table
    bool full() const;			// 64 configurations, 64 tables or 64 MB: the collector is due
    void clear() { tables.clear(); configs.clear(); }
};

// Chained launches (mifsk_device.h WaveChain): the groups' streams and events and the state array,
// made at the first batch that is cut.  `view` is what the launchers are handed.
struct ChainRes {
    DevMem<mifsk_stream_state>	state;		// (before the streams: freed after they are synchronised)
    HipStream	streams[WaveChain::kMaxGroups];
    HipEvent	ev_fork, ev_done[WaveChain::kMaxGroups];
    bool	made = false;
    WaveChain	view = {};
};

// the host-memory pipeline's streams, events and pinned staging (mifsk_hostpipe.cpp)
struct HostWork {
    std::mutex	lock;			// one host call at a time per context
    HipStream	s_in, s_comp, s_out;
    HipEvent	ev_in[2], ev_comp[2], ev_out[2];
    PinMem<uint8_t>	pin[2];		// staging for sources that are not page-locked
    PinMem<uint32_t>	pin_n[2];	// per-chunk stream lengths
    bool	ready = false;
};

} // namespace mifsk

struct mifsk_ctx {
    int			device;
    int			ncu;		// compute units (occupancy planning)
    char		name[256];
    std::mutex		lock;
    // Cached device tables (twiddles, DevCfg copies, the spectrum table) are shared by every
    // call on the context.  A call holds `gate` shared from the moment it looks a table up
    // until its kernels are enqueued; the collector (cache_gc, mifsk_ctx.cpp) takes it
    // exclusively and synchronises the device before it frees anything -- so nothing is freed
    // between a lookup and a launch, or under a kernel that is still running.
    std::shared_mutex	gate;
    mifsk::TableCache	cache;
    // the derived kernel configuration of the configurations seen last (fill_devcfg plans the
    // shared segments of every scan: 0.3 ms for RTTY -- per call, on the launch path, it was
    // 3 % of that kernel's time): a few entries, replaced round-robin
    struct DerivedCfg { mifsk_rx_config key; DevCfg d; };
    std::vector<DerivedCfg>	derived;
    size_t		derived_next = 0;
    std::unique_ptr<mifsk::HostWork>	host;
    // one chain is enqueued at a time (chain_lock), and each waits for the one before on the
    // device (ev_done)
    std::mutex		chain_lock;
    mifsk::ChainRes	chain;
};

// -EINVAL for a configuration the kernels cannot take (mifsk_config.cpp)
int mifsk_check_cfg( const mifsk_rx_config *cfg );

namespace mifsk {

// What every launching entry point does once its own arguments are checked (prepare()): bind the
// device, collect the caches if they are due, take the gate, look the tables up.  The gate stays
// held (shared) as long as this object lives: from the lookup until the caller has enqueued.
struct Prepared {
    std::shared_lock<std::shared_mutex> gate;
    DevCfg		d;
    const double	*d_tw = nullptr;
    CfgTables		tables;
};
int prepare( mifsk_ctx *ctx, const mifsk_rx_config *cfg, Prepared &p );

// fill_devcfg through the context's small cache
void derive_cfg( mifsk_ctx *ctx, const mifsk_rx_config &cfg, DevCfg &d );

// The first two steps of prepare() for a caller that needs only the spectrum table (the legacy
// fsk_detect_carrier): the device bound, the caches collected if due, `gate` taken.
int enter( mifsk_ctx *ctx, std::shared_lock<std::shared_mutex> &gate );

// The tables a launching entry point looks up for `cfg`: the derived kernel configuration, the
// context's twiddle table, and the gate that keeps them alive while it is held.  For
// mifsk_selftest.hip and mifsk_softbits.hip, whose kernels must run on the product's own tables.
// d_cfg (may be NULL): the context's device copy of `d`.
int lookup_tables( mifsk_ctx *ctx, const mifsk_rx_config *cfg, std::shared_lock<std::shared_mutex> &gate,
	DevCfg &d, const double **d_tw, const DevCfg **d_cfg = nullptr );
// The context's spectrum table for FFT size N: cos, -sin of 2 pi k / N for k < N, [N][2] doubles in
// device memory.  Called with the gate held (it is freed only by the collector).
int get_cs( mifsk_ctx *ctx, unsigned N, const double **d_out );

// What a chained launch needs (ctx->chain.view), with room for `ns` streams' states.  Called with
// ctx->chain_lock held.
int chain_prepare( mifsk_ctx *ctx, size_t ns );

// `overlapped`: the copy streams and the events of the host pipeline are wanted (mifsk_hostpipe.cpp)
int host_work_init( HostWork *w, bool overlapped );

}
