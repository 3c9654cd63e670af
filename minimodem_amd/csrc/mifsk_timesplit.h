// mifsk_timesplit.h -- the host logic of the time split (mifsk_timesplit_plan.cpp) as the driver in
// mifsk_timesplit.hip and a stand-alone program (tools/timesplit_rounds.cpp) share it: the planner,
// the row layout of a planned call, the host half of a round and the tail placement.  No HIP
// runtime call is made here; <hip/hip_runtime.h> is included for __host__ __device__ only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "mifsk.h"

// -EINVAL for a configuration the kernels cannot take (mifsk_config.cpp)
int mifsk_check_cfg( const mifsk_rx_config *cfg );

namespace mifsk {

// What the planner refuses whatever the lengths are (host only; the entry points that take host
// memory or files ask this before they touch the device or a file): the configuration, the flags,
// a warmup below 2 * samplebuf_size, a chunk off the lattice.
int time_split_check_params( const mifsk_rx_config *cfg, const mifsk_time_split *params );

namespace timesplit {

constexpr uint32_t kSentinel = 0xFFFFFFFFu;	// ep_first of an episode that began before the row
constexpr uint32_t kNoconfSat = 21u;		// FSK_MAX_NOCONFIDENCE_BITS + 1 (minimodem.c:1294)
constexpr double kDefaultWarmupSeconds = 10.0;	// DESIGN.md "cutting a stream in time"
constexpr uint32_t kChunksPerCu = 4;
// The rows are laid out apart, so the copy holds the recording plus (K - 1) * W samples of
// warm-up overlap; the library's choice of K keeps that overlap within this many bytes.
constexpr uint64_t kOverlapBudget = 4ull << 30;

// A row's starting state with the bookkeeping zeroed: the row's outputs then count from 0 and
// its running episode values are deltas against the state it starts from.  `shift` moves the
// state into the coordinates of a row that starts `shift` samples later.
__host__ __device__ inline mifsk_stream_state reset_book( mifsk_stream_state s, uint64_t shift )
{
    s.base -= shift;
    s.rp -= shift;
    s.carrier_nsamples = 0;
    s.nframes_total = 0;
    s.confidence_total = 0.0f;
    s.amplitude_total = 0.0f;
    s.nframes_decoded = 0;
    s.first_band = -1;
    s.ep_first = ( s.flags & MIFSK_STATE_CARRIER ) ? kSentinel : 0u;
    s.nbytes_total = 0;
    s.nepisodes_total = 0;
    s.status = 0;
    return s;
}

// Several recordings are cut by one plan (mifsk_demod_long_batch): all streams' chunks are rows of
// one flat batch, row rowbase[m] + k being chunk k of stream m, and stream m's tail is row R + m
// behind the R chunk rows.  A row is verified against its predecessor only inside its own stream.
struct RowRef {
    uint32_t	m, k;		// chunk k of stream m (k == K of the stream: its tail)
};

struct StreamRef {
    uint64_t	n;		// the stream's length
    uint64_t	tail_off;	// where its tail starts
    uint32_t	rowbase, K;	// its chunks are rows rowbase .. rowbase + K - 1
};

uint64_t gcd64( uint64_t a, uint64_t b );

// the planner, for a batch of recordings cut by one W and one L (every row has the same stride,
// a pass is one launch); chunks_hint: the chunk count that fills the chip (0: params->chunks or
// the default of a host-only call)
int plan( const mifsk_rx_config *cfg, const uint64_t *n, int nstreams, const mifsk_time_split *params,
	uint32_t chunks_hint, mifsk_time_split_stats *out );

// The rows of a planned call that cuts: stream m's chunks are rows rowbase[m] .. rowbase[m] + K_m - 1,
// its tail (the final slab) is row R + m.  hns[r]: the samples row r runs over (a tail's: 0 until
// place_tails).
struct RowLayout {
    int				M, R, nrows;	// streams, chunk rows, chunk rows + tails
    uint64_t			L, W, rstride;	// chunk, warmup, floats between the chunk rows
    size_t			fcap, ecap;	// frames (and bytes) and episodes a row can make
    std::vector<StreamRef>	hs;		// [M]
    std::vector<RowRef>		hrow;		// [nrows]
    std::vector<uint32_t>	hns;		// [nrows]

    RowLayout( const mifsk_rx_config *cfg, const uint64_t *nsamples, const std::vector<mifsk_time_split_stats> &ps );
};

// What the host knows of every row through the rounds: `settled` (a stream's consistent prefix,
// its row 0 from the start), `drop` (behind a row that finished its stream: decodes nothing),
// `ran` (was run again at least once), `mark` (runs again in this round).
struct RowFlags {
    std::vector<uint8_t>	settled, drop, ran, mark;	// [nrows] each

    explicit RowFlags( const RowLayout &lay );
};

// The host half of a round, which launches nothing.  From the codes of ts_verify: every stream's
// settled prefix grows over the rows that are consistent (accepted, unless they ran again) or
// dropped, and every unsettled row whose code is 0 is marked to run again in `f.mark` -- rows
// [lo, hi] hold them all; lo < 0: there is none, the rounds are over.
struct RowSpan {
    int	lo, hi;
};
RowSpan settle_round( const std::vector<uint32_t> &hcode, const RowLayout &lay, RowFlags &f,
	std::vector<mifsk_time_split_stats> &ps );

// Where the tails go.  last[m]: the paused state of stream m's last chunk, replaced by the state
// its tail starts from.  A stream whose last chunk was dropped or finished it gets no tail:
// tail_off = n, a finished state, length 0, drop[R + m].  Any other tail starts at the 16-byte
// aligned base of the last state, tail_off = (K - 1) * L + (base & ~3), from reset_book of it, and
// runs over hns[R + m] = n - tail_off samples.
struct Tails {
    uint64_t	longest;	// the longest tail
    bool	live;		// false: every tail is dropped
};
Tails place_tails( RowLayout &lay, std::vector<mifsk_stream_state> &last, std::vector<uint8_t> &drop );

} // namespace timesplit
} // namespace mifsk
