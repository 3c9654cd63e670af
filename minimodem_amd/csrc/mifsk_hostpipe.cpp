// mifsk_hostpipe.cpp -- the receive path for streams that start in HOST memory or in
// FILES (SURVEY 8 d "H2D-inclusive", 8 f3; reference: src/simpleaudio-sndfile.c:42-74,
// src/minimodem.c:1014-1032 -- `--rx --file x.wav`).
//
// The kernels take 0.5 ms for a batch that needs 35 ms to cross PCIe, so what a
// host caller sees is the copy.  This file makes the copy the only thing it sees:
//
//   chunk k+1:  stage (threads: memcpy / pread into pinned memory, or nothing when the
//               caller's memory is pinned) -> hipMemcpyAsync on the copy stream
//   chunk k  :  S16 -> float + --Xrxnoise (device, mifsk_ingest.hip) -> receive loop
//               (mifsk_demod_batch) on the compute stream
//   chunk k-1:  results -> host on the output stream
//
// Two slots of everything; events order the three streams; the host thread only
// waits for a slot when it is about to reuse it.  16-bit input crosses the bus as
// 16-bit and is converted on the device, exactly as libsndfile converts it
// (value / 32768).  Nothing here computes on the host: no device, no result.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"
#include "mifsk_outputs.h"
#include "mifsk_timesplit.h"

namespace mifsk {

// wav header of a file of which only the first `have` bytes are in memory (mifsk_ingest.hip)
int wav_parse_sized( const void *file, size_t have, size_t file_size, mifsk_wav_info *info );

namespace {

constexpr size_t kChunkBytes = 64u << 20;	// of input per chunk: ~1 ms of PCIe gen5 x16

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int host_work_get( mifsk_ctx *ctx, HostWork **out )
{
    std::lock_guard<std::mutex> g(ctx->lock);
    if ( !ctx->host )
	ctx->host.reset(new (std::nothrow) HostWork());
    if ( !ctx->host )
	return -ENOMEM;
    *out = ctx->host.get();
    return 0;
}

// both pinned buffers of one kind, `n` elements long at least
template <class T>
int pin_grow( PinMem<T> ( &buf )[2], size_t n )
{
    if ( n <= buf[0].cap && n <= buf[1].cap )
	return 0;
    buf[0].reset();
    buf[1].reset();
    if ( const int rc = buf[0].alloc(n) )
	return rc;
    return buf[1].alloc(n);
}

int pin_reserve( HostWork *w, size_t bytes, size_t nrows )
{
    if ( const int rc = pin_grow(w->pin, bytes) )
	return rc;
    return pin_grow(w->pin_n, nrows);
}

bool is_pinned( const void *p )
{
    if ( !p )
	return false;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    if ( hipPointerGetAttributes(&a, p) != hipSuccess ) {
	(void)hipGetLastError();		// ordinary memory: not an error
	return false;
    }
    return a.type == hipMemoryTypeHost;
}

// fn(i) for i in [0, n) on up to `nthreads` threads (the caller's included)
template <typename F>
void parallel_for( size_t n, unsigned nthreads, F fn )
{
    if ( n == 0 )
	return;
    if ( nthreads > n ) nthreads = (unsigned)n;
    if ( nthreads <= 1 ) {
	for ( size_t i = 0; i < n; i++ ) fn(i);
	return;
    }
    // An exception on a worker thread would terminate the process, and one thrown while the
    // threads are being created would destroy joinable threads (the same): every item runs
    // inside a try, the first exception is kept, every thread that did start is joined, and
    // the exception is rethrown on the caller -- whose own catch turns it into an error code
    // at the C ABI.
    std::atomic<size_t> next(0);
    std::exception_ptr first;
    std::mutex first_lock;
    auto body = [&]() {
	for (;;) {
	    const size_t i = next.fetch_add(1);
	    if ( i >= n ) break;
	    try {
		fn(i);
	    } catch ( ... ) {
		std::lock_guard<std::mutex> g(first_lock);
		if ( !first )
		    first = std::current_exception();
		next.store(n);			// nothing more is started
	    }
	}
    };
    std::vector<std::thread> ts;
    try {
	ts.reserve(nthreads);
	for ( unsigned t = 1; t < nthreads; t++ )
	    ts.emplace_back(body);
    } catch ( ... ) {				// thread creation failed: go on with those there are
    }
    body();
    for ( std::thread &t : ts )
	t.join();
    if ( first )
	std::rethrow_exception(first);
}

unsigned staging_threads()
{
    unsigned hw = std::thread::hardware_concurrency();
    if ( hw == 0 ) hw = 4;
    unsigned t = hw / 2;
    if ( t < 2 ) t = 2;
    if ( t > 16 ) t = 16;
    return t;
}

// one stream: `n` samples at `mem`, or in the file `path` from byte `off`
struct Row {
    const void	*mem;
    const char	*path;
    uint64_t	off;
    uint64_t	n;
    int		*err;		// file rows: where a read error is reported
};

int read_fully( int fd, void *buf, size_t n, uint64_t off )
{
    unsigned char *p = (unsigned char *)buf;
    while ( n ) {
	const ssize_t r = pread(fd, p, n, (off_t)off);
	if ( r < 0 ) {
	    if ( errno == EINTR ) continue;
	    return -errno;
	}
	if ( r == 0 )
	    return -EIO;		// shorter than its header said a moment ago
	p += r; off += (uint64_t)r; n -= (size_t)r;
    }
    return 0;
}

// MIFSK_TEST_FAULT_READ: file rows whose path holds this tag cannot be read (fault injection for
// tests/test_gpu_files.py: a file that shrinks between its header and its samples cannot be staged
// without a race).  A test hook like every other knob: honoured only with MIFSK_EXPERIMENT set, so
// that a stray variable cannot turn production reads into rows of zeros.
const char *read_fault_tag()
{
    const char *tag = experiment_env("MIFSK_TEST_FAULT_READ");
    return tag && *tag ? tag : nullptr;
}

// a file row's descriptor for as long as the row is staged (memory rows, empty rows: none)
struct RowFile {
    int fd = -1, err = 0;
    RowFile( const Row &row, const char *fault_tag )
    {
	if ( row.mem || !row.n )
	    return;
	fd = open(row.path, O_RDONLY | O_CLOEXEC);
	if ( fd < 0 )
	    err = -errno;
	else if ( fault_tag && std::strstr(row.path, fault_tag) )
	    err = -EIO;
    }
    ~RowFile() { if ( fd >= 0 ) close(fd); }
    RowFile( const RowFile & ) = delete;
    RowFile &operator=( const RowFile & ) = delete;
};

// Bytes [first, first + count) of a row's samples into pinned memory at `dst`, from the caller's
// memory or from the row's file.  What cannot be read (a file that shrank after its header was
// read, a read error) is this row's error, not the batch's: zeros stand in its place, the error
// goes to the row's own slot -- several blocks of one row may report at once -- and is returned.
int stage( const Row &row, const RowFile &file, uint64_t first, size_t count, void *dst )
{
    if ( row.mem ) {
	std::memcpy(dst, (const char *)row.mem + first, count);
	return 0;
    }
    const int e = file.err ? file.err : count ? read_fully(file.fd, dst, count, row.off + first) : 0;
    if ( e ) {
	std::memset(dst, 0, count);
	if ( row.err )
	    __atomic_store_n(row.err, e, __ATOMIC_RELAXED);
    }
    return e;
}

// Page-locked source rows are copied from where they are.  Rows at one pitch in one host array
// (`src_pitch` set): its first and its last byte answer for all of them; otherwise every row that
// has samples is asked, and there has to be one.
bool rows_pinned( const std::vector<Row> &rows, size_t esz, size_t src_pitch )
{
    auto last_byte = [esz]( const Row &r ) { return (const char *)r.mem + (size_t)r.n * esz - ( r.n ? 1 : 0 ); };
    if ( src_pitch )
	return rows.front().mem && is_pinned(rows.front().mem) && is_pinned(last_byte(rows.back()));
    bool any = false;
    for ( const Row &r : rows )
	if ( r.n ) {
	    if ( !( r.mem && is_pinned(r.mem) && is_pinned(last_byte(r)) ) )
		return false;
	    any = true;
	}
    return any;
}

void host_stats_add( mifsk_host_stats *st, double t_begin, double t_stage, uint64_t bytes_in, uint64_t bytes_out,
	size_t chunks, size_t streams, bool direct )
{
    if ( !st )
	return;
    st->seconds_total += now_s() - t_begin;
    st->seconds_staging += t_stage;
    st->bytes_h2d += bytes_in;
    st->bytes_d2h += bytes_out;
    st->chunks += (uint32_t)chunks;
    st->streams += (uint32_t)streams;
    st->source_pinned = direct ? 1u : 0u;
}

struct Chunk {
    size_t	lo, hi;		// rows
    size_t	stride;		// elements per device row
};

struct Slot {
    DevMem<uint8_t>	in;	// the chunk as it crossed the bus
    DevMem<float>	x;	// S16 input: the converted samples
    DevMem<uint32_t>	n;	// the chunk's stream lengths
    OutMirror		out;	// the mirror of the host's result arrays
};

// A batch of streams (`s16`: rows are int16_t, else float) through the chunked pipeline the head
// of this file draws.  `flags`: MIFSK_IO_* for mifsk_demod_batch; `src_pitch`: the rows are
// equally spaced in one host array (memory rows only), in elements; `ho`: the host result arrays,
// [rows][cap], any of which may be NULL.
int run_job( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const std::vector<Row> &rows, bool s16, float rxnoise,
	unsigned flags, size_t src_pitch, const mifsk_demod_io &ho, mifsk_host_stats *stats )
{
    const size_t nrows = rows.size();
    if ( nrows == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    HostWork *w = nullptr;
    int rc = host_work_get(ctx, &w);
    if ( rc )
	return rc;
    std::lock_guard<std::mutex> g(w->lock);
    // MIFSK_CLI_TIMING=1: the phases of a job on stderr (what a batch of ONE pays: INTEGRATION.md 1b)
    const bool timing = std::getenv("MIFSK_CLI_TIMING") != nullptr;
    const double t_enter = now_s();
    const size_t esz = s16 ? 2 : 4;

    // chunks of whole streams, ~kChunkBytes of input each
    std::vector<Chunk> chunks;
    size_t max_bytes = 0, max_rows = 0, max_floats = 0;
    bool uniform_n = true;
    for ( size_t lo = 0; lo < nrows; ) {
	size_t hi = lo, maxn = 0;
	while ( hi < nrows ) {
	    const size_t m = std::max(maxn, (size_t)rows[hi].n);
	    const size_t stride = ( m + 7 ) & ~(size_t)7;
	    if ( hi > lo && ( hi - lo + 1 ) * stride * esz > kChunkBytes )
		break;
	    maxn = m;
	    hi++;
	}
	const Chunk c = { lo, hi, std::max<size_t>(( maxn + 7 ) & ~(size_t)7, 8) };
	chunks.push_back(c);
	max_bytes = std::max(max_bytes, ( hi - lo ) * c.stride * esz);
	max_floats = std::max(max_floats, ( hi - lo ) * c.stride);
	max_rows = std::max(max_rows, hi - lo);
	lo = hi;
    }
    for ( size_t i = 1; i < nrows; i++ )
	uniform_n = uniform_n && rows[i].n == rows[0].n;
    const bool single = chunks.size() == 1;
    rc = host_work_init(w, !single);
    if ( rc )
	return rc;
    const double t_begin = now_s();
    // (one chunk: everything in order on the null stream, which the runtime has anyway)
    const hipStream_t st_comp = single ? nullptr : w->s_comp;
    const hipStream_t st_in = single ? st_comp : w->s_in, st_out = single ? st_comp : w->s_out;

    const bool direct = rows_pinned(rows, esz, src_pitch);
    rc = pin_reserve(w, direct ? 0 : max_bytes, max_rows);
    if ( rc )
	return rc;

    // every array the host asked for is mirrored, counters included, and left as allocated (the
    // receive loop writes every row of them); d_carrier_band comes back only under --auto-carrier
    mifsk_demod_io back = ho;
    if ( !( cfg->auto_carrier_threshold > 0.0f ) )
	back.d_carrier_band = nullptr;
    Slot slots[2];
    for ( Slot &s : slots )
	if ( ( rc = s.in.alloc(max_bytes + 64) )
		|| ( s16 && ( rc = s.x.alloc(max_floats + 16) ) )
		|| ( rc = s.n.alloc(max_rows) )
		|| ( rc = s.out.alloc(ho, max_rows, false) ) )
	    return rc;

    const double t_alloc = now_s();
    const unsigned nthreads = staging_threads();
    const char *fault_tag = read_fault_tag();
    double t_stage = 0.0;
    uint64_t bytes_in = 0, bytes_out = 0;

    auto copy_out = [&]( size_t ci ) -> int {		// results of chunk ci -> host, on s_out
	const Chunk &c = chunks[ci];
	if ( !single )
	    HIP_OK(hipStreamWaitEvent(st_out, w->ev_comp[ci & 1], 0));
	if ( const int e = slots[ci & 1].out.copy_out(back, c.lo, c.hi, st_out, &bytes_out) )
	    return e;
	if ( !single )
	    HIP_OK(hipEventRecord(w->ev_out[ci & 1], st_out));
	return 0;
    };

    for ( size_t ci = 0; ci < chunks.size(); ci++ ) {
	const Chunk &c = chunks[ci];
	const int sl = (int)( ci & 1 );
	Slot &s = slots[sl];
	uint32_t *const d_n = s.n.p;
	const size_t r = c.hi - c.lo;
	if ( ci >= 2 )
	    HIP_OK(hipEventSynchronize(w->ev_out[sl]));	// chunk ci - 2 has left this slot
	// ---- stage
	const void *src = nullptr;
	size_t src_pitch_bytes = 0;
	if ( direct ) {
	    src = rows[c.lo].mem;
	    src_pitch_bytes = src_pitch * esz;
	} else {
	    const double t0 = now_s();
	    unsigned char *dst = w->pin[sl].p;
	    parallel_for(r, nthreads, [&]( size_t i ) {
		const Row &row = rows[c.lo + i];
		(void)stage(row, RowFile(row, fault_tag), 0, (size_t)row.n * esz, dst + i * c.stride * esz);
	    });
	    t_stage += now_s() - t0;
	    src = dst;
	    src_pitch_bytes = c.stride * esz;
	}
	for ( size_t i = 0; i < r; i++ )
	    w->pin_n[sl].p[i] = (uint32_t)rows[c.lo + i].n;
	// ---- host -> device
	size_t width = std::min(src_pitch_bytes, c.stride * esz);
	if ( direct && nrows == 1 ) {
	    // a lone row's stride means nothing (its length is not clipped to it either)
	    width = (size_t)rows[0].n * esz;
	    src_pitch_bytes = c.stride * esz;
	}
	if ( src_pitch_bytes == c.stride * esz )	// rows back to back on both sides: one linear copy
	    HIP_OK(hipMemcpyAsync(s.in.p, src, width * r, hipMemcpyHostToDevice, st_in));
	else
	    HIP_OK(hipMemcpy2DAsync(s.in.p, c.stride * esz, src, src_pitch_bytes, width, r,
				    hipMemcpyHostToDevice, st_in));
	HIP_OK(hipMemcpyAsync(d_n, w->pin_n[sl].p, r * sizeof(uint32_t), hipMemcpyHostToDevice, st_in));
	bytes_in += width * r;
	// ---- convert + receive loop
	if ( !single ) {
	    HIP_OK(hipEventRecord(w->ev_in[sl], st_in));
	    HIP_OK(hipStreamWaitEvent(st_comp, w->ev_in[sl], 0));
	}
	const float *d_x = (const float *)s.in.p;
	if ( s16 ) {
	    rc = mifsk_ingest_s16(ctx, (const int16_t *)s.in.p, c.stride, s.x.p, c.stride, d_n, 0,
				  (int)r, rxnoise, st_comp);
	    d_x = s.x.p;
	} else if ( rxnoise != 0.0f ) {
	    rc = mifsk_ingest_rxnoise_f32(ctx, (float *)s.in.p, c.stride, d_n, 0, (int)r, rxnoise, st_comp);
	}
	if ( rc )
	    return rc;
	mifsk_demod_io io = s.out.io;
	io.d_samples = d_x;
	io.stream_stride = c.stride;
	io.d_nsamples = uniform_n ? nullptr : d_n;
	io.nsamples = (uint32_t)rows[c.lo].n;
	io.nstreams = (int)r;
	io.flags = flags;
	rc = mifsk_demod_batch(ctx, cfg, &io, st_comp);
	if ( rc )
	    return rc;
	if ( !single )
	    HIP_OK(hipEventRecord(w->ev_comp[sl], st_comp));
	// ---- the chunk before this one: results -> host (after this chunk's work is queued,
	// so that a copy into pageable memory, which blocks this thread, hides behind it)
	if ( ci >= 1 ) {
	    rc = copy_out(ci - 1);
	    if ( rc )
		return rc;
	}
    }
    rc = copy_out(chunks.size() - 1);
    if ( rc )
	return rc;
    const double t_queued = now_s();
    if ( !single )
	HIP_OK(hipStreamSynchronize(w->s_out));
    HIP_OK(hipStreamSynchronize(st_comp));
    if ( !single )
	HIP_OK(hipStreamSynchronize(w->s_in));
    if ( timing )
	std::fprintf(stderr, "### TIMING job of %zu rows: streams + events %.1f ms, pinned + device buffers %.1f ms, "
			     "read + queue (incl. the first launch: code object, tables) %.1f ms, device until done %.1f ms\n",
		     nrows, 1e3 * ( t_begin - t_enter ), 1e3 * ( t_alloc - t_begin ), 1e3 * ( t_queued - t_alloc ),
		     1e3 * ( now_s() - t_queued ));
    host_stats_add(stats, t_begin, t_stage, bytes_in, bytes_out, chunks.size(), nrows, direct);
    return 0;		// (what a row could not read is in its own error slot)
}

// ---- long recordings, cut in time (mifsk_timesplit.hip), from host memory or from files ----
//
// A few long recordings instead of many short ones: the samples cross the bus as they are (PCM16
// as 16-bit) into ONE device buffer with a common stride, in pieces of kChunkBytes -- by DMA from
// where they are when every row is page-locked, through the context's two pinned staging buffers
// otherwise, piece k+1 being staged while piece k is copied -- and the buffer is decoded by
// mifsk_demod_long_batch_s16 (PCM16: the rows are gathered straight from it, no float copy of the
// recording) or mifsk_demod_long_batch (floats, --Xrxnoise added in place first).

struct Piece {
    size_t	row;
    uint64_t	first, count;	// samples of the row
};

int run_long( mifsk_ctx *ctx, const mifsk_rx_config *cfg, const std::vector<Row> &rows, bool s16,
	float rxnoise, const mifsk_time_split *params, const mifsk_demod_io &ho,
	mifsk_time_split_stats *tstats, mifsk_host_stats *hstats )
{
    const size_t M = rows.size();
    if ( M == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    HostWork *w = nullptr;
    int rc = host_work_get(ctx, &w);
    if ( rc )
	return rc;
    std::lock_guard<std::mutex> g(w->lock);
    const double t_begin = now_s();
    const size_t esz = s16 ? 2 : 4, align = s16 ? 8 : 4;
    uint64_t longest = 0;
    std::vector<uint64_t> lens(M);
    for ( size_t m = 0; m < M; m++ ) {
	lens[m] = rows[m].n;
	longest = std::max(longest, rows[m].n);
    }
    const size_t stride = std::max<size_t>(align, ( (size_t)longest + align - 1 ) & ~( align - 1 ));

    // pieces of one row each, kChunkBytes at most
    const uint64_t per = kChunkBytes / esz;
    std::vector<Piece> pieces;
    for ( size_t m = 0; m < M; m++ )
	for ( uint64_t first = 0; first < rows[m].n; first += per )
	    pieces.push_back(Piece{ m, first, std::min<uint64_t>(per, rows[m].n - first) });
    const bool single = pieces.size() <= 1;
    if ( ( rc = host_work_init(w, !single) ) )
	return rc;
    const hipStream_t st_in = single ? nullptr : w->s_in, st_comp = single ? nullptr : w->s_comp;

    const bool direct = rows_pinned(rows, esz, 0);
    if ( !direct && ( rc = pin_reserve(w, (size_t)std::min<uint64_t>(per, longest) * esz, 0) ) )
	return rc;

    DevMem<uint8_t> d_in;
    if ( ( rc = d_in.alloc(M * stride * esz, 16, true) ) )
	return rc;
    const unsigned nthreads = staging_threads();
    const char *fault_tag = read_fault_tag();
    constexpr size_t kBlock = 1u << 20;		// of a piece per staging task
    double t_stage = 0.0;
    uint64_t bytes_in = 0, bytes_out = 0;
    for ( size_t k = 0; k < pieces.size(); k++ ) {
	const Piece &pc = pieces[k];
	const Row &row = rows[pc.row];
	const int sl = (int)( k & 1 );
	const size_t bytes = (size_t)pc.count * esz;
	uint8_t *dst = d_in.p + ( pc.row * stride + (size_t)pc.first ) * esz;
	const void *src;
	if ( direct ) {
	    src = (const char *)row.mem + (size_t)pc.first * esz;
	} else {
	    if ( k >= 2 )
		HIP_OK(hipEventSynchronize(w->ev_in[sl]));	// piece k - 2 has left this buffer
	    const double t0 = now_s();
	    uint8_t *pin = w->pin[sl].p;
	    const RowFile file(row, fault_tag);		// (opened once per piece, not per block)
	    parallel_for(( bytes + kBlock - 1 ) / kBlock, nthreads, [&]( size_t b ) {
		const size_t o = b * kBlock;
		(void)stage(row, file, pc.first * esz + o, std::min(kBlock, bytes - o), pin + o);
	    });
	    t_stage += now_s() - t0;
	    src = pin;
	}
	HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st_in));
	if ( !direct && !single )
	    HIP_OK(hipEventRecord(w->ev_in[sl], st_in));
	bytes_in += bytes;
    }
    HIP_OK(hipStreamSynchronize(st_in));

    // --Xrxnoise on floats, in place (PCM16: added as the rows are gathered)
    if ( !s16 && rxnoise != 0.0f )
	for ( size_t m = 0; m < M; m++ )
	    for ( uint64_t o = 0; o < rows[m].n; o += 1ull << 30 ) {
		const uint32_t cnt = (uint32_t)std::min<uint64_t>(1ull << 30, rows[m].n - o);
		if ( ( rc = mifsk_ingest_rxnoise_f32(ctx, (float *)d_in.p + m * stride + o, stride, nullptr, cnt,
						      1, rxnoise, st_comp) ) )
		    return rc;
	    }

    // the outputs, as mifsk_demod_batch_host lays them out: no counters, d_carrier_band only under
    // --auto-carrier, and zero-filled
    mifsk_demod_io want = ho;
    want.d_counters = nullptr;
    if ( !( cfg->auto_carrier_threshold > 0.0f ) )
	want.d_carrier_band = nullptr;
    OutMirror out;
    if ( ( rc = out.alloc(want, M, true) ) )
	return rc;
    mifsk_demod_io io = out.io;
    io.nstreams = (int)M;
    rc = s16 ? mifsk_demod_long_batch_s16(ctx, cfg, (const int16_t *)d_in.p, stride, lens.data(), (int)M, rxnoise,
					  params, &io, tstats, st_comp)
	     : mifsk_demod_long_batch(ctx, cfg, (const float *)d_in.p, stride, lens.data(), (int)M, params, &io,
				      tstats, st_comp);
    if ( rc )
	return rc;
    // (the call has waited for its stream)
    if ( ( rc = out.copy_out(ho, 0, M, nullptr, &bytes_out) ) )
	return rc;
    HIP_OK(hipStreamSynchronize(nullptr));
    host_stats_add(hstats, t_begin, t_stage, bytes_in, bytes_out, pieces.size(), M, direct);
    return 0;
}

} // namespace
} // namespace mifsk

using mifsk::Row;

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" void *mifsk_host_alloc( size_t bytes )
{
    void *p = nullptr;
    if ( hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess ) {
	(void)hipGetLastError();
	return nullptr;
    }
    return p;
}

extern "C" void mifsk_host_free( void *p )
{
    if ( p )
	(void)hipHostFree(p);
}

extern "C" int mifsk_demod_batch_host_ex( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *hio, float rxnoise, mifsk_host_stats *stats )
{
    if ( !ctx || !hio || mifsk_check_cfg(cfg) || hio->nstreams < 0 )
	return -EINVAL;
    if ( stats )
	std::memset(stats, 0, sizeof(*stats));
    const size_t ns = (size_t)hio->nstreams;
    if ( ns == 0 )
	return 0;
    if ( !hio->d_samples )
	return -EINVAL;
    try {		// (no exception crosses the C ABI)
    const bool s16 = ( hio->flags & MIFSK_IO_HOST_S16 ) != 0;
    const size_t esz = s16 ? 2 : 4;
    std::vector<Row> rows(ns);
    for ( size_t i = 0; i < ns; i++ ) {
	uint32_t n = hio->d_nsamples ? hio->d_nsamples[i] : hio->nsamples;
	if ( ns > 1 && (size_t)n > hio->stream_stride )
	    n = (uint32_t)hio->stream_stride;		// never trust a length beyond the row
	rows[i] = Row{ (const char *)hio->d_samples + i * hio->stream_stride * esz, nullptr, 0, n, nullptr };
    }
    return mifsk::run_job(ctx, cfg, rows, s16, rxnoise, hio->flags & ~MIFSK_IO_HOST_S16, hio->stream_stride, *hio,
			  stats);
    } catch ( const std::bad_alloc & ) {
	return -ENOMEM;
    } catch ( ... ) {
	return -EIO;
    }
}

extern "C" int mifsk_demod_batch_host( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_demod_io *hio )
{
    return mifsk_demod_batch_host_ex(ctx, cfg, hio, 0.0f, nullptr);
}

extern "C" int mifsk_demod_long_batch_host( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const void *const *rows, const uint64_t *nsamples, int nstreams, unsigned src_flags, float rxnoise,
	const mifsk_time_split *params, const mifsk_demod_io *io_out, mifsk_time_split_stats *stats,
	mifsk_host_stats *hstats )
{
    if ( !ctx || !cfg || !io_out || !nsamples || !rows || nstreams <= 0 )
	return -EINVAL;
    if ( src_flags & ~MIFSK_IO_HOST_S16 )
	return -EINVAL;
    for ( int m = 0; m < nstreams; m++ )
	if ( nsamples[m] && !rows[m] )
	    return -EINVAL;
    if ( const int rc = mifsk::time_split_check_params(cfg, params) )
	return rc;
    if ( hstats )
	std::memset(hstats, 0, sizeof(*hstats));
    try {		// (no exception crosses the C ABI)
	std::vector<Row> lr((size_t)nstreams);
	for ( int m = 0; m < nstreams; m++ )
	    lr[(size_t)m] = Row{ rows[m], nullptr, 0, nsamples[m], nullptr };
	return mifsk::run_long(ctx, cfg, lr, ( src_flags & MIFSK_IO_HOST_S16 ) != 0, rxnoise, params, *io_out,
			       stats, hstats);
    } catch ( const std::bad_alloc & ) {
	return -ENOMEM;
    } catch ( ... ) {
	return -EIO;
    }
}

// ---------------------------------------------------------------------------
// a list of files -> one batch (what `minimodem --rx --file` does for one)
// ---------------------------------------------------------------------------

struct mifsk_files {
    struct Group {				// files of one (sample rate, sample format)
	mifsk_rx_config			cfg;
	std::vector<int>		members;	// indices into `files`
	size_t				fcap = 0, ecap = 0;
	std::vector<uint8_t>		bytes;
	std::vector<uint64_t>		bits;
	std::vector<mifsk_frame>	frames;
	std::vector<mifsk_episode>	eps;
	std::vector<uint32_t>		nbytes, nframes, neps, status;
	std::vector<int32_t>		band;
    };
    std::vector<mifsk_file_result>	files;
    std::vector<Group>			groups;
    std::vector<std::string>		paths;
    mifsk_host_stats			stats;
    // mifsk_demod_files_long: file i's plan and verification figures
    bool				time_split = false;
    std::vector<mifsk_time_split_stats>	tsplit;
};

// ---- headers (threads): format, rate, where the samples start, how many
static void read_headers( mifsk_files *F, const char *const *paths, int nfiles )
{
    F->files.resize((size_t)nfiles);
    F->paths.resize((size_t)nfiles);
    for ( int i = 0; i < nfiles; i++ ) {
	std::memset(&F->files[(size_t)i], 0, sizeof(mifsk_file_result));
	F->paths[(size_t)i] = paths[i] ? paths[i] : "";
	F->files[(size_t)i].carrier_band = -1;
    }
    mifsk::parallel_for((size_t)nfiles, mifsk::staging_threads(), [&]( size_t i ) {
	mifsk_file_result &fr = F->files[i];
	const int fd = open(F->paths[i].c_str(), O_RDONLY | O_CLOEXEC);
	if ( fd < 0 ) {
	    fr.error = -errno;
	    return;
	}
	struct stat st;
	if ( fstat(fd, &st) != 0 ) {
	    fr.error = -errno;
	    close(fd);
	    return;
	}
	// (the data chunk normally starts at byte 44; LIST / fact chunks in front of it are
	// rarely more than a few hundred bytes)
	std::vector<unsigned char> head(65536);
	const ssize_t got = pread(fd, head.data(), head.size(), 0);
	close(fd);
	if ( got < 0 ) {
	    fr.error = -errno;
	    return;
	}
	fr.error = mifsk::wav_parse_sized(head.data(), (size_t)got, (size_t)st.st_size, &fr.info);
	if ( !fr.error && fr.info.nframes > 0xFFFFFF00ull )
	    fr.error = -EFBIG;			// stream lengths are 32-bit on the device
    });
}

// ---- one group per (sample rate, sample format): the reference takes its sample rate from the
// file and derives everything from it (minimodem.c:1021-1032)
static void group_by_rate_and_format( mifsk_files *F, const mifsk_modem_args *args )
{
    std::map<std::pair<unsigned, int>, size_t> index;
    for ( size_t i = 0; i < F->files.size(); i++ ) {
	const mifsk_file_result &fr = F->files[i];
	if ( fr.error )
	    continue;
	const std::pair<unsigned, int> key(fr.info.sample_rate, fr.info.is_float);
	auto it = index.find(key);
	if ( it == index.end() ) {
	    mifsk_files::Group g;
	    mifsk_modem_args a = *args;
	    a.sample_rate = fr.info.sample_rate;
	    const int rc = mifsk_rx_config_init(&g.cfg, &a);
	    if ( rc ) {
		F->files[i].error = rc;		// (e.g. tones above this file's Nyquist rate)
		continue;
	    }
	    F->groups.push_back(std::move(g));
	    it = index.emplace(key, F->groups.size() - 1).first;
	}
	F->groups[it->second].members.push_back((int)i);
    }
}

// ---- length classes.  A batch's output arrays (host vectors, device slots, the copies back) are
// sized by its LONGEST file, so one hour-long recording among ten thousand short ones would cost
// every one of them the long one's capacity.  Each (rate, format) group is therefore cut, by
// length, into classes whose longest file is at most twice the shortest: a class is one batch with
// its own capacities, at most 2 x what its files need.
static void cut_into_length_classes( mifsk_files *F )
{
    std::vector<mifsk_files::Group> classes;
    for ( mifsk_files::Group &g : F->groups ) {
	std::stable_sort(g.members.begin(), g.members.end(), [&]( int a, int b ) {
	    return F->files[(size_t)a].info.nframes < F->files[(size_t)b].info.nframes;
	});
	size_t lo = 0;
	while ( lo < g.members.size() ) {
	    const uint64_t shortest = std::max<uint64_t>(F->files[(size_t)g.members[lo]].info.nframes, 4096);
	    size_t hi = lo;
	    while ( hi < g.members.size() && F->files[(size_t)g.members[hi]].info.nframes <= 2 * shortest )
		hi++;
	    mifsk_files::Group c;
	    c.cfg = g.cfg;
	    c.members.assign(g.members.begin() + (long)lo, g.members.begin() + (long)hi);
	    classes.push_back(std::move(c));
	    lo = hi;
	}
    }
    F->groups.swap(classes);
}

// a group's result vectors, sized by its longest file, as the host result arrays of either decode
static mifsk_demod_io size_group( const mifsk_files *F, mifsk_files::Group &g, unsigned flags )
{
    const size_t n = g.members.size();
    size_t maxn = 0;
    for ( int i : g.members )
	maxn = std::max(maxn, F->files[(size_t)i].info.nframes);
    g.fcap = mifsk_max_frames(&g.cfg, maxn);
    g.ecap = mifsk_max_episodes(&g.cfg, maxn);
    g.bits.assign(n * g.fcap, 0);
    g.bytes.assign(n * g.fcap, 0);
    if ( flags & MIFSK_FILES_WANT_FRAMES )
	g.frames.resize(n * g.fcap);
    g.eps.resize(n * g.ecap);
    g.nbytes.assign(n, 0); g.nframes.assign(n, 0); g.neps.assign(n, 0); g.status.assign(n, 0);
    g.band.assign(n, -1);
    mifsk_demod_io ho;
    std::memset(&ho, 0, sizeof(ho));
    ho.d_bytes = g.bytes.data();	ho.d_nbytes = g.nbytes.data();
    ho.d_bits = g.bits.data();
    ho.d_frames = g.frames.empty() ? nullptr : g.frames.data();
    ho.d_nframes = g.nframes.data();	ho.frames_cap = g.fcap;
    ho.d_episodes = g.eps.data();	ho.d_nepisodes = g.neps.data();	ho.episodes_cap = g.ecap;
    ho.d_status = g.status.data();
    ho.d_carrier_band = g.band.data();
    return ho;
}

// `long_params`: the groups are decoded through the time split (mifsk_demod_files_long) with these
// parameters, each (sample rate, sample format) group as one batch of long recordings -- a few
// long recordings, and one plan cuts the whole group: no length classes
static int demod_files_impl( mifsk_ctx *ctx, const mifsk_modem_args *args,
	const char *const *paths, int nfiles, float rxnoise, unsigned flags, mifsk_files *F,
	const mifsk_time_split *long_params )
{
    std::memset(&F->stats, 0, sizeof(F->stats));
    F->time_split = long_params != nullptr;
    if ( long_params )
	F->tsplit.assign((size_t)nfiles, mifsk_time_split_stats{});
    const double t0 = mifsk::now_s();
    read_headers(F, paths, nfiles);
    group_by_rate_and_format(F, args);
    if ( !long_params )
	cut_into_length_classes(F);
    int rc_all = 0;
    for ( mifsk_files::Group &g : F->groups ) {
	const size_t n = g.members.size();
	const mifsk_demod_io ho = size_group(F, g, flags);
	const bool s16 = !F->files[(size_t)g.members[0]].info.is_float;
	std::vector<Row> rows(n);
	for ( size_t k = 0; k < n; k++ ) {
	    mifsk_file_result &fr = F->files[(size_t)g.members[k]];
	    rows[k] = Row{ nullptr, F->paths[(size_t)g.members[k]].c_str(), fr.info.data_offset, fr.info.nframes,
			   &fr.error };
	}
	int rc;
	if ( long_params ) {
	    std::vector<mifsk_time_split_stats> ts(n);
	    rc = mifsk::run_long(ctx, &g.cfg, rows, s16, rxnoise, long_params, ho, ts.data(), &F->stats);
	    for ( size_t k = 0; k < n; k++ )
		F->tsplit[(size_t)g.members[k]] = ts[k];
	} else {
	    rc = mifsk::run_job(ctx, &g.cfg, rows, s16, rxnoise,
				flags & ( MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP ), 0, ho,
				&F->stats);
	}
	if ( rc && !rc_all )
	    rc_all = rc;
	for ( size_t k = 0; k < n; k++ ) {
	    mifsk_file_result &fr = F->files[(size_t)g.members[k]];
	    fr.cfg = &g.cfg;
	    if ( fr.error )
		continue;			// (could not be read after all: its row was zeros)
	    fr.nframes = g.nframes[k] < g.fcap ? g.nframes[k] : (uint32_t)g.fcap;
	    fr.nbytes = g.nbytes[k] < g.fcap ? g.nbytes[k] : (uint32_t)g.fcap;
	    fr.nepisodes = g.neps[k] < g.ecap ? g.neps[k] : (uint32_t)g.ecap;
	    fr.status = g.status[k];
	    fr.carrier_band = g.band[k];
	    fr.bits = g.bits.data() + k * g.fcap;
	    fr.bytes = g.bytes.data() + k * g.fcap;
	    fr.frames = g.frames.empty() ? nullptr : g.frames.data() + k * g.fcap;
	    fr.episodes = g.eps.data() + k * g.ecap;
	}
    }
    F->stats.seconds_total = mifsk::now_s() - t0;	// headers and grouping included
    // a file that could not be read is that file's error (mifsk_file_result.error), not the
    // batch's: the decodes report only what stopped the pipeline (HIP, allocation)
    return rc_all;
}

static int demod_files_entry( mifsk_ctx *ctx, const mifsk_modem_args *args, const char *const *paths,
	int nfiles, float rxnoise, unsigned flags, const mifsk_time_split *long_params, mifsk_files **out )
{
    if ( !ctx || !args || !out || nfiles < 0 || ( nfiles && !paths ) )
	return -EINVAL;
    *out = nullptr;
    mifsk_files *F = new (std::nothrow) mifsk_files();
    if ( !F )
	return -ENOMEM;
    int rc;
    try {		// (no exception crosses the C ABI: the vectors above can throw)
	rc = demod_files_impl(ctx, args, paths, nfiles, rxnoise, flags, F, long_params);
    } catch ( const std::bad_alloc & ) {
	delete F;
	return -ENOMEM;
    } catch ( ... ) {
	delete F;
	return -EIO;
    }
    *out = F;
    return rc;
}

extern "C" int mifsk_demod_files( mifsk_ctx *ctx, const mifsk_modem_args *args,
	const char *const *paths, int nfiles, float rxnoise, unsigned flags, mifsk_files **out )
{
    return demod_files_entry(ctx, args, paths, nfiles, rxnoise, flags, nullptr, out);
}

extern "C" int mifsk_demod_files_long( mifsk_ctx *ctx, const mifsk_modem_args *args,
	const char *const *paths, int nfiles, float rxnoise, unsigned flags, const mifsk_time_split *params,
	mifsk_files **out )
{
    if ( !ctx || !args || !out || nfiles < 0 || ( nfiles && !paths ) )
	return -EINVAL;
    *out = nullptr;
    mifsk_time_split p;
    std::memset(&p, 0, sizeof(p));
    if ( params )
	p = *params;
    p.flags |= flags & ( MIFSK_IO_RING_EXACT | MIFSK_IO_ENGINE_WAVE | MIFSK_IO_ENGINE_WORKGROUP );
    if ( p.flags & MIFSK_IO_RING_EXACT )
	return -ENOTSUP;		// (before any file is opened)
    return demod_files_entry(ctx, args, paths, nfiles, rxnoise, flags, &p, out);
}

extern "C" const mifsk_time_split_stats *mifsk_files_time_split( const mifsk_files *f, int i )
{
    if ( !f || !f->time_split || i < 0 || (size_t)i >= f->files.size() || f->files[(size_t)i].error )
	return nullptr;
    return &f->tsplit[(size_t)i];
}

extern "C" int mifsk_files_count( const mifsk_files *f ) { return f ? (int)f->files.size() : 0; }

extern "C" const mifsk_file_result *mifsk_files_get( const mifsk_files *f, int i )
{
    return ( f && i >= 0 && (size_t)i < f->files.size() ) ? &f->files[(size_t)i] : nullptr;
}

extern "C" const mifsk_host_stats *mifsk_files_stats( const mifsk_files *f ) { return f ? &f->stats : nullptr; }

extern "C" void mifsk_files_free( mifsk_files *f ) { delete f; }
