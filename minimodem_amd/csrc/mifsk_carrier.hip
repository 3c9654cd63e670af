// mifsk_carrier.hip -- mifsk_detect_carrier_batch (include/mifsk.h): fsk_detect_carrier
// (fsk.c:543-581) on windows of every stream of a batch, and the two host helpers that go with it.
//
// The work is windows x bands x samples double-precision FMA pairs, far more arithmetic than bytes,
// so the kernel is laid out around what feeds the FP64 pipe:
//   * a lane owns NB bands (b, b + 64) and kCarW windows: 2 * NB * kCarW independent accumulator
//     chains.  The twiddle index k = (b n) mod N does not depend on the window, so ONE table read
//     per band and sample feeds 2 * kCarW FMAs; a sample is the same for all lanes of a wave, so
//     ONE broadcast read per window and sample feeds 2 * NB FMAs.
//   * samples are staged per workgroup into LDS, kCarTile samples of each of its windows at a time,
//     widened to double once on the way (PCM16 converted by sample_from_s16, in float); a window
//     of any length is walked in such tiles, the accumulators stay in registers across them.
//   * the table (16 bytes per entry, fftsize entries) sits in LDS when it fits beside the samples
//     (TWLDS), one pad entry after every 16 so that the strides b n that are multiples of 16 entries
//     do not put a group of lanes on one bank; otherwise every lane reads its entry from memory
//     (L2).  Either way k is walked incrementally, as spectrum_kernel and wave_detect_window do.
//   * a workgroup of 4 or 8 waves takes WG groups of kCarW windows and all band groups: with fewer
//     band groups than waves the waves split the windows, otherwise wave i takes band groups i,
//     i + waves, ... in rounds (the samples are staged again per round: 1 load per 128 FMA pairs).
//   * the peak pick: per lane over its ascending bands, then the wave's shuffle reduction with
//     wave_detect_window's rule, then the waves' results through LDS.
// The sums are the oracle's in the oracle's order (re, im from 0.0, n ascending, one fma each), the
// magnitude is band_mag(): nothing of either is restated differently here.  No f64 MFMA: its
// internal summation is not that chain.  The kernel reads nothing it wrote, so it needs no fences;
// the outputs are plain vector stores.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "mifsk.h"
#include "mifsk_batch.h"
#include "mifsk_ctx.h"
#include "mifsk_devlib.h"

namespace mifsk {

constexpr int kCarW = 8;				// windows per lane
constexpr uint32_t kCarTile = 64u;			// samples of each window staged at a time
constexpr uint32_t kCarMaxLds = 160u * 1024u;		// a workgroup may have all of a CU's LDS
constexpr uint32_t kCarBigTable = 40u * 1024u;		// a table beyond this: one workgroup of 8 waves per CU

struct CarrierArgs {
    const double	*cs;		// the context's spectrum table, [N][2]
    RowsIn		in;		// rows of float or int16_t
    uint32_t		s16;		// the rows hold PCM16
    float		dc;		// rxnoise_term(): PCM16 only
    uint64_t		first;
    uint32_t		window, hop, nwindows;
    float		threshold, magscalar;
    uint32_t		N, nbands;
    uint32_t		s0;		// first stream of this launch
    uint32_t		G;		// band groups of 64 * NB bands
    uint32_t		WG;		// groups of kCarW windows a workgroup takes at a time
    int32_t		*band;
    float		*mag;
    float		*spectrum;
};

struct CarrierPeak {
    float	mag;
    int32_t	band;
};

// words of the table's image in LDS: entry k sits in slot k + k / 16
__host__ __device__ inline uint32_t carrier_table_slots( uint32_t N ) { return N + ( N >> 4 ) + 1u; }

// one tile of tl samples of the lane's kCarW windows (xw: window w's at xw[w * kCarTile ..]) onto
// its accumulators; k[j] = (b_j n) mod N walks on
template <int NB, bool TWLDS>
__device__ __forceinline__ void carrier_tile( const double2 *tw, const double *__restrict__ cs, const double *xw,
	uint32_t tl, uint32_t N, uint32_t (&k)[NB], const uint32_t (&kstep)[NB],
	double (&re)[kCarW][NB], double (&im)[kCarW][NB] )
{
#pragma unroll 2
    for ( uint32_t e = 0; e < tl; e++ ) {
	double2 c[NB];
#pragma unroll
	for ( int j = 0; j < NB; j++ ) {
	    const uint32_t kk = k[j];
	    if constexpr ( TWLDS )
		c[j] = tw[kk + ( kk >> 4 )];
	    else
		c[j] = *reinterpret_cast<const double2 *>(cs + 2 * (size_t)kk);
	    k[j] = kk + kstep[j];
	    if ( k[j] >= N )
		k[j] -= N;
	}
#pragma unroll
	for ( int w = 0; w < kCarW; w++ ) {
	    const double x = xw[(uint32_t)w * kCarTile + e];	// one address for the whole wave
#pragma unroll
	    for ( int j = 0; j < NB; j++ ) {
		re[w][j] = fma(x, c[j].x, re[w][j]);
		im[w][j] = fma(x, c[j].y, im[w][j]);
	    }
	}
    }
}

// NB: bands per lane.  TWLDS: the table is in LDS.
template <int NB, bool TWLDS>
__global__ __launch_bounds__(512)
void carrier_survey_kernel( const CarrierArgs A )
{
    extern __shared__ double2 car_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const uint32_t N = A.N, nbands = A.nbands, window = A.window;
    const uint32_t WB = A.WG * (uint32_t)kCarW;			// windows of a workgroup's chunk
    // LDS: the table's image | WB * kCarTile staged samples | a peak per wave and window
    double2 *tw = car_lds;
    double *xs = reinterpret_cast<double *>(car_lds + ( TWLDS ? carrier_table_slots(N) : 0u ));
    CarrierPeak *part = reinterpret_cast<CarrierPeak *>(xs + WB * kCarTile);
    if constexpr ( TWLDS ) {
	for ( uint32_t k = tid; k < N; k += blockDim.x )
	    tw[k + ( k >> 4 )] = *reinterpret_cast<const double2 *>(A.cs + 2 * (size_t)k);
	// (the first tile's barriers come before any read of it)
    }

    const uint32_t s = A.s0 + blockIdx.y;
    const uint32_t n_row = A.in.nsamples_v ? A.in.nsamples_v[s] : A.in.nsamples_u;
    const uint32_t nv = n_row < A.in.stride ? n_row : (uint32_t)A.in.stride;	// samples the row holds
    const float *rowf = reinterpret_cast<const float *>(A.in.x) + (size_t)s * A.in.stride;
    const int16_t *rowh = reinterpret_cast<const int16_t *>(A.in.x) + (size_t)s * A.in.stride;
    // windows that lie wholly inside the row, of those the outputs have room for: window w < nuse
    // reads x[first + w * hop + n] with n < window, all below nv
    uint64_t nfit = 0;
    if ( A.first <= nv && nv - A.first >= window )
	nfit = ( nv - A.first - window ) / A.hop + 1u;
    const uint64_t nuse = nfit < A.nwindows ? nfit : A.nwindows;
    const size_t out0 = (size_t)s * A.nwindows;

    const uint32_t ntasks = A.G * A.WG;				// (band group, window group) pairs
    const uint32_t nrounds = ( ntasks + nwaves - 1u ) / nwaves;	// (1 when WG > 1: then ntasks <= nwaves)
    const uint32_t nchunks = (uint32_t)( ( (uint64_t)A.nwindows + WB - 1u ) / WB );
    for ( uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x ) {
	const uint64_t w0 = (uint64_t)c * WB;
	if ( w0 >= nuse ) {					// (the whole workgroup) nothing to evaluate
	    for ( uint32_t t = tid; t < WB; t += blockDim.x )
		if ( w0 + t < A.nwindows ) {
		    A.band[out0 + w0 + t] = MIFSK_CARRIER_NO_WINDOW;
		    if ( A.mag )
			A.mag[out0 + w0 + t] = 0.0f;
		}
	    continue;
	}
	float best[kCarW];
	int32_t best_band[kCarW];
#pragma unroll
	for ( int w = 0; w < kCarW; w++ ) {
	    best[w] = 0.0f;
	    best_band[w] = -1;
	}
	for ( uint32_t r = 0; r < nrounds; r++ ) {
	    const uint32_t task = wave + r * nwaves;
	    const bool busy = task < ntasks;			// (per wave)
	    const uint32_t g = A.WG > 1u ? task % A.G : task;
	    const uint32_t wg = A.WG > 1u && busy ? task / A.G : 0u;
	    uint32_t b[NB], k[NB], kstep[NB];
	    bool active[NB];
	    double re[kCarW][NB], im[kCarW][NB];
#pragma unroll
	    for ( int j = 0; j < NB; j++ ) {
		b[j] = ( g * (uint32_t)NB + (uint32_t)j ) * 64u + lane;
		active[j] = busy && b[j] < nbands;
		k[j] = 0;
		kstep[j] = ( active[j] ? b[j] : 1u ) % N;	// a lane without a band shadows band 1
#pragma unroll
		for ( int w = 0; w < kCarW; w++ ) {
		    re[w][j] = 0.0;
		    im[w][j] = 0.0;
		}
	    }
	    for ( uint32_t n0 = 0; n0 < window; n0 += kCarTile ) {
		const uint32_t tl = window - n0 < kCarTile ? window - n0 : kCarTile;
		__syncthreads();				// the tile before has been read
		for ( uint32_t i = tid; i < WB * kCarTile; i += blockDim.x ) {
		    const uint32_t t = i / kCarTile, e = i % kCarTile;
		    float v = 0.0f;
		    if ( e < tl && w0 + t < nuse ) {
			const uint64_t at = A.first + ( w0 + t ) * A.hop + n0 + e;	// < nv
			v = A.s16 ? sample_from_s16((int)rowh[at], A.dc) : rowf[at];
		    }
		    xs[i] = (double)v;
		}
		__syncthreads();
		if ( busy )
		    carrier_tile<NB, TWLDS>(tw, A.cs, xs + wg * (uint32_t)kCarW * kCarTile, tl, N, k, kstep, re, im);
	    }
	    if ( busy ) {
#pragma unroll
		for ( int w = 0; w < kCarW; w++ ) {
		    const uint64_t widx = w0 + wg * (uint32_t)kCarW + (uint32_t)w;
#pragma unroll
		    for ( int j = 0; j < NB; j++ ) {		// ascending bands per lane (fsk.c:570-575)
			const float m = band_mag(re[w][j], im[w][j], A.magscalar);
			if ( A.spectrum && active[j] && widx < nuse )
			    A.spectrum[( out0 + widx ) * nbands + b[j]] = m;
			if ( active[j] && b[j] >= 1u && !( m < A.threshold ) && best[w] < m ) {
			    best[w] = m;
			    best_band[w] = (int32_t)b[j];
			}
		    }
		}
	    }
	}
	// first strict maximum over all bands = largest magnitude, lowest band on ties
#pragma unroll
	for ( int w = 0; w < kCarW; w++ ) {
	    float m = best[w];
	    int32_t bb = best_band[w];
#pragma unroll
	    for ( int o = 32; o > 0; o >>= 1 ) {
		const float m2 = __shfl_xor(m, o);
		const int32_t b2 = __shfl_xor(bb, o);
		const bool take = b2 >= 0 && ( bb < 0 || m2 > m || ( m2 == m && b2 < bb ) );
		if ( take ) {
		    m = m2;
		    bb = b2;
		}
	    }
	    if ( lane == 0u )
		part[wave * (uint32_t)kCarW + (uint32_t)w] = CarrierPeak{m, bb};
	}
	__syncthreads();
	for ( uint32_t t = tid; t < WB; t += blockDim.x ) {
	    const uint64_t widx = w0 + t;
	    if ( widx >= A.nwindows )
		continue;
	    float m = 0.0f;
	    int32_t bb = MIFSK_CARRIER_NO_WINDOW;
	    if ( widx < nuse ) {
		bb = MIFSK_CARRIER_NONE;
		const uint32_t wg = t / (uint32_t)kCarW, w = t % (uint32_t)kCarW;
		// the waves that took this window: with WG > 1 wave i took window group i / G
		for ( uint32_t i = 0; i < nwaves; i++ ) {
		    if ( A.WG > 1u && ( i >= ntasks || i / A.G != wg ) )
			continue;
		    const CarrierPeak p = part[i * (uint32_t)kCarW + w];
		    if ( p.band >= 0 && ( bb < 0 || p.mag > m || ( p.mag == m && p.band < bb ) ) ) {
			m = p.mag;
			bb = p.band;
		    }
		}
	    }
	    A.band[out0 + widx] = bb;
	    if ( A.mag )
		A.mag[out0 + widx] = m;
	}
	// (part is written again only behind the next chunk's barriers)
    }
}

namespace {

// the negative shift --auto-carrier applies, in the reference's float arithmetic
// (minimodem.c:1203-1206; demod_batch_wave in mifsk_capi.cpp)
int carrier_b_shift( const mifsk_rx_config *cfg )
{
    int b_shift = - (float)( cfg->autodetect_shift + cfg->band_width / 2.0f ) / cfg->band_width;
    if ( cfg->inverted_freqs )
	b_shift *= -1;
    return b_shift;
}

} // namespace
} // namespace mifsk

extern "C" uint64_t mifsk_carrier_windows( uint64_t nsamples, uint64_t first, uint32_t window, uint32_t hop )
{
    if ( first > nsamples || nsamples - first < window )
	return 0;
    if ( hop == 0 )
	hop = window;
    if ( hop == 0 )
	return 0;				// (window 0, hop 0: no window at all)
    return ( nsamples - first - window ) / hop + 1u;
}

extern "C" int mifsk_carrier_tones( const mifsk_rx_config *cfg, int band, unsigned *b_mark, unsigned *b_space,
	float *mark_f, float *space_f )
{
    if ( !cfg || band < 1 || (unsigned)band >= cfg->nbands )
	return -EINVAL;
    const int b_shift = mifsk::carrier_b_shift(cfg);
    if ( b_shift == 0 )
	return -EINVAL;				// assert in fsk_set_tones_by_bandshift (fsk.c:587)
    const long long space = (long long)band + b_shift;
    if ( space < 1 || space >= (long long)cfg->nbands )
	return -ERANGE;				// minimodem.c:1207-1213: the detection is dropped
    if ( b_mark ) *b_mark = (unsigned)band;
    if ( b_space ) *b_space = (unsigned)space;
    if ( mark_f ) *mark_f = (unsigned)band * cfg->band_width;	// fsk.c:595-596
    if ( space_f ) *space_f = (unsigned)space * cfg->band_width;
    return 0;
}

extern "C" int mifsk_detect_carrier_batch( mifsk_ctx *ctx, const mifsk_rx_config *cfg,
	const mifsk_carrier_io *io, void *stream )
{
    using namespace mifsk;
    if ( !ctx || !cfg || !io || !io->d_samples || !io->d_band )
	return -EINVAL;
    if ( io->nstreams <= 0 || io->nwindows == 0 )
	return -EINVAL;
    if ( int rc = feed_rows_check(io->kind, io->rxnoise, io->d_samples, io->stream_stride) )
	return rc;
    const bool s16 = io->kind == MIFSK_FEED_S16;
    if ( int rc = mifsk_check_cfg(cfg) )
	return rc;
    if ( cfg->nbands < 2 )
	return -EINVAL;
    const uint32_t N = (uint32_t)cfg->fftsize;
    uint32_t window = io->window;
    if ( window == 0 ) {			// what --auto-carrier scans with (minimodem.c:1179-1190)
	const float nps = cfg->nsamples_per_bit > (float)cfg->fftsize ? (float)cfg->fftsize : cfg->nsamples_per_bit;
	window = nps >= 1.0f ? (uint32_t)nps : 0u;
    }
    if ( window == 0 || window > N )
	return -EINVAL;			// assert in fsk_detect_carrier (fsk.c:547)
    if ( (uint64_t)cfg->nbands * window > 0xFFFFFFFFull )
	return -EINVAL;			// (b * n is reduced in 32 bits on the device)
    if ( io->d_spectrum && (uint64_t)io->nwindows * cfg->nbands > 0xFFFFFFFFull )
	return -EINVAL;

    std::shared_lock<std::shared_mutex> gate;	// held until the launches are enqueued
    DevCfg d;
    const double *d_tw = nullptr;
    if ( int rc = lookup_tables(ctx, cfg, gate, d, &d_tw) )
	return rc;
    const double *d_cs = nullptr;
    if ( int rc = get_cs(ctx, N, &d_cs) )
	return rc;

    CarrierArgs A = {};
    A.cs = d_cs;
    A.in = rows_in(io);
    A.s16 = s16 ? 1u : 0u;
    A.dc = s16 ? rxnoise_term(io->rxnoise) : 0.0f;
    A.first = io->first;
    A.window = window;
    A.hop = io->hop ? io->hop : window;
    A.nwindows = io->nwindows;
    A.threshold = io->threshold;
    A.magscalar = 1.0f / ( (float)window / 2.0f );		// fsk.c:553
    A.N = N;
    A.nbands = cfg->nbands;
    A.band = io->d_band;
    A.mag = io->d_mag;
    A.spectrum = io->d_spectrum;

    // two bands per lane once there are more bands than a wave has lanes; the table in LDS when it
    // fits beside the samples, and then -- a big one leaves room for one workgroup per CU -- 8 waves
    const int nb = cfg->nbands > 64u ? 2 : 1;
    A.G = ( cfg->nbands + 64u * (uint32_t)nb - 1u ) / ( 64u * (uint32_t)nb );
    const size_t table = (size_t)carrier_table_slots(N) * sizeof(double2);
    auto shape = [&]( unsigned waves, bool tw_lds, size_t &lds ) {
	A.WG = A.G < waves ? waves / A.G : 1u;
	lds = ( tw_lds ? table : 0u ) + (size_t)A.WG * kCarW * kCarTile * sizeof(double)
	    + (size_t)waves * kCarW * sizeof(CarrierPeak);
    };
    unsigned waves = table > kCarBigTable ? 8u : 4u;
    size_t lds = 0;
    bool tw_lds = true;
    shape(waves, true, lds);
#ifdef MIFSK_CARRIER_TABLE_L2		/* (measurement builds: make variant TAG=twl2 DEFS=-DMIFSK_CARRIER_TABLE_L2) */
    lds = kCarMaxLds + 1u;
#endif
    if ( lds > kCarMaxLds ) {
	tw_lds = false;
	waves = 4u;
	shape(waves, false, lds);
    }
    const uint32_t WB = A.WG * (uint32_t)kCarW;
    const uint32_t nchunks = (uint32_t)( ( (uint64_t)A.nwindows + WB - 1u ) / WB );
    const hipStream_t st = (hipStream_t)stream;
    return for_row_blocks((uint32_t)io->nstreams, [&]( uint32_t s0, uint32_t rows ) {
	// a workgroup walks several chunks of a row once the chip is full: the table is loaded once
	uint32_t gx = ( 8u * (uint32_t)ctx->ncu + rows - 1u ) / rows;
	gx = gx < nchunks ? gx : nchunks;
	A.s0 = s0;
	const dim3 grid(gx, rows), block(64u * waves);
	if ( nb == 2 )
	    return tw_lds ? launch_lds(carrier_survey_kernel<2, true>, grid, block, lds, st, A)
			  : launch_lds(carrier_survey_kernel<2, false>, grid, block, lds, st, A);
	return tw_lds ? launch_lds(carrier_survey_kernel<1, true>, grid, block, lds, st, A)
		      : launch_lds(carrier_survey_kernel<1, false>, grid, block, lds, st, A);
    });
}
