// mifsk_selftest.hip -- the device arithmetic of mifsk_devlib.h / mifsk_devmath.h, one value or
// one frame per thread, for the host to compare with an independent reference
// (mifsk_selftest_rcp / _mag / _confidence in include/mifsk.h; tests/test_gpu_devmath.py; _gauss:
// the noise field's transform of mifsk_gauss.h, tests/test_gpu_impair.py; _turn: the FM stage's
// angle of mifsk_angle.h, tests/test_gpu_fm.py), and the
// wave-wide routines -- the correlators, the replay's lane scans, the wave maximum -- one window
// or one frame per LANE of whole waves (mifsk_selftest_corr / _scan / _wave_max;
// tests/test_gpu_correlators.py, tests/test_gpu_scans.py).
//
// The kernels CALL the routines the receive loops call and restate nothing; a translation unit
// of their own, so that no receive kernel's code depends on what is here.  What this pins is the
// routines' arithmetic as the compiler inlines it into these kernels, not how it schedules them
// inside a receive loop (every parity test compares that with the oracle, on real audio).
// gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <vector>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"
#include "mifsk_devlib.h"
#include "mifsk_gauss.h"
#include "mifsk_angle.h"

namespace mifsk {

// rc[i] = rcp_of_float(c[i]); q[i] = div_by_rcp(x[i], rc[i])
__global__ __launch_bounds__(256)
void selftest_rcp_kernel( const float *__restrict__ c, const float *__restrict__ x, uint64_t n,
	double *__restrict__ rc_out, float *__restrict__ q_out )
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n )
	return;
    const double rc = rcp_of_float(c[i]);
    rc_out[i] = rc;
    q_out[i] = div_by_rcp(x[i], rc);
}

// z[i] = { R(w[i].x) C(w[i].y), R(w[i].x) S(w[i].y) } (mifsk_gauss.h)
__global__ __launch_bounds__(256)
void selftest_gauss_kernel( const uint2 *__restrict__ w, uint64_t n, double2 *__restrict__ z_out )
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n )
	return;
    const uint2 wi = w[i];
    double z0, z1;
    mifsk_gauss_pair(wi.x, wi.y, &z0, &z1);
    z_out[i] = double2{z0, z1};
}

// t[i] = mifsk_turn(y[i], x[i]) (mifsk_angle.h)
__global__ __launch_bounds__(256)
void selftest_turn_kernel( const double *__restrict__ y, const double *__restrict__ x, uint64_t n,
	double *__restrict__ t_out )
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n )
	return;
    t_out[i] = mifsk_turn(y[i], x[i]);
}

// s as band_mag() builds it from (re[i], im[i]); root[i] = sqrt_sumsq(s); g[i], unsafe[i] =
// sqrt_newton1(s); mag[i] = band_mag(re[i], im[i], scalar)
__global__ __launch_bounds__(256)
void selftest_mag_kernel( const double *__restrict__ re, const double *__restrict__ im, float scalar, uint64_t n,
	double *__restrict__ root_out, double *__restrict__ g_out, uint8_t *__restrict__ unsafe_out,
	float *__restrict__ mag_out )
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n )
	return;
    const float fr = (float)re[i], fi = (float)im[i];
    const double s = __builtin_fma((double)fr, (double)fr, (double)fi * (double)fi);
    root_out[i] = sqrt_sumsq(s);
    bool unsafe;
    g_out[i] = sqrt_newton1(s, unsafe);
    unsafe_out[i] = unsafe ? 1u : 0u;
    mag_out[i] = band_mag(re[i], im[i], scalar);
}

// Case i on global thread i: wave w holds cases 64 w .. 64 w + 63, so the caller decides which
// frames share a wave -- and with it the wave-wide vote that sends every lane of a wave through
// the divisions proper.  Lanes beyond ncases leave before the call, as idle lanes of a receive
// loop do.
template <int VARIANT>
__global__ __launch_bounds__(256)
void selftest_confidence_kernel( const float2 *__restrict__ mags, uint64_t ncases, uint32_t n_bits,
	uint64_t req_mask, uint64_t req_val, float *__restrict__ conf, float *__restrict__ ampl,
	unsigned long long *__restrict__ bits, uint32_t *__restrict__ fell_back )
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= ncases )
	return;
    const float2 *m = mags + i * n_bits;
    uint32_t fb = 0u;
    FrameOut f;
    if ( VARIANT == 0 )
	f = frame_confidence(m, req_mask, req_val, n_bits);
    else if ( VARIANT == 1 )
	f = frame_confidence_any(m, req_mask, req_val, n_bits, fb);
    else
	f = frame_confidence_any_staged(m, req_mask, req_val, n_bits, fb);
    conf[i] = f.conf;
    ampl[i] = f.ampl;
    bits[i] = f.bits;
    fell_back[i] = fb;
}

// ---------------------------------------------------------------------------
// The correlators.  One wave per block, case 64 w + l on lane l of wave w; EVERY lane runs the
// routine (the DPP broadcasts need them all): a lane beyond the wave's cases shadows the wave's
// first case, as idle lanes of the receive loops shadow a real window, and stores nothing.
// The host entry has checked every precondition (alignment, reach, LDS room): nothing here
// reads or writes outside `x[0 .. N)` rounded up to whole float4s, or outside its LDS.
// ---------------------------------------------------------------------------
struct CorrArgs {
    const DevCfg	*cfg;		// the planner's DevCfg (skew as the caller forced it)
    const double	*tw;		// the context's table for this configuration
    const float		*x;		// N samples, the array padded with zeros to whole float4s
    uint32_t		N;
    const uint32_t	*starts;	// window (segment) start per case
    const uint32_t	*lens;		// MIFSK_SELFTEST_CORR_SEG_GROUP: segment length per case
    uint32_t		ncases;
    uint32_t		lo;		// _SKEWED_STREAM: the sample in row 0, word 0 of the slab
    uint32_t		lds_floats;	// floats of dynamic LDS
    uint32_t		never_whole;	// _SEG_GROUP: mask every group, also those below the shortest segment
    double		*acc;		// [ncases][4]
    float		*esum;		// [ncases], _SEG_GROUP only
};

template <int R, int NQ>
__global__ __launch_bounds__(64)
void selftest_corr_kernel( const CorrArgs A )
{
    extern __shared__ float4 corr_lds4[];
    float *lds = reinterpret_cast<float *>(corr_lds4);
    const DevCfg &cfg = *A.cfg;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c0 = 64u * blockIdx.x;
    const uint32_t nw = A.ncases - c0 < 64u ? A.ncases - c0 : 64u;	// cases of this wave (uniform)
    const bool active = lane < nw;
    const uint32_t c = c0 + ( active ? lane : 0u );
    const uint32_t a = A.starts[c];
    const uint32_t B = cfg.bit_nsamples, N = A.N;
    const float *x = A.x;
    const double *tw = A.tw;
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
    float energy = 0.0f;

    if constexpr ( R <= MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN || R == MIFSK_SELFTEST_CORR_SLAB_PLAIN ) {
	// the samples as they are, sample i in word i; zeros up to the end of the region
	for ( uint32_t i = lane; i < A.lds_floats; i += 64u )
	    lds[i] = i < N ? x[i] : 0.0f;
	wave_lds_sync();
    }
    if constexpr ( R == MIFSK_SELFTEST_CORR_LDS_FIXED || R == MIFSK_SELFTEST_CORR_LDS_FIXED_HALVES ) {
	TwGroup tg[3];
#pragma unroll
	for ( int g = 0; g < 3; g++ )
	    tg[g] = tw_group_load(tw, (uint32_t)g, lane);	// (the table never has fewer than three groups)
	if constexpr ( R == MIFSK_SELFTEST_CORR_LDS_FIXED )
	    corr_lds_fixed<NQ>(tg, lds + a, acc);
	else
	    corr_lds_fixed_halves<NQ>(tg, lds + a, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_LDS_STREAM ) {
	corr_lds_stream(tw, lds + a, B >> 2, lane, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN ) {
	corr_lds_stream_lean(tw, lds + a, B >> 2, lane, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_GLOBAL_STREAM ) {
	corr_global_stream(tw, x + a, B, lane, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_GLOBAL_TILED ) {
	corr_global_tiled(tw, x, a, nw, B, lane, lds, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_SLAB_PLAIN ) {
	corr_slab_plain(tw, lds + a, B, lane, acc);
    } else if constexpr ( R == MIFSK_SELFTEST_CORR_SKEWED_STREAM ) {
	// [lo, N) into the slab whose row 0 starts at sample lo, as the receive loops stage a
	// search's span (Wave::stage_slab): whole aligned float4s from the one below lo on
	const uint32_t lo = A.lo, org4 = lo & ~3u, head = lo - org4, cap = N - lo;
	const uint32_t nvec = ( cap + head + 3u ) >> 2;
	for ( uint32_t v0 = 0; v0 < nvec; v0 += 64u ) {
	    const uint32_t v = v0 + lane;
	    if ( v < nvec )
		store4_skewed(cfg, lds, cap, v << 2, head, load4_raw(x, org4 + ( v << 2 ), N), org4 + ( v << 2 ), N);
	}
	wave_lds_sync();
	corr_skewed_stream(cfg, tw, lds, a - lo, lane, acc);
    } else {
	// MIFSK_SELFTEST_CORR_SEG_GROUP: every lane sums a segment of its own length in lock step
	// over the wave's longest, group by group from the table's first entry on (a segment's
	// phase origin is its own start); groups below the wave's shortest segment go unmasked
	const uint32_t len = A.lens[c];
	const uint32_t lmax = wave_max_u32(len), lmin = wave_min_u32(len);
	const uint32_t ng = ( lmax + 15u ) >> 4;
	float2v esum = { 0.0f, 0.0f };
	for ( uint32_t gi = 0; gi < ng; gi++ ) {
	    const TwGroup G = tw_group_load(tw, gi, lane);
	    float xs[16];
#pragma unroll
	    for ( int j = 0; j < 16; j++ ) {
		const uint32_t idx = a + 16u * gi + (uint32_t)j;
		xs[j] = idx < N ? x[idx] : 0.0f;		// (what lies beyond a lane's length is masked)
	    }
	    seg_group(acc, esum, G, make_float4(xs[0], xs[1], xs[2], xs[3]), make_float4(xs[4], xs[5], xs[6], xs[7]),
		      make_float4(xs[8], xs[9], xs[10], xs[11]), make_float4(xs[12], xs[13], xs[14], xs[15]),
		      16u * gi, len, !A.never_whole && 16u * gi + 16u <= lmin);
	}
	energy = esum.x + esum.y;				// (as Wave::seg_correlate keeps it)
    }
    if ( active ) {
	double *o = A.acc + 4 * (size_t)c;
	o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
	if ( R == MIFSK_SELFTEST_CORR_SEG_GROUP )
	    A.esum[c] = energy;
    }
}

// ---------------------------------------------------------------------------
// The lane scans of the bulk replay, seeded exactly as the receive loops seed them
// (Wave::master_loop in mifsk_wave.hip, master_loop in mifsk_kernels.hip): wave w replays K[w]
// candidates (cv, av; lanes at or beyond K carry zeros) from the state before frame 0.
// R 0: replay_scan_asm, 1: replay_scan_soft, 2: replay_scan_track.  Every lane's x* (the state
// after its frame) and b* (the state before it) come back, as (track, peak, confidence total,
// amplitude total).
// ---------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256)
void selftest_scan_kernel( const float4 *__restrict__ state, const float *__restrict__ cv_in,
	const float *__restrict__ av_in, const uint32_t *__restrict__ Ks, uint32_t nwaves, bool totals,
	float4 *__restrict__ x_out, float4 *__restrict__ b_out )
{
    const uint32_t wave = ( blockIdx.x * blockDim.x + threadIdx.x ) >> 6, lane = threadIdx.x & 63u;
    if ( wave >= nwaves )
	return;						// (whole waves)
    const uint32_t K = (uint32_t)__builtin_amdgcn_readfirstlane((int)Ks[wave]);
    const float4 st = state[wave];
    const float track_amplitude = st.x, peak_confidence = st.y, confidence_total = st.z, amplitude_total = st.w;
    const bool have = lane < K;
    const float cv = have ? cv_in[64u * wave + lane] : 0.0f;
    const float av = have ? av_in[64u * wave + lane] : 0.0f;
    constexpr bool soft = R != 0;
    float xt = ( track_amplitude + av ) / 2.0f;
    float xpk = peak_confidence < cv ? cv : peak_confidence;
    if ( soft && cv < peak_confidence * 0.75f )
	xpk = cv;
    float xsc = confidence_total + cv;
    float xsa = amplitude_total + av;
    float my_t = track_amplitude, my_pk = peak_confidence;
    float my_sc = confidence_total, my_sa = amplitude_total;
    if constexpr ( R == 2 )
	replay_scan_track(xt, xsc, xsa, my_t, my_sc, my_sa, cv, av, K, totals);
    else if constexpr ( R == 1 )
	replay_scan_soft(xt, xpk, xsc, xsa, my_t, my_pk, my_sc, my_sa, cv, av, K, lane, totals);
    else
	replay_scan_asm(xt, xpk, xsc, xsa, my_t, my_pk, my_sc, my_sa, cv, av, K, totals);
    x_out[64u * wave + lane] = make_float4(xt, xpk, xsc, xsa);
    b_out[64u * wave + lane] = make_float4(my_t, my_pk, my_sc, my_sa);
}

// out[w] = wave_max_f32 over v[64 w .. 64 w + 63]
__global__ __launch_bounds__(256)
void selftest_wave_max_kernel( const float *__restrict__ v, uint32_t nwaves, float *__restrict__ out )
{
    const uint32_t wave = ( blockIdx.x * blockDim.x + threadIdx.x ) >> 6, lane = threadIdx.x & 63u;
    if ( wave >= nwaves )
	return;
    const float m = wave_max_f32(v[64u * wave + lane]);
    if ( lane == 0 )
	out[wave] = m;
}

namespace {

// device memory for the length of one call
struct TestBuf : DevMem<uint8_t> {
    bool make( size_t bytes ) { return alloc(bytes, 1) == 0; }
    bool put( const void *h, size_t bytes ) { return hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess; }
    bool get( void *h, size_t bytes ) const { return hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

constexpr uint64_t kMaxValues = 1ull << 30;		// (blocks of 256 in 32 bits, arrays the host can hold)

inline int finish()
{
    if ( hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess )
	return -EIO;
    return 0;
}

} // namespace
} // namespace mifsk

using mifsk::TestBuf;

extern "C" int mifsk_selftest_rcp( mifsk_ctx *ctx, const float *c, const float *x, uint64_t n,
	double *rcp_out, float *quot_out )
{
    if ( !ctx || !c || !x || !rcp_out || !quot_out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    TestBuf d_c, d_x, d_rc, d_q;
    if ( !d_c.make(n * sizeof(float)) || !d_x.make(n * sizeof(float))
	    || !d_rc.make(n * sizeof(double)) || !d_q.make(n * sizeof(float)) )
	return -ENOMEM;
    if ( !d_c.put(c, n * sizeof(float)) || !d_x.put(x, n * sizeof(float)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_rcp_kernel, dim3((unsigned)( ( n + 255u ) / 256u )), dim3(256), 0, nullptr,
	    (const float *)d_c.p, (const float *)d_x.p, n, (double *)d_rc.p, (float *)d_q.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_rc.get(rcp_out, n * sizeof(double)) && d_q.get(quot_out, n * sizeof(float)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_gauss( mifsk_ctx *ctx, const uint32_t *words, uint64_t n, double *z_out )
{
    if ( !ctx || !words || !z_out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    TestBuf d_w, d_z;
    if ( !d_w.make(n * sizeof(uint2)) || !d_z.make(n * sizeof(double2)) )
	return -ENOMEM;
    if ( !d_w.put(words, n * sizeof(uint2)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_gauss_kernel, dim3((unsigned)( ( n + 255u ) / 256u )), dim3(256), 0, nullptr,
	    (const uint2 *)d_w.p, n, (double2 *)d_z.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_z.get(z_out, n * sizeof(double2)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_turn( mifsk_ctx *ctx, const double *y, const double *x, uint64_t n, double *out )
{
    if ( !ctx || !y || !x || !out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    TestBuf d_y, d_x, d_t;
    if ( !d_y.make(n * sizeof(double)) || !d_x.make(n * sizeof(double)) || !d_t.make(n * sizeof(double)) )
	return -ENOMEM;
    if ( !d_y.put(y, n * sizeof(double)) || !d_x.put(x, n * sizeof(double)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_turn_kernel, dim3((unsigned)( ( n + 255u ) / 256u )), dim3(256), 0, nullptr,
	    (const double *)d_y.p, (const double *)d_x.p, n, (double *)d_t.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_t.get(out, n * sizeof(double)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_mag( mifsk_ctx *ctx, const double *re, const double *im, float scalar, uint64_t n,
	double *sqrt_out, double *g_out, uint8_t *unsafe_out, float *mag_out )
{
    if ( !ctx || !re || !im || !sqrt_out || !g_out || !unsafe_out || !mag_out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    TestBuf d_re, d_im, d_root, d_g, d_u, d_mag;
    if ( !d_re.make(n * sizeof(double)) || !d_im.make(n * sizeof(double)) || !d_root.make(n * sizeof(double))
	    || !d_g.make(n * sizeof(double)) || !d_u.make(n) || !d_mag.make(n * sizeof(float)) )
	return -ENOMEM;
    if ( !d_re.put(re, n * sizeof(double)) || !d_im.put(im, n * sizeof(double)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_mag_kernel, dim3((unsigned)( ( n + 255u ) / 256u )), dim3(256), 0, nullptr,
	    (const double *)d_re.p, (const double *)d_im.p, scalar, n, (double *)d_root.p, (double *)d_g.p,
	    (uint8_t *)d_u.p, (float *)d_mag.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_root.get(sqrt_out, n * sizeof(double)) && d_g.get(g_out, n * sizeof(double))
	    && d_u.get(unsafe_out, n) && d_mag.get(mag_out, n * sizeof(float)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_confidence( mifsk_ctx *ctx, int variant, uint32_t n_bits, uint64_t req_mask,
	uint64_t req_val, const float *mags, uint64_t ncases, float *conf_out, float *ampl_out,
	uint64_t *bits_out, uint32_t *fell_back_out )
{
    if ( !ctx || !mags || !conf_out || !ampl_out || !bits_out || !fell_back_out
	    || variant < 0 || variant > 2 || n_bits == 0 || n_bits > MIFSK_MAX_FRAME_BITS
	    || ncases > mifsk::kMaxValues / MIFSK_MAX_FRAME_BITS )
	return -EINVAL;
    if ( ncases == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    const size_t mag_bytes = (size_t)ncases * n_bits * 2 * sizeof(float);
    TestBuf d_m, d_conf, d_ampl, d_bits, d_fb;
    if ( !d_m.make(mag_bytes) || !d_conf.make(ncases * sizeof(float)) || !d_ampl.make(ncases * sizeof(float))
	    || !d_bits.make(ncases * sizeof(uint64_t)) || !d_fb.make(ncases * sizeof(uint32_t)) )
	return -ENOMEM;
    if ( !d_m.put(mags, mag_bytes) )
	return -EIO;
    const dim3 grid((unsigned)( ( ncases + 255u ) / 256u )), block(256);	// (256: whole waves of 64)
#define MIFSK_SELFTEST_CONF(V)										\
    hipLaunchKernelGGL(mifsk::selftest_confidence_kernel<V>, grid, block, 0, nullptr,			\
	    (const float2 *)d_m.p, ncases, n_bits, req_mask, req_val, (float *)d_conf.p, (float *)d_ampl.p,	\
	    (unsigned long long *)d_bits.p, (uint32_t *)d_fb.p)
    if ( variant == 0 )
	MIFSK_SELFTEST_CONF(0);
    else if ( variant == 1 )
	MIFSK_SELFTEST_CONF(1);
    else
	MIFSK_SELFTEST_CONF(2);
#undef MIFSK_SELFTEST_CONF
    if ( int rc = mifsk::finish() )
	return rc;
    return d_conf.get(conf_out, ncases * sizeof(float)) && d_ampl.get(ampl_out, ncases * sizeof(float))
	    && d_bits.get(bits_out, ncases * sizeof(uint64_t)) && d_fb.get(fell_back_out, ncases * sizeof(uint32_t))
	    ? 0 : -EIO;
}

namespace mifsk {
namespace {

constexpr uint32_t kCorrMaxSamples = 1u << 24;
constexpr uint32_t kCorrMaxLdsFloats = 12288u;		// 48 KiB of the 64 a workgroup may have
constexpr uint32_t kCorrMaxCases = 1u << 16;

template <int R, int NQ>
void launch_corr( const CorrArgs &A, uint32_t nwaves )
{
    hipLaunchKernelGGL(( selftest_corr_kernel<R, NQ> ), dim3(nwaves), dim3(64), (size_t)A.lds_floats * sizeof(float),
	    nullptr, A);
}

template <int R>
bool launch_corr_fixed( const CorrArgs &A, uint32_t nwaves, uint32_t nq )
{
    switch ( nq ) {
#define MIFSK_NQ(Q) case Q: launch_corr<R, Q>(A, nwaves); return true
    case 1:
	if constexpr ( R == MIFSK_SELFTEST_CORR_LDS_FIXED ) {
	    launch_corr<R, 1>(A, nwaves);
	    return true;
	}
	return false;
    MIFSK_NQ(2); MIFSK_NQ(3); MIFSK_NQ(4); MIFSK_NQ(5); MIFSK_NQ(6); MIFSK_NQ(7);
    MIFSK_NQ(8); MIFSK_NQ(9); MIFSK_NQ(10); MIFSK_NQ(11); MIFSK_NQ(12);
#undef MIFSK_NQ
    }
    return false;
}

} // namespace
} // namespace mifsk

extern "C" int mifsk_selftest_corr( mifsk_ctx *ctx, const mifsk_rx_config *cfg, int routine, int param,
	const float *samples, uint32_t nsamples, const uint32_t *starts, const uint32_t *lens,
	uint32_t ncases, double *acc_out, float *esum_out )
{
    using namespace mifsk;
    const bool seg = routine == MIFSK_SELFTEST_CORR_SEG_GROUP;
    if ( !ctx || mifsk_check_cfg(cfg) || !samples || !starts || !acc_out
	    || routine < MIFSK_SELFTEST_CORR_LDS_FIXED || routine > MIFSK_SELFTEST_CORR_SEG_GROUP
	    || ( seg && ( !lens || !esum_out ) )
	    || nsamples == 0 || nsamples > kCorrMaxSamples || ncases > kCorrMaxCases
	    || param < 0 || param > 1
	    || ( param != 0 && !seg && routine != MIFSK_SELFTEST_CORR_SKEWED_STREAM ) )
	return -EINVAL;
    if ( ncases == 0 )
	return 0;
    // every routine's precondition, case by case: nothing is launched that would read outside
    // the samples or outside its LDS
    const uint64_t B = cfg->bit_nsamples, N = nsamples;
    const bool in_lds = routine <= MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN || routine == MIFSK_SELFTEST_CORR_SLAB_PLAIN
		     || routine == MIFSK_SELFTEST_CORR_SKEWED_STREAM;
    const bool aligned = routine <= MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN;	// 16-byte aligned LDS windows of whole float4s
    if ( B >= 65536u || ( in_lds && N > kCorrMaxLdsFloats ) || ( aligned && ( B % 4u != 0 || B == 0 ) ) )
	return -EINVAL;
    uint64_t reach = B;								// samples a routine loads from a window's start on
    if ( routine == MIFSK_SELFTEST_CORR_LDS_STREAM || routine == MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN
	    || routine == MIFSK_SELFTEST_CORR_GLOBAL_STREAM )
	reach = 16u * ( ( B + 15u ) / 16u );					// whole groups
    else if ( routine == MIFSK_SELFTEST_CORR_GLOBAL_TILED )
	reach = TILE_K * ( ( B + TILE_K - 1u ) / TILE_K );			// whole tile steps
    uint32_t lo = 0xFFFFFFFFu;
    for ( uint32_t i = 0; i < ncases; i++ ) {
	const uint64_t a = starts[i];
	if ( aligned && a % 4u != 0 )
	    return -EINVAL;
	if ( seg ) {
	    if ( lens[i] == 0 || lens[i] > B || a + lens[i] > N )
		return -EINVAL;
	} else if ( a + reach > N ) {
	    return -EINVAL;
	}
	lo = starts[i] < lo ? starts[i] : lo;
    }
    const uint32_t nq = (uint32_t)( B / 4u );
    if ( ( routine == MIFSK_SELFTEST_CORR_LDS_FIXED && ( nq < 1 || nq > 12 ) )
	    || ( routine == MIFSK_SELFTEST_CORR_LDS_FIXED_HALVES && ( nq < 2 || nq > 12 ) ) )
	return -EINVAL;

    // the tables the receive entry points would launch with for this configuration
    std::shared_lock<std::shared_mutex> gate;
    DevCfg d;
    const double *d_tw = nullptr;
    if ( int rc = lookup_tables(ctx, cfg, gate, d, &d_tw) )
	return rc;
    if ( routine == MIFSK_SELFTEST_CORR_SKEWED_STREAM )
	d.skew = (uint32_t)param;

    CorrArgs A = {};
    const size_t padded = ( (size_t)nsamples + 3u ) & ~(size_t)3u;
    std::vector<float> hx(padded, 0.0f);
    for ( uint32_t i = 0; i < nsamples; i++ )
	hx[i] = samples[i];
    TestBuf d_cfg, d_x, d_starts, d_lens, d_acc, d_esum;
    if ( !d_cfg.make(sizeof(DevCfg)) || !d_x.make(padded * sizeof(float)) || !d_starts.make(ncases * sizeof(uint32_t))
	    || !d_lens.make(ncases * sizeof(uint32_t)) || !d_acc.make((size_t)ncases * 4 * sizeof(double))
	    || !d_esum.make(ncases * sizeof(float)) )
	return -ENOMEM;
    if ( !d_cfg.put(&d, sizeof(DevCfg)) || !d_x.put(hx.data(), padded * sizeof(float))
	    || !d_starts.put(starts, ncases * sizeof(uint32_t)) || ( seg && !d_lens.put(lens, ncases * sizeof(uint32_t)) ) )
	return -EIO;
    A.cfg = (const DevCfg *)d_cfg.p;
    A.tw = d_tw;
    A.x = (const float *)d_x.p;
    A.N = nsamples;
    A.starts = (const uint32_t *)d_starts.p;
    A.lens = (const uint32_t *)d_lens.p;
    A.ncases = ncases;
    A.lo = lo;
    A.never_whole = seg ? (uint32_t)param : 0u;
    A.acc = (double *)d_acc.p;
    A.esum = (float *)d_esum.p;
    if ( routine == MIFSK_SELFTEST_CORR_GLOBAL_TILED ) {
	A.lds_floats = TILE_FLOATS;
    } else if ( routine == MIFSK_SELFTEST_CORR_SKEWED_STREAM ) {
	// rows of B samples with `skew` pad words in between, from sample lo on
	const uint64_t cap = N - lo;
	const uint64_t words = cap + ( cap / B + 2u ) * d.skew + 4u;
	if ( words > kCorrMaxLdsFloats + 8192u / sizeof(float) )
	    return -EINVAL;
	A.lds_floats = (uint32_t)( ( words + 3u ) & ~(uint64_t)3u );
    } else if ( in_lds ) {
	A.lds_floats = (uint32_t)padded;
    } else {
	A.lds_floats = 4u;
    }
    const uint32_t nwaves = ( ncases + 63u ) / 64u;
    bool launched = true;
    switch ( routine ) {
    case MIFSK_SELFTEST_CORR_LDS_FIXED:
	launched = launch_corr_fixed<MIFSK_SELFTEST_CORR_LDS_FIXED>(A, nwaves, nq);
	break;
    case MIFSK_SELFTEST_CORR_LDS_FIXED_HALVES:
	launched = launch_corr_fixed<MIFSK_SELFTEST_CORR_LDS_FIXED_HALVES>(A, nwaves, nq);
	break;
    case MIFSK_SELFTEST_CORR_LDS_STREAM:	launch_corr<MIFSK_SELFTEST_CORR_LDS_STREAM, 0>(A, nwaves); break;
    case MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN:	launch_corr<MIFSK_SELFTEST_CORR_LDS_STREAM_LEAN, 0>(A, nwaves); break;
    case MIFSK_SELFTEST_CORR_GLOBAL_STREAM:	launch_corr<MIFSK_SELFTEST_CORR_GLOBAL_STREAM, 0>(A, nwaves); break;
    case MIFSK_SELFTEST_CORR_GLOBAL_TILED:	launch_corr<MIFSK_SELFTEST_CORR_GLOBAL_TILED, 0>(A, nwaves); break;
    case MIFSK_SELFTEST_CORR_SLAB_PLAIN:	launch_corr<MIFSK_SELFTEST_CORR_SLAB_PLAIN, 0>(A, nwaves); break;
    case MIFSK_SELFTEST_CORR_SKEWED_STREAM:	launch_corr<MIFSK_SELFTEST_CORR_SKEWED_STREAM, 0>(A, nwaves); break;
    default:					launch_corr<MIFSK_SELFTEST_CORR_SEG_GROUP, 0>(A, nwaves); break;
    }
    if ( !launched )
	return -EINVAL;
    if ( int rc = finish() )
	return rc;
    if ( !d_acc.get(acc_out, (size_t)ncases * 4 * sizeof(double)) || ( seg && !d_esum.get(esum_out, ncases * sizeof(float)) ) )
	return -EIO;
    return 0;
}

extern "C" int mifsk_selftest_scan( mifsk_ctx *ctx, int routine, int totals, const float *state, const float *cv,
	const float *av, const uint32_t *k, uint32_t nwaves, float *x_out, float *b_out )
{
    if ( !ctx || !state || !cv || !av || !k || !x_out || !b_out || routine < 0 || routine > 2
	    || totals < 0 || totals > 1 || nwaves > ( 1u << 20 ) )
	return -EINVAL;
    for ( uint32_t w = 0; w < nwaves; w++ )
	if ( k[w] < 1u || k[w] > 64u )
	    return -EINVAL;
    if ( nwaves == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    const size_t lanes = (size_t)nwaves * 64u;
    TestBuf d_st, d_cv, d_av, d_k, d_x, d_b;
    if ( !d_st.make(nwaves * 4 * sizeof(float)) || !d_cv.make(lanes * sizeof(float)) || !d_av.make(lanes * sizeof(float))
	    || !d_k.make(nwaves * sizeof(uint32_t)) || !d_x.make(lanes * 4 * sizeof(float)) || !d_b.make(lanes * 4 * sizeof(float)) )
	return -ENOMEM;
    if ( !d_st.put(state, nwaves * 4 * sizeof(float)) || !d_cv.put(cv, lanes * sizeof(float))
	    || !d_av.put(av, lanes * sizeof(float)) || !d_k.put(k, nwaves * sizeof(uint32_t)) )
	return -EIO;
    const dim3 grid(( nwaves + 3u ) / 4u), block(256);
#define MIFSK_SELFTEST_SCAN(R)										\
    hipLaunchKernelGGL(mifsk::selftest_scan_kernel<R>, grid, block, 0, nullptr, (const float4 *)d_st.p,	\
	    (const float *)d_cv.p, (const float *)d_av.p, (const uint32_t *)d_k.p, nwaves, totals != 0,		\
	    (float4 *)d_x.p, (float4 *)d_b.p)
    if ( routine == 0 )
	MIFSK_SELFTEST_SCAN(0);
    else if ( routine == 1 )
	MIFSK_SELFTEST_SCAN(1);
    else
	MIFSK_SELFTEST_SCAN(2);
#undef MIFSK_SELFTEST_SCAN
    if ( int rc = mifsk::finish() )
	return rc;
    return d_x.get(x_out, lanes * 4 * sizeof(float)) && d_b.get(b_out, lanes * 4 * sizeof(float)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_wave_max( mifsk_ctx *ctx, const float *v, uint32_t nwaves, float *max_out )
{
    if ( !ctx || !v || !max_out || nwaves > ( 1u << 20 ) )
	return -EINVAL;
    if ( nwaves == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    TestBuf d_v, d_m;
    if ( !d_v.make((size_t)nwaves * 64u * sizeof(float)) || !d_m.make(nwaves * sizeof(float)) )
	return -ENOMEM;
    if ( !d_v.put(v, (size_t)nwaves * 64u * sizeof(float)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_wave_max_kernel, dim3(( nwaves + 3u ) / 4u), dim3(256), 0, nullptr,
	    (const float *)d_v.p, nwaves, (float *)d_m.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_m.get(max_out, nwaves * sizeof(float)) ? 0 : -EIO;
}
