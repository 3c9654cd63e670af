// mifsk_selftest.hip -- the device arithmetic of mifsk_devlib.h / mifsk_devmath.h, one value or
// one frame per thread, for the host to compare with an independent reference
// (mifsk_selftest_rcp / _mag / _confidence in include/mifsk.h; tests/test_gpu_devmath.py).
//
// The kernels CALL the routines the receive loops call and restate nothing; a translation unit
// of their own, so that no receive kernel's code depends on what is here.  What this pins is the
// routines' arithmetic as the compiler inlines it into these kernels, not how it schedules them
// inside a receive loop (every parity test compares that with the oracle, on real audio).
// gfx950 only.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_devlib.h"

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

namespace {

// device memory for the length of one call
struct DevBuf {
    void	*p = nullptr;
    DevBuf() {}
    DevBuf( const DevBuf & ) = delete;
    ~DevBuf() { if ( p ) (void)hipFree(p); }
    bool alloc( size_t bytes ) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
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

using mifsk::DevBuf;

extern "C" int mifsk_selftest_rcp( mifsk_ctx *ctx, const float *c, const float *x, uint64_t n,
	double *rcp_out, float *quot_out )
{
    if ( !ctx || !c || !x || !rcp_out || !quot_out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    DevBuf d_c, d_x, d_rc, d_q;
    if ( !d_c.alloc(n * sizeof(float)) || !d_x.alloc(n * sizeof(float))
	    || !d_rc.alloc(n * sizeof(double)) || !d_q.alloc(n * sizeof(float)) )
	return -ENOMEM;
    if ( !d_c.put(c, n * sizeof(float)) || !d_x.put(x, n * sizeof(float)) )
	return -EIO;
    hipLaunchKernelGGL(mifsk::selftest_rcp_kernel, dim3((unsigned)( ( n + 255u ) / 256u )), dim3(256), 0, nullptr,
	    (const float *)d_c.p, (const float *)d_x.p, n, (double *)d_rc.p, (float *)d_q.p);
    if ( int rc = mifsk::finish() )
	return rc;
    return d_rc.get(rcp_out, n * sizeof(double)) && d_q.get(quot_out, n * sizeof(float)) ? 0 : -EIO;
}

extern "C" int mifsk_selftest_mag( mifsk_ctx *ctx, const double *re, const double *im, float scalar, uint64_t n,
	double *sqrt_out, double *g_out, uint8_t *unsafe_out, float *mag_out )
{
    if ( !ctx || !re || !im || !sqrt_out || !g_out || !unsafe_out || !mag_out || n > mifsk::kMaxValues )
	return -EINVAL;
    if ( n == 0 )
	return 0;
    HIP_OK(hipSetDevice(ctx->device));
    DevBuf d_re, d_im, d_root, d_g, d_u, d_mag;
    if ( !d_re.alloc(n * sizeof(double)) || !d_im.alloc(n * sizeof(double)) || !d_root.alloc(n * sizeof(double))
	    || !d_g.alloc(n * sizeof(double)) || !d_u.alloc(n) || !d_mag.alloc(n * sizeof(float)) )
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
    DevBuf d_m, d_conf, d_ampl, d_bits, d_fb;
    if ( !d_m.alloc(mag_bytes) || !d_conf.alloc(ncases * sizeof(float)) || !d_ampl.alloc(ncases * sizeof(float))
	    || !d_bits.alloc(ncases * sizeof(uint64_t)) || !d_fb.alloc(ncases * sizeof(uint32_t)) )
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
