// Micro-benchmark (gfx950): the rate of the FP64 vector FMA (v_fma_f64) with nothing else in the
// way -- 16 independent accumulator chains per lane, operands in registers, no memory traffic in
// the loop.  The guides give no figure for it; the carrier survey (csrc/mifsk_carrier.hip) is
// measured against this one (tools/bench_carrier.py runs it and reads the JSON line).
// Waves per SIMD 1, 2 and 4; every CU busy.  Reports FMA/s per chip and CU cycles per
// wave-instruction at the clock the run held (s_memtime against the 100 MHz constant clock).
//   hipcc --offload-arch=gfx950 -O3 -o fma64_rate fma64_rate.hip && ./fma64_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e = (x); if ( e != hipSuccess ) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kChains = 16;

__global__ __launch_bounds__(256) void k( int iters, double a, double b, double *out, unsigned long long *clocks )
{
    double acc[kChains];
#pragma unroll
    for ( int j = 0; j < kChains; j++ )
	acc[j] = (double)( threadIdx.x + j );
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for ( int i = 0; i < iters; i++ ) {
#pragma unroll
	for ( int u = 0; u < 4; u++ )
#pragma unroll
	    for ( int j = 0; j < kChains; j++ )
		acc[j] = __builtin_fma(acc[j], a, b);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double s = 0.0;
#pragma unroll
    for ( int j = 0; j < kChains; j++ )
	s += acc[j];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ( threadIdx.x == 0 ) {
	clocks[2 * blockIdx.x] = t1 - t0;
	clocks[2 * blockIdx.x + 1] = r1 - r0;
    }
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int ncu = prop.multiProcessorCount;
    const int iters = 1 << 15;
    double *out;
    unsigned long long *clocks;
    const int max_blocks = ncu * 4;
    CK(hipMalloc(&out, (size_t)max_blocks * 256 * sizeof(double)));
    CK(hipMalloc(&clocks, (size_t)max_blocks * 2 * sizeof(unsigned long long)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    double best = 0.0;
    printf("%s, %d CUs\n", prop.gcnArchName, ncu);
    for ( int per_simd = 1; per_simd <= 4; per_simd *= 2 ) {
	const int blocks = ncu * per_simd;			// 256 threads: one wave on each SIMD
	for ( int w = 0; w < 3; w++ )				// warm-up
	    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, iters, 0.999999, 1e-9, out, clocks);
	CK(hipDeviceSynchronize());
	std::vector<double> ms;
	for ( int r = 0; r < 7; r++ ) {
	    CK(hipEventRecord(e0));
	    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, iters, 0.999999, 1e-9, out, clocks);
	    CK(hipEventRecord(e1));
	    CK(hipEventSynchronize(e1));
	    float t;
	    CK(hipEventElapsedTime(&t, e0, e1));
	    ms.push_back(t);
	}
	std::sort(ms.begin(), ms.end());
	std::vector<unsigned long long> h(2 * (size_t)blocks);
	CK(hipMemcpy(h.data(), clocks, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
	std::vector<double> mhz;
	for ( int i = 0; i < blocks; i++ )
	    mhz.push_back(h[2 * i + 1] ? (double)h[2 * i] / (double)h[2 * i + 1] * 100.0 : 0.0);
	std::sort(mhz.begin(), mhz.end());
	const double fma = (double)blocks * 256.0 * iters * 4.0 * kChains;
	const double rate = fma / ( ms[3] * 1e-3 );
	const double wave_instr_per_simd = (double)per_simd * iters * 4.0 * kChains;
	const double cyc = ms[3] * 1e-3 * mhz[mhz.size() / 2] * 1e6 / wave_instr_per_simd;
	printf("%d wave(s) per SIMD: %.3f ms (min %.3f max %.3f)  %.2f TFMA/s  clock %.0f MHz  %.2f cycles per wave-instruction per SIMD\n",
	       per_simd, ms[3], ms[0], ms[6], rate * 1e-12, mhz[mhz.size() / 2], cyc);
	best = std::max(best, rate);
    }
    printf("{\"fma64_per_s\": %.6e, \"compute_units\": %d}\n", best, ncu);
    return 0;
}
