// mifsk_legacy.cpp -- the reference's five-function API (include/fsk.h) over the same kernels as
// the batch entry points: a plan owns a context and the few device buffers one call at a time needs.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <shared_mutex>
#include <vector>

#include "fsk.h"
#include "mifsk.h"
#include "mifsk_ctx.h"
#include "mifsk_hostmem.h"

namespace {

struct LegacyPlan {
    mifsk_ctx				*ctx = nullptr;
    mifsk::DevMem<float>		d_samples, d_mags;
    mifsk::DevMem<mifsk_search>		d_problem;
    mifsk::DevMem<mifsk_search_result>	d_result;
};

} // namespace

extern "C" fsk_plan *fsk_plan_new( float sample_rate, float f_mark, float f_space,
	float filter_bw )
{
    fsk_plan *p = (fsk_plan *)std::calloc(1, sizeof(fsk_plan));
    if ( !p ) {
	errno = ENOMEM;
	return nullptr;
    }
    p->sample_rate = sample_rate;
    p->f_mark = f_mark;
    p->f_space = f_space;
    p->band_width = filter_bw;
    const float half = p->band_width / 2.0f;			// fsk.c:52-57
    p->fftsize = (int)( (sample_rate + half) / p->band_width );
    p->nbands = (unsigned)( p->fftsize / 2 + 1 );
    p->b_mark = (unsigned)( (f_mark + half) / p->band_width );
    p->b_space = (unsigned)( (f_space + half) / p->band_width );
    if ( p->b_mark >= p->nbands || p->b_space >= p->nbands ) {	// fsk.c:58-64
	fprintf(stderr, "b_mark=%u or b_space=%u is invalid (nbands=%u)\n",
		p->b_mark, p->b_space, p->nbands);
	std::free(p);
	errno = EINVAL;
	return nullptr;
    }
    LegacyPlan *lp = new (std::nothrow) LegacyPlan();
    if ( !lp ) {
	std::free(p);
	errno = ENOMEM;
	return nullptr;
    }
    int rc = mifsk_ctx_create(&lp->ctx, -1);
    if ( rc == 0 && ( lp->d_problem.fit(1) || lp->d_result.fit(1) ) )
	rc = -ENOMEM;
    if ( rc ) {
	if ( lp->ctx ) mifsk_ctx_destroy(lp->ctx);
	delete lp;
	std::free(p);
	errno = -rc;
	return nullptr;
    }
    p->fftplan = lp;
    p->fftin = nullptr;
    p->fftout = nullptr;
    return p;
}

extern "C" void fsk_plan_destroy( fsk_plan *p )
{
    if ( !p )
	return;
    LegacyPlan *lp = (LegacyPlan *)p->fftplan;
    if ( lp ) {
	mifsk_ctx *ctx = lp->ctx;
	delete lp;			// (its buffers free themselves)
	mifsk_ctx_destroy(ctx);
    }
    std::free(p);
}

extern "C" float fsk_find_frame( fsk_plan *p, float *samples, unsigned int frame_nsamples,
	unsigned int try_first_sample, unsigned int try_max_nsamples,
	unsigned int try_step_nsamples, float try_confidence_search_limit,
	const char *expect_bits_string, unsigned long long *bits_outp,
	float *ampl_outp, unsigned int *frame_start_outp )
{
    *bits_outp = 0;
    *ampl_outp = 0.0f;
    *frame_start_outp = 0;
    LegacyPlan *lp = p ? (LegacyPlan *)p->fftplan : nullptr;
    const size_t n_bits = expect_bits_string ? std::strlen(expect_bits_string) : 0;
    if ( !lp || n_bits == 0 || n_bits > MIFSK_MAX_FRAME_BITS	// assert in fsk.c:463
	    || (int)try_first_sample >= (int)try_max_nsamples || try_step_nsamples == 0 )
	return 0.0f;

    // the slice of the configuration that fsk_find_frame itself derives
    // (fsk.c:465,183,204); everything else in DevCfg is unused by this kernel
    mifsk_rx_config c;
    std::memset(&c, 0, sizeof(c));
    c.expect_n_bits = (unsigned)n_bits;
    const float spb = (float)frame_nsamples / (float)(int)n_bits;
    c.find_samples_per_bit = spb;
    c.bit_nsamples = (unsigned)( spb + 0.5f );
    if ( c.bit_nsamples == 0 )
	return 0.0f;
    for ( unsigned k = 0; k < n_bits; k++ ) {
	c.bit_offset[k] = (unsigned)( spb * (float)(int)k + 0.5f );
	c.expect_data[k] = expect_bits_string[k];
	c.expect_sync[k] = expect_bits_string[k];
    }
    c.fftsize = p->fftsize;
    c.b_mark = p->b_mark;
    c.b_space = p->b_space;

    // what the reference can touch (fsk.c:204-206,477-484): the highest candidate
    // it may try, first + k * step < try_max, plus the last bit window -- not
    // try_max - 1: a caller whose buffer ends at the reference's true extent
    // must not be over-read
    const unsigned up_steps = ( try_max_nsamples - try_first_sample - 1u ) / try_step_nsamples;
    const size_t t_last = (size_t)try_first_sample + (size_t)up_steps * try_step_nsamples;
    const size_t reach = t_last + c.bit_offset[n_bits - 1] + c.bit_nsamples;
    if ( hipSetDevice(mifsk::ctx_device(lp->ctx)) != hipSuccess || lp->d_samples.fit(reach) )
	return 0.0f;
    mifsk_search pr;
    pr.sample_offset = 0;
    pr.navail = (uint32_t)reach;
    pr.try_first = try_first_sample;
    pr.try_max = try_max_nsamples;
    pr.try_step = try_step_nsamples;
    pr.search_limit = try_confidence_search_limit;
    pr.use_sync_string = 0;
    mifsk_search_result res;
    if ( hipMemcpy(lp->d_samples.p, samples, reach * sizeof(float), hipMemcpyHostToDevice) != hipSuccess
	    || hipMemcpy(lp->d_problem.p, &pr, sizeof(pr), hipMemcpyHostToDevice) != hipSuccess )
	return 0.0f;
    if ( mifsk_find_frame_batch(lp->ctx, &c, lp->d_samples.p, lp->d_problem.p, lp->d_result.p, 1, nullptr) )
	return 0.0f;
    if ( hipMemcpy(&res, lp->d_result.p, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess )
	return 0.0f;
    *bits_outp = res.bits;
    *ampl_outp = res.amplitude;
    *frame_start_outp = res.frame_start;
    return res.confidence;
}

extern "C" int fsk_detect_carrier( fsk_plan *p, float *samples, unsigned int nsamples,
	float min_mag_threshold )
{
    LegacyPlan *lp = p ? (LegacyPlan *)p->fftplan : nullptr;
    if ( !lp || nsamples == 0 || nsamples > (unsigned)p->fftsize )	// assert in fsk.c:547
	return -1;
    mifsk_ctx *ctx = lp->ctx;
    const unsigned N = (unsigned)p->fftsize;
    std::shared_lock<std::shared_mutex> gate;			// lookup .. enqueue
    if ( mifsk::enter(ctx, gate) )
	return -1;
    const double *d_cs = nullptr;
    if ( mifsk::get_cs(ctx, N, &d_cs) )
	return -1;
    if ( lp->d_samples.fit(nsamples) || lp->d_mags.fit(p->nbands) )
	return -1;
    if ( hipMemcpy(lp->d_samples.p, samples, nsamples * sizeof(float), hipMemcpyHostToDevice) != hipSuccess )
	return -1;
    if ( mifsk::launch_detect_carrier(lp->d_samples.p, nsamples, d_cs, N, p->nbands,
				      lp->d_mags.p, nullptr) )
	return -1;
    std::vector<float> mags(p->nbands);
    if ( hipMemcpy(mags.data(), lp->d_mags.p, p->nbands * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess )
	return -1;
    // peak pick over the device-computed magnitudes (fsk.c:554-580)
    float max_mag = 0.0f;
    int max_band = -1;
    for ( unsigned i = 1; i < p->nbands; i++ ) {
	const float mag = mags[i];
	if ( mag < min_mag_threshold )
	    continue;
	if ( max_mag < mag ) {
	    max_mag = mag;
	    max_band = (int)i;
	}
    }
    return max_band;
}

extern "C" void fsk_set_tones_by_bandshift( fsk_plan *p, unsigned int b_mark, int b_shift )
{
    if ( !p || b_shift == 0 || b_mark >= p->nbands )		// asserts in fsk.c:587-592
	return;
    const int b_space = (int)b_mark + b_shift;
    if ( b_space < 0 || b_space >= (int)p->nbands )
	return;
    p->b_mark = b_mark;
    p->b_space = (unsigned)b_space;
    p->f_mark = b_mark * p->band_width;
    p->f_space = b_space * p->band_width;
}
