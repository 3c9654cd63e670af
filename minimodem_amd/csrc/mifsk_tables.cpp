// mifsk_tables.cpp -- the contents of the context's device tables (mifsk_tables.h).
#include "mifsk_tables.h"

#include <cmath>

#include "mifsk_device.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace mifsk {

// cos, -sin of an angle as the oracle's tables hold them (ofsk_twiddle, and the spectrum table
// of ofsk_detect_carrier): its cos(ang) and -sin(ang) are compiled into ONE sincos() call, and the
// C library's sincos() is not its sin(): at 2 pi 198 / 240, for one, the two sines differ in the
// last place.  Separate calls made three entries of the Bell-202 table differ from the oracle's by
// an ulp -- invisible once a sum is rounded to float, but not "the oracle's sums"
// (tests/test_gpu_correlators.py compares the doubles).
static inline void cos_msin( double ang, double w[2] )
{
    double s, c;
    ::sincos(ang, &s, &c);
    w[0] = c;
    w[1] = -s;
}

// exp(-2 pi i b n / N): the angle is reduced exactly in integers first
static inline void twiddle( unsigned b, unsigned n, unsigned fftsize, double w[2] )
{
    const unsigned long long k = ( (unsigned long long)b * n ) % fftsize;
    cos_msin(2.0 * M_PI * (double)k / (double)fftsize, w);
}

std::vector<double> bit_table( const TwKey &key )
{
    const size_t n = tw_entries(key.bit_nsamples);
    std::vector<double> h(4 * ( n ? n : 8 ), 0.0);
    for ( unsigned i = 0; i < key.bit_nsamples; i++ ) {
	twiddle(key.b_mark, i, key.fftsize, &h[4 * (size_t)i]);
	twiddle(key.b_space, i, key.fftsize, &h[4 * (size_t)i + 2]);
    }
    return h;
}

std::vector<double> spectrum_table( unsigned N )
{
    std::vector<double> h(2 * (size_t)N);
    for ( unsigned k = 0; k < N; k++ )
	cos_msin(2.0 * M_PI * (double)k / (double)N, &h[2 * (size_t)k]);
    return h;
}

std::vector<double> rotation_table( const DevCfg &d, int kind, uint32_t &stride )
{
    stride = 0;
    const SegPlan &sp = d.seg[kind];
    if ( !sp.valid )
	return {};
    unsigned cmax = 0;
    for ( unsigned w = 0; w < sp.nwin; w++ )
	cmax = sp.win_count[w] > cmax ? sp.win_count[w] : cmax;
    stride = ( sp.nwin + 63u ) & ~63u;
    // (zero rows beyond the longest window's: Wave::seg_correlate walks the rows with a running
    // pointer, four segments a turn, and where two lanes share a window -- every other row each --
    // up to 2 x 3 + 1 rows beyond the last)
    std::vector<double> h((size_t)( ( cmax + 12u + 3u ) & ~3u ) * stride * 4, 0.0);
    for ( unsigned w = 0; w < sp.nwin; w++ )
	for ( unsigned i = 0; i < sp.win_count[w]; i++ ) {
	    const unsigned off = sp.seg_rel[sp.win_first[w] + i] - ( sp.p_win[w] >> 16 );
	    double *t = &h[( (size_t)i * stride + w ) * 4];
	    twiddle(d.b_mark, off, d.fftsize, t);
	    twiddle(d.b_space, off, d.fftsize, t + 2);
	}
    return h;
}

} // namespace mifsk
