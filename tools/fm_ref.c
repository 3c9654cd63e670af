/* fm_ref.c -- the FM stage's definition (include/mifsk.h: mifsk_fm_demod_batch,
 * mifsk_fm_modulate_batch) restated for the host from the header comment, as plain
 * serial loops with explicit fma(), rint() and lrintf(): the angle in turns, the discriminator's
 * element, the modulator's integer phase, both kinds and the rows' tails.  It includes NEITHER
 * minimodem_amd/csrc/mifsk_angle.h NOR mifsk_gauss.h: it is the yardstick those headers and the
 * device kernels are compared with (tests/_fm.py compiles it into a temporary shared object with
 * -O2 -ffp-contract=off; tests/test_fm_ref.py, tests/test_gpu_fm.py).  Never linked into
 * libmifsk.so.
 *
 *   cc -O2 -ffp-contract=off -shared -fPIC -o fm_ref.so tools/fm_ref.c -lm
 */
#include <math.h>
#include <stdint.h>

#define FM_REF_S16 1			/* MIFSK_FEED_S16 */

/* the argument of x + i y in turns */
double fm_ref_turn( double y, double x )
{
    const double ax = fabs(x), ay = fabs(y);
    const int sw = ay > ax;
    double mx, mn, a;
    if ( sw ) {
	mx = ay;
	mn = ax;
    } else {
	mx = ax;
	mn = ay;
    }
    if ( mx == 0.0 ) {
	a = 0.0;
    } else {
	const double edge = mx * 0x1.a827999fcef32p-2;
	const int big = mn > edge;
	double u;
	if ( big ) {
	    const double num = mn - mx, den = mn + mx;
	    u = num / den;
	} else {
	    u = mn / mx;
	}
	const double v = u * u;
	double p = -1.0 / 23.0;
	for ( int k = 10; k >= 0; k-- )
	    p = fma(p, v, ( k % 2 ? -1.0 : 1.0 ) / (double)( 2 * k + 1 ));
	const double r = u * p;
	a = fma(r, 0x1.45f306dc9c883p-3, big ? 0.125 : 0.0);
    }
    if ( sw )
	a = 0.25 - a;
    if ( x < 0.0 )
	a = 0.5 - a;
    if ( y < 0.0 )
	a = -a;
    return a;
}

/* out[i] = turn(y[i], x[i]) */
void fm_ref_turns( const double *y, const double *x, uint64_t n, double *out )
{
    for ( uint64_t i = 0; i < n; i++ )
	out[i] = fm_ref_turn(y[i], x[i]);
}

/* scalar j (0: I, 1: Q) of element i of a row, as a float */
static float scalar_at( const void *row, uint32_t kind, uint64_t i, int j )
{
    if ( kind == FM_REF_S16 )
	return (float)( (const int16_t *)row )[2 * i + j] / 32768.0f;
    return ( (const float *)row )[2 * i + j];
}

/* The discriminator on host arrays: x is nstreams rows of interleaved I, Q of `kind`, stream_stride
 * complex elements apart; len (NULL: all = nsamples) the rows' lengths; out nstreams rows of
 * out_stride floats; prev (or NULL) and last (or NULL) [nstreams][2] floats.  Every element of out
 * is written: zero from W_s on. */
void fm_ref_demod_rows( const void *x, uint64_t stream_stride, const uint32_t *len, uint32_t nsamples, int nstreams,
	uint32_t kind, float *out, uint64_t out_stride, const float *prev, float *last, float gain )
{
    const uint64_t scalar_bytes = kind == FM_REF_S16 ? 2 : 4;
    for ( int s = 0; s < nstreams; s++ ) {
	uint64_t W = len ? len[s] : nsamples;
	if ( W > stream_stride )
	    W = stream_stride;
	if ( W > out_stride )
	    W = out_stride;
	const void *row = (const char *)x + (uint64_t)s * stream_stride * 2 * scalar_bytes;
	float pi = prev ? prev[2 * s] : 0.0f, pq = prev ? prev[2 * s + 1] : 0.0f;
	for ( uint64_t n = 0; n < out_stride; n++ ) {
	    float o = 0.0f;
	    if ( n < W ) {
		const float fi = scalar_at(row, kind, n, 0), fq = scalar_at(row, kind, n, 1);
		const double a = (double)fi, b = (double)fq, c = (double)pi, d = (double)pq;
		const double bd = b * d, ad = a * d;
		const double re = fma(a, c, bd);
		const double im = fma(b, c, -ad);
		o = (float)( (double)gain * fm_ref_turn(im, re) );
		pi = fi;
		pq = fq;
	    }
	    out[(uint64_t)s * out_stride + n] = o;
	}
	if ( last ) {
	    last[2 * s] = pi;
	    last[2 * s + 1] = pq;
	}
    }
}

static double factorial( int n )			/* exact in double up to 20! (and beyond) */
{
    double f = 1.0;
    for ( int i = 2; i <= n; i++ )
	f = f * (double)i;
    return f;
}

/* cs[0] = C(w), cs[1] = S(w): cos, sin of 2 pi w / 2^32, the channel model's */
void fm_ref_cs( uint32_t w, double *cs_out )
{
    const uint32_t q = w >> 29, fr = w & 0x1FFFFFFFu;
    const uint32_t a = ( q % 2 == 0 ) ? fr : 0x20000000u - fr;
    const double phi = 0x1.921fb54442d18p-1 * ( (double)a * 0x1p-29 );
    const double y = phi * phi;
    double ps = -1.0 / factorial(19);
    for ( int k = 8; k >= 0; k-- )
	ps = fma(ps, y, ( k % 2 ? -1.0 : 1.0 ) / factorial(2 * k + 1));
    const double sn = phi * ps;
    double pc = 1.0 / factorial(20);
    for ( int k = 9; k >= 0; k-- )
	pc = fma(pc, y, ( k % 2 ? -1.0 : 1.0 ) / factorial(2 * k));
    const double cs = pc;
    double C, S;
    switch ( q ) {
    case 0: C = cs; S = sn; break;
    case 1: C = sn; S = cs; break;
    case 2: C = -sn; S = cs; break;
    case 3: C = -cs; S = sn; break;
    case 4: C = -cs; S = -sn; break;
    case 5: C = -sn; S = -cs; break;
    case 6: C = sn; S = -cs; break;
    default: C = cs; S = -sn; break;
    }
    cs_out[0] = C;
    cs_out[1] = S;
}

/* the PCM16 write conversion (mux_ref.c's): a NaN gives 0 */
static int16_t to_s16( float v )
{
    float t = v * 32767.0f;
    if ( t > 32767.0f ) t = 32767.0f;
    if ( t < -32768.0f ) t = -32768.0f;
    if ( t != t )
	return 0;
    return (int16_t)lrintf(t);
}

/* the phase step of one sample */
uint64_t fm_ref_step( float x, double deviation, double centre )
{
    const double d = fma((double)x, deviation, centre);
    if ( !( fabs(d) < 16384.0 ) )
	return 0;
    return (uint64_t)(int64_t)rint(d * 0x1p48);
}

/* The modulator on host arrays: x is nstreams rows of floats, stream_stride apart; out nstreams rows
 * of interleaved I, Q of out_kind, out_stride complex elements apart; phase0 (or NULL) and phase_out
 * (or NULL) [nstreams].  Every element of out is written: zero from W_s on. */
void fm_ref_mod_rows( const float *x, uint64_t stream_stride, const uint32_t *len, uint32_t nsamples, int nstreams,
	uint32_t out_kind, void *out, uint64_t out_stride, double deviation, double centre, const uint64_t *phase0,
	uint64_t *phase_out, float amplitude )
{
    const double A = (double)amplitude;
    for ( int s = 0; s < nstreams; s++ ) {
	uint64_t W = len ? len[s] : nsamples;
	if ( W > stream_stride )
	    W = stream_stride;
	if ( W > out_stride )
	    W = out_stride;
	uint64_t phase = phase0 ? phase0[s] : 0;
	for ( uint64_t i = 0; i < out_stride; i++ ) {
	    float oi = 0.0f, oq = 0.0f;
	    if ( i < W ) {
		double cs[2];
		phase += fm_ref_step(x[(uint64_t)s * stream_stride + i], deviation, centre);
		fm_ref_cs((uint32_t)( phase >> 16 ), cs);
		oi = (float)( A * cs[0] );
		oq = (float)( A * cs[1] );
	    }
	    const uint64_t e = 2 * ( (uint64_t)s * out_stride + i );
	    if ( out_kind == FM_REF_S16 ) {
		( (int16_t *)out )[e] = i < W ? to_s16(oi) : 0;
		( (int16_t *)out )[e + 1] = i < W ? to_s16(oq) : 0;
	    } else {
		( (float *)out )[e] = oi;
		( (float *)out )[e + 1] = oq;
	    }
	}
	if ( phase_out )
	    phase_out[s] = phase;
    }
}
