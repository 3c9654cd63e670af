/* channel_ref.c -- the channelizer's definition (include/mifsk.h) restated for the
 * host as three nested loops with explicit fma() and sincos(): the yardstick of
 * tests/test_channel_args.py and tests/test_gpu_channel.py, which compile it into a temporary
 * shared object with -O2 -ffp-contract=off.  Never linked into libmifsk.so: the library has no
 * host channelizer.  channel_ref_iq restates the I/Q entry (include/mifsk/channel_iq.h) the same
 * way, for tests/test_channel_iq_args.py and tests/test_gpu_channel_iq.py; channel_ref_stream and
 * channel_ref_stream_iq restate one feed of a channel stream (include/mifsk/channel_stream.h), for
 * tests/test_channel_stream_args.py and tests/test_gpu_channel_stream.py.
 *
 *   cc -O2 -ffp-contract=off -shared -fPIC -o channel_ref.so tools/channel_ref.c -lm
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>

#define CHANNEL_REF_COMPLEX 1
#define CHANNEL_REF_S16     2

static const double two_pi = 6.283185307179586476925286766559;

static int64_t reduce( int64_t q, int64_t P )
{
    q %= P;
    return q < 0 ? q + P : q;
}

/* G of one channel: g[t][0] = h[t] cos, g[t][1] = -(h[t] sin) of 2 pi ((q t) mod P) / P */
void channel_ref_table( uint32_t P, uint32_t T, const float *h, int32_t q, double *g )
{
    const int64_t qq = reduce(q, P);
    for ( uint32_t t = 0; t < T; t++ ) {
	const int64_t idx = ( qq * (int64_t)t ) % (int64_t)P;
	double s, c;
	sincos(two_pi * (double)idx / (double)P, &s, &c);
	g[2 * t] = (double)h[t] * c;
	g[2 * t + 1] = -( (double)h[t] * s );
    }
}

static double scalar( const void *x, int s16, uint64_t i )
{
    if ( s16 )
	return (double)( (float)( (const int16_t *)x )[i] / 32768.0f );
    return (double)( (const float *)x )[i];
}

/* Every output of K channels of one row of N elements; out is [K][out_stride], g a scratch of
 * [T][2] doubles.  Returns the number of outputs that exist, M; out[k][m] is written for
 * m < min(M, out_stride), nothing else is touched. */
uint64_t channel_ref( const void *x, uint64_t N, int kind, uint32_t P, uint32_t T, const float *h,
	uint32_t D, uint32_t K, const int32_t *q, int32_t r, float *out, uint64_t out_stride, double *g )
{
    const int cx = kind & CHANNEL_REF_COMPLEX, s16 = kind & CHANNEL_REF_S16;
    const uint64_t M = N >= T ? ( N - T ) / D + 1 : 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_ref_table(P, T, h, q[k], g);
	const int64_t dq = reduce((int64_t)r - reduce(q[k], P), P);
	for ( uint64_t m = 0; m < M && m < out_stride; m++ ) {
	    double re = 0.0, im = 0.0;
	    for ( uint32_t t = 0; t < T; t++ ) {
		const uint64_t n = m * D + t;
		if ( cx ) {
		    const double xr = scalar(x, s16, 2 * n), xi = scalar(x, s16, 2 * n + 1);
		    re = fma(xr, g[2 * t], re);
		    re = fma(-xi, g[2 * t + 1], re);
		    im = fma(xr, g[2 * t + 1], im);
		    im = fma(xi, g[2 * t], im);
		} else {
		    const double v = scalar(x, s16, n);
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    const int64_t p = ( dq * (int64_t)( ( m * D ) % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    out[(uint64_t)k * out_stride + m] = (float)fma(re, C, -( im * S ));
	}
    }
    return M;
}

/* The I/Q entry's definition (include/mifsk/channel_iq.h), written out again from it: the same sums,
 * then both halves of the rotation.  out is [K][out_stride][2]: (I, Q) of output m of channel k at
 * out[(k * out_stride + m) * 2]; otherwise as channel_ref. */
uint64_t channel_ref_iq( const void *x, uint64_t N, int kind, uint32_t P, uint32_t T, const float *h,
	uint32_t D, uint32_t K, const int32_t *q, int32_t r, float *out, uint64_t out_stride, double *g )
{
    const int cx = kind & CHANNEL_REF_COMPLEX, s16 = kind & CHANNEL_REF_S16;
    const uint64_t M = N >= T ? ( N - T ) / D + 1 : 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_ref_table(P, T, h, q[k], g);
	const int64_t dq = reduce((int64_t)r - reduce(q[k], P), P);
	for ( uint64_t m = 0; m < M && m < out_stride; m++ ) {
	    double re = 0.0, im = 0.0;
	    for ( uint32_t t = 0; t < T; t++ ) {
		const uint64_t n = m * D + t;
		if ( cx ) {
		    const double xr = scalar(x, s16, 2 * n), xi = scalar(x, s16, 2 * n + 1);
		    re = fma(xr, g[2 * t], re);
		    re = fma(-xi, g[2 * t + 1], re);
		    im = fma(xr, g[2 * t + 1], im);
		    im = fma(xi, g[2 * t], im);
		} else {
		    const double v = scalar(x, s16, n);
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    const int64_t p = ( dq * (int64_t)( ( m * D ) % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    const double neg = -( im * S ), pos = im * C;
	    float *o = out + ( (uint64_t)k * out_stride + m ) * 2;
	    o[0] = (float)fma(re, C, neg);
	    o[1] = (float)fma(re, S, pos);
	}
    }
    return M;
}

/* The channel stream's definition (include/mifsk/channel_stream.h): the outputs of ONE feed.  x holds
 * the stream's elements from index first_output * D on, N of them: what the stream kept and the new
 * piece.  Output ml < Mloc = (N >= T ? (N - T) / D + 1 : 0) is output m = first_output + ml of the
 * capture: the same three loops as channel_ref over x, and p from the absolute m, each factor reduced
 * mod P first (m D passes 2^64 long after m does not).  out is [K][out_stride], out[k][ml] written for
 * ml < min(Mloc, out_stride); returns Mloc.  A host that keeps x[Mloc * D ..] for the next call and
 * adds Mloc to first_output is the host model of the whole object. */
uint64_t channel_ref_stream( const void *x, uint64_t N, uint64_t first_output, int kind, uint32_t P, uint32_t T,
	const float *h, uint32_t D, uint32_t K, const int32_t *q, int32_t r, float *out, uint64_t out_stride, double *g )
{
    const int cx = kind & CHANNEL_REF_COMPLEX, s16 = kind & CHANNEL_REF_S16;
    const uint64_t M = N >= T ? ( N - T ) / D + 1 : 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_ref_table(P, T, h, q[k], g);
	const int64_t dq = reduce((int64_t)r - reduce(q[k], P), P);
	for ( uint64_t ml = 0; ml < M && ml < out_stride; ml++ ) {
	    double re = 0.0, im = 0.0;
	    for ( uint32_t t = 0; t < T; t++ ) {
		const uint64_t n = ml * D + t;
		if ( cx ) {
		    const double xr = scalar(x, s16, 2 * n), xi = scalar(x, s16, 2 * n + 1);
		    re = fma(xr, g[2 * t], re);
		    re = fma(-xi, g[2 * t + 1], re);
		    im = fma(xr, g[2 * t + 1], im);
		    im = fma(xi, g[2 * t], im);
		} else {
		    const double v = scalar(x, s16, n);
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    const uint64_t m = first_output + ml;
	    const int64_t p = ( dq * (int64_t)( ( ( m % P ) * ( D % P ) ) % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    out[(uint64_t)k * out_stride + ml] = (float)fma(re, C, -( im * S ));
	}
    }
    return M;
}

/* ... with MIFSK_CHANNEL_STREAM_IQ: both halves of the rotation, as channel_ref_iq keeps them.  out is
 * [K][out_stride][2]. */
uint64_t channel_ref_stream_iq( const void *x, uint64_t N, uint64_t first_output, int kind, uint32_t P, uint32_t T,
	const float *h, uint32_t D, uint32_t K, const int32_t *q, int32_t r, float *out, uint64_t out_stride, double *g )
{
    const int cx = kind & CHANNEL_REF_COMPLEX, s16 = kind & CHANNEL_REF_S16;
    const uint64_t M = N >= T ? ( N - T ) / D + 1 : 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	channel_ref_table(P, T, h, q[k], g);
	const int64_t dq = reduce((int64_t)r - reduce(q[k], P), P);
	for ( uint64_t ml = 0; ml < M && ml < out_stride; ml++ ) {
	    double re = 0.0, im = 0.0;
	    for ( uint32_t t = 0; t < T; t++ ) {
		const uint64_t n = ml * D + t;
		if ( cx ) {
		    const double xr = scalar(x, s16, 2 * n), xi = scalar(x, s16, 2 * n + 1);
		    re = fma(xr, g[2 * t], re);
		    re = fma(-xi, g[2 * t + 1], re);
		    im = fma(xr, g[2 * t + 1], im);
		    im = fma(xi, g[2 * t], im);
		} else {
		    const double v = scalar(x, s16, n);
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    const uint64_t m = first_output + ml;
	    const int64_t p = ( dq * (int64_t)( ( ( m % P ) * ( D % P ) ) % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    const double neg = -( im * S ), pos = im * C;
	    float *o = out + ( (uint64_t)k * out_stride + ml ) * 2;
	    o[0] = (float)fma(re, C, neg);
	    o[1] = (float)fma(re, S, pos);
	}
    }
    return M;
}
