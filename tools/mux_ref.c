/* mux_ref.c -- the multiplexer's definition (include/mifsk.h) restated for the host
 * as plain nested loops with explicit fma(), sincos() and lrintf(): the yardstick of
 * tests/test_mux_args.py and tests/test_gpu_mux.py, which compile it into a temporary shared
 * object with -O2 -ffp-contract=off.  Never linked into libmifsk.so: the library has no host
 * multiplexer.  mux_ref_iq at the end is the same for the I/Q entry (include/mifsk/mux_iq.h, DESIGN.md
 * 4.19; tests/test_mux_iq_args.py and tests/test_gpu_mux_iq.py).  mux_ref_stream and mux_ref_stream_iq behind
 * it restate one feed of a multiplexer stream (include/mifsk/mux_stream.h, DESIGN.md 4.21;
 * tests/test_mux_stream_args.py and tests/test_gpu_mux_stream.py).
 *
 *   cc -O2 -ffp-contract=off -shared -fPIC -o mux_ref.so tools/mux_ref.c -lm
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>

#define MUX_REF_COMPLEX 1
#define MUX_REF_S16     2

static const double two_pi = 6.283185307179586476925286766559;

static int64_t reduce( int64_t q, int64_t P )
{
    q %= P;
    return q < 0 ? q + P : q;
}

/* G: g[t][0] = h[t] cos, g[t][1] = h[t] sin of 2 pi ((r t) mod P) / P */
void mux_ref_table( uint32_t P, uint32_t T, const float *h, int32_t r, double *g )
{
    const int64_t rr = reduce(r, P);
    for ( uint32_t t = 0; t < T; t++ ) {
	const int64_t idx = ( rr * (int64_t)t ) % (int64_t)P;
	double s, c;
	sincos(two_pi * (double)idx / (double)P, &s, &c);
	g[2 * t] = (double)h[t] * c;
	g[2 * t + 1] = (double)h[t] * s;
    }
}

/* the PCM16 write conversion of oracle/shim/sndfile_shim.c; a NaN gives 0 */
int16_t mux_ref_s16( float v )
{
    float t = v * 32767.0f;
    if ( t > 32767.0f ) t = 32767.0f;
    if ( t < -32768.0f ) t = -32768.0f;
    if ( t != t )
	return 0;
    return (int16_t)lrintf(t);
}

/* One stream: K rows x[k * stride ..] of valid lengths min(len[k], stride); out is out_stride
 * elements of the kind (float or int16_t, one or two scalars each), g a scratch of [T][2] doubles.
 * Returns the count min(M, nout_cap); out[n] is written for every n < out_stride, zero from the
 * count on. */
uint64_t mux_ref( const float *x, uint64_t stride, const uint32_t *len, int kind, uint32_t P, uint32_t T,
	const float *h, uint32_t L, uint32_t K, const int32_t *q, int32_t r, const float *gains,
	void *out, uint64_t out_stride, uint64_t nout_cap, double *g )
{
    const int cx = kind & MUX_REF_COMPLEX, s16 = kind & MUX_REF_S16;
    const int64_t rr = reduce(r, P);
    uint64_t nmax = 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	const uint64_t n = len[k] < stride ? len[k] : stride;
	if ( n > nmax )
	    nmax = n;
    }
    uint64_t M = nmax ? ( nmax - 1 ) * L + T : 0;
    if ( M > nout_cap )
	M = nout_cap;
    mux_ref_table(P, T, h, r, g);
    for ( uint64_t n = 0; n < out_stride; n++ ) {
	double o = 0.0, oi = 0.0;
	for ( uint32_t k = 0; k < K && n < M; k++ ) {
	    const int64_t nk = len[k] < stride ? len[k] : stride;
	    const int64_t m = n / L;
	    const uint64_t phi = n % L;
	    double re = 0.0, im = 0.0;
	    for ( uint64_t j = 0; phi + j * L < T; j++ ) {
		const uint64_t t = phi + j * L;
		const int64_t i = m - (int64_t)j;
		if ( i >= 0 && i < nk ) {
		    const double v = (double)x[(uint64_t)k * stride + i];
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    if ( gains ) {
		re = re * (double)gains[k];
		im = im * (double)gains[k];
	    }
	    const int64_t dq = reduce(reduce(q[k], P) - rr, P);
	    const int64_t p = ( dq * (int64_t)( n % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    o = fma(re, C, o);
	    o = fma(-im, S, o);
	    if ( cx ) {
		oi = fma(re, S, oi);
		oi = fma(im, C, oi);
	    }
	}
	const float vr = n < M ? (float)o : 0.0f, vi = n < M ? (float)oi : 0.0f;
	if ( s16 ) {
	    int16_t *o16 = (int16_t *)out;
	    if ( cx ) {
		o16[2 * n] = n < M ? mux_ref_s16(vr) : 0;
		o16[2 * n + 1] = n < M ? mux_ref_s16(vi) : 0;
	    } else
		o16[n] = n < M ? mux_ref_s16(vr) : 0;
	} else {
	    float *of = (float *)out;
	    if ( cx ) {
		of[2 * n] = vr;
		of[2 * n + 1] = vi;
	    } else
		of[n] = vr;
	}
    }
    return M;
}

/* mux_ref with I/Q rows in (include/mifsk/mux_iq.h): x is [K][stride][2] floats, len
 * and stride count (I, Q) elements.  The tap step is the product of the complex sample and the
 * complex table entry, four fma()s; everything else is mux_ref's, written out again. */
uint64_t mux_ref_iq( const float *x, uint64_t stride, const uint32_t *len, int kind, uint32_t P, uint32_t T,
	const float *h, uint32_t L, uint32_t K, const int32_t *q, int32_t r, const float *gains,
	void *out, uint64_t out_stride, uint64_t nout_cap, double *g )
{
    const int cx = kind & MUX_REF_COMPLEX, s16 = kind & MUX_REF_S16;
    const int64_t rr = reduce(r, P);
    uint64_t nmax = 0;
    for ( uint32_t k = 0; k < K; k++ ) {
	const uint64_t n = len[k] < stride ? len[k] : stride;
	if ( n > nmax )
	    nmax = n;
    }
    uint64_t M = nmax ? ( nmax - 1 ) * L + T : 0;
    if ( M > nout_cap )
	M = nout_cap;
    mux_ref_table(P, T, h, r, g);
    for ( uint64_t n = 0; n < out_stride; n++ ) {
	double o = 0.0, oi = 0.0;
	for ( uint32_t k = 0; k < K && n < M; k++ ) {
	    const int64_t nk = len[k] < stride ? len[k] : stride;
	    const int64_t m = n / L;
	    const uint64_t phi = n % L;
	    double re = 0.0, im = 0.0;
	    for ( uint64_t j = 0; phi + j * L < T; j++ ) {
		const uint64_t t = phi + j * L;
		const int64_t i = m - (int64_t)j;
		if ( i >= 0 && i < nk ) {
		    const double a = (double)x[2 * ( (uint64_t)k * stride + i )];
		    const double b = (double)x[2 * ( (uint64_t)k * stride + i ) + 1];
		    re = fma(a, g[2 * t], re);
		    re = fma(-b, g[2 * t + 1], re);
		    im = fma(a, g[2 * t + 1], im);
		    im = fma(b, g[2 * t], im);
		}
	    }
	    if ( gains ) {
		re = re * (double)gains[k];
		im = im * (double)gains[k];
	    }
	    const int64_t dq = reduce(reduce(q[k], P) - rr, P);
	    const int64_t p = ( dq * (int64_t)( n % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    o = fma(re, C, o);
	    o = fma(-im, S, o);
	    if ( cx ) {
		oi = fma(re, S, oi);
		oi = fma(im, C, oi);
	    }
	}
	const float vr = n < M ? (float)o : 0.0f, vi = n < M ? (float)oi : 0.0f;
	if ( s16 ) {
	    int16_t *o16 = (int16_t *)out;
	    if ( cx ) {
		o16[2 * n] = n < M ? mux_ref_s16(vr) : 0;
		o16[2 * n + 1] = n < M ? mux_ref_s16(vi) : 0;
	    } else
		o16[n] = n < M ? mux_ref_s16(vr) : 0;
	} else {
	    float *of = (float *)out;
	    if ( cx ) {
		of[2 * n] = vr;
		of[2 * n + 1] = vi;
	    } else
		of[n] = vr;
	}
    }
    return M;
}

/* One feed of one stream of a multiplexer stream (include/mifsk/mux_stream.h): mux_ref's loops over a
 * buffer [tail | piece] per row.  x is [K][stride] floats, row k's element H + i the stream's sample
 * seen + i: H = ceil(T / L) - 1 tail elements (what they hold in front of `first` does not matter),
 * then the piece, continued with +0.0 up to ks by the caller (stride >= H + ks).  `seen`: the samples
 * the stream has taken, so the feed's first output is the absolute output seen * L; `first`: the
 * absolute sample index in front of which samples do not exist: such a term is skipped.  out is
 * out_stride elements of the kind, g a scratch of [T][2] doubles.  Returns the count ks * L (at most
 * out_stride, the caller sees to it); out[n] is written for every n < out_stride, zero from the count on. */
uint64_t mux_ref_stream( const float *x, uint64_t stride, uint32_t H, uint64_t ks, uint64_t seen, uint64_t first,
	int kind, uint32_t P, uint32_t T, const float *h, uint32_t L, uint32_t K, const int32_t *q, int32_t r,
	const float *gains, void *out, uint64_t out_stride, double *g )
{
    const int cx = kind & MUX_REF_COMPLEX, s16 = kind & MUX_REF_S16;
    const int64_t rr = reduce(r, P);
    const uint64_t M = ks * L;
    mux_ref_table(P, T, h, r, g);
    for ( uint64_t nl = 0; nl < out_stride; nl++ ) {
	const uint64_t n = seen * L + nl;			/* the absolute output */
	double o = 0.0, oi = 0.0;
	for ( uint32_t k = 0; k < K && nl < M; k++ ) {
	    const int64_t m = (int64_t)( n / L );
	    const uint64_t phi = n % L;
	    double re = 0.0, im = 0.0;
	    for ( uint64_t j = 0; phi + j * L < T; j++ ) {
		const uint64_t t = phi + j * L;
		const int64_t i = m - (int64_t)j;		/* the absolute sample: j <= H */
		if ( i >= (int64_t)first ) {
		    const uint64_t at = (uint64_t)( (int64_t)H + i - (int64_t)seen );
		    const double v = (double)x[(uint64_t)k * stride + at];
		    re = fma(v, g[2 * t], re);
		    im = fma(v, g[2 * t + 1], im);
		}
	    }
	    if ( gains ) {
		re = re * (double)gains[k];
		im = im * (double)gains[k];
	    }
	    const int64_t dq = reduce(reduce(q[k], P) - rr, P);
	    const int64_t p = ( dq * (int64_t)( n % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    o = fma(re, C, o);
	    o = fma(-im, S, o);
	    if ( cx ) {
		oi = fma(re, S, oi);
		oi = fma(im, C, oi);
	    }
	}
	const float vr = nl < M ? (float)o : 0.0f, vi = nl < M ? (float)oi : 0.0f;
	if ( s16 ) {
	    int16_t *o16 = (int16_t *)out;
	    if ( cx ) {
		o16[2 * nl] = nl < M ? mux_ref_s16(vr) : 0;
		o16[2 * nl + 1] = nl < M ? mux_ref_s16(vi) : 0;
	    } else
		o16[nl] = nl < M ? mux_ref_s16(vr) : 0;
	} else {
	    float *of = (float *)out;
	    if ( cx ) {
		of[2 * nl] = vr;
		of[2 * nl + 1] = vi;
	    } else
		of[nl] = vr;
	}
    }
    return M;
}

/* mux_ref_stream with I/Q rows in, as mux_ref_iq is mux_ref's: x is [K][stride][2] floats, stride, H and
 * ks count (I, Q) elements. */
uint64_t mux_ref_stream_iq( const float *x, uint64_t stride, uint32_t H, uint64_t ks, uint64_t seen, uint64_t first,
	int kind, uint32_t P, uint32_t T, const float *h, uint32_t L, uint32_t K, const int32_t *q, int32_t r,
	const float *gains, void *out, uint64_t out_stride, double *g )
{
    const int cx = kind & MUX_REF_COMPLEX, s16 = kind & MUX_REF_S16;
    const int64_t rr = reduce(r, P);
    const uint64_t M = ks * L;
    mux_ref_table(P, T, h, r, g);
    for ( uint64_t nl = 0; nl < out_stride; nl++ ) {
	const uint64_t n = seen * L + nl;			/* the absolute output */
	double o = 0.0, oi = 0.0;
	for ( uint32_t k = 0; k < K && nl < M; k++ ) {
	    const int64_t m = (int64_t)( n / L );
	    const uint64_t phi = n % L;
	    double re = 0.0, im = 0.0;
	    for ( uint64_t j = 0; phi + j * L < T; j++ ) {
		const uint64_t t = phi + j * L;
		const int64_t i = m - (int64_t)j;		/* the absolute sample: j <= H */
		if ( i >= (int64_t)first ) {
		    const uint64_t at = (uint64_t)( (int64_t)H + i - (int64_t)seen );
		    const double a = (double)x[2 * ( (uint64_t)k * stride + at )];
		    const double b = (double)x[2 * ( (uint64_t)k * stride + at ) + 1];
		    re = fma(a, g[2 * t], re);
		    re = fma(-b, g[2 * t + 1], re);
		    im = fma(a, g[2 * t + 1], im);
		    im = fma(b, g[2 * t], im);
		}
	    }
	    if ( gains ) {
		re = re * (double)gains[k];
		im = im * (double)gains[k];
	    }
	    const int64_t dq = reduce(reduce(q[k], P) - rr, P);
	    const int64_t p = ( dq * (int64_t)( n % P ) ) % (int64_t)P;
	    double S, C;
	    sincos(two_pi * (double)p / (double)P, &S, &C);
	    o = fma(re, C, o);
	    o = fma(-im, S, o);
	    if ( cx ) {
		oi = fma(re, S, oi);
		oi = fma(im, C, oi);
	    }
	}
	const float vr = nl < M ? (float)o : 0.0f, vi = nl < M ? (float)oi : 0.0f;
	if ( s16 ) {
	    int16_t *o16 = (int16_t *)out;
	    if ( cx ) {
		o16[2 * nl] = nl < M ? mux_ref_s16(vr) : 0;
		o16[2 * nl + 1] = nl < M ? mux_ref_s16(vi) : 0;
	    } else
		o16[nl] = nl < M ? mux_ref_s16(vr) : 0;
	} else {
	    float *of = (float *)out;
	    if ( cx ) {
		of[2 * nl] = vr;
		of[2 * nl + 1] = vi;
	    } else
		of[nl] = vr;
	}
    }
    return M;
}
