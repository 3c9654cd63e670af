/* impair_ref.c -- the channel model's definition (include/mifsk.h: mifsk_impair_batch, DESIGN.md
 * 4.16) restated for the host from the header comment, as plain loops with explicit fma(), sqrt()
 * and lrintf(): Philox4x32-10, the Box-Muller transform from exact operations, the element, both
 * kinds each way and the rows' tails.  It does NOT include minimodem_amd/csrc/mifsk_gauss.h: it
 * is the yardstick that header and the device kernel are compared with (tests/_impair.py compiles
 * it into a temporary shared object with -O2 -ffp-contract=off; tests/test_impair_ref.py,
 * tests/test_gpu_impair.py).  Never linked into libmifsk.so.
 *
 *   cc -O2 -ffp-contract=off -shared -fPIC -o impair_ref.so tools/impair_ref.c -lm
 */
#include <math.h>
#include <stdint.h>

#define IMPAIR_REF_S16 1		/* MIFSK_FEED_S16 */

/* ten rounds on counter ctr[4] under key[2] -> out[4] */
void impair_ref_philox( const uint32_t *ctr, const uint32_t *key, uint32_t *out )
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for ( int r = 0; r < 10; r++ ) {
	const uint64_t p0 = 0xD2511F53ull * c0;
	const uint64_t p1 = 0xCD9E8D57ull * c2;
	const uint32_t hi0 = (uint32_t)( p0 >> 32 ), lo0 = (uint32_t)( p0 & 0xFFFFFFFFull );
	const uint32_t hi1 = (uint32_t)( p1 >> 32 ), lo1 = (uint32_t)( p1 & 0xFFFFFFFFull );
	const uint32_t a = hi1 ^ c1 ^ k0, b = lo1, c = hi0 ^ c3 ^ k1, d = lo0;
	c0 = a;
	c1 = b;
	c2 = c;
	c3 = d;
	k0 += 0x9E3779B9u;
	k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

/* R(w) = sqrt(-2 ln((w + 1) / 2^32)) */
double impair_ref_r( uint32_t w )
{
    const uint64_t t = (uint64_t)w + 1;
    int e = 0;
    while ( ( t >> ( e + 1 ) ) != 0 )
	e++;						/* floor(log2 t) */
    double m = ldexp((double)t, -e);			/* exact, in [1, 2) */
    if ( m > 0x1.6a09e667f3bcdp+0 ) {
	m = m * 0.5;
	e = e + 1;
    }
    const double f = m - 1.0;
    const double s = f / ( 2.0 + f );
    const double y = s * s;
    double p = 1.0 / 23.0;
    for ( int k = 10; k >= 0; k-- )
	p = fma(p, y, 1.0 / (double)( 2 * k + 1 ));
    const double lnm = ( 2.0 * s ) * p;
    const double ln = fma((double)( e - 32 ), 0x1.62e42fefa39efp-1, lnm);
    return sqrt(-2.0 * ln);
}

static double factorial( int n )			/* exact in double up to 20! (and beyond) */
{
    double f = 1.0;
    for ( int i = 2; i <= n; i++ )
	f = f * (double)i;
    return f;
}

/* cs[0] = C(w), cs[1] = S(w): cos, sin of 2 pi w / 2^32 */
void impair_ref_cs( uint32_t w, double *cs_out )
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

/* z[0] = R(wr) C(wa), z[1] = R(wr) S(wa) */
void impair_ref_pair( uint32_t wr, uint32_t wa, double *z )
{
    double cs[2];
    const double r = impair_ref_r(wr);
    impair_ref_cs(wa, cs);
    z[0] = r * cs[0];
    z[1] = r * cs[1];
}

/* n pairs of words [n][2] -> rcs[n][3] = R(w[0]), C(w[1]), S(w[1]) and z[n][2]; either may be NULL */
void impair_ref_words( const uint32_t *words, uint64_t n, double *rcs, double *z )
{
    for ( uint64_t i = 0; i < n; i++ ) {
	if ( rcs ) {
	    rcs[3 * i] = impair_ref_r(words[2 * i]);
	    impair_ref_cs(words[2 * i + 1], rcs + 3 * i + 1);
	}
	if ( z )
	    impair_ref_pair(words[2 * i], words[2 * i + 1], z + 2 * i);
    }
}

/* z(seed, S, n) */
double impair_ref_z( uint64_t seed, uint64_t S, uint64_t n )
{
    const uint64_t j = n >> 2;
    const uint32_t ctr[4] = { (uint32_t)j, (uint32_t)( j >> 32 ), (uint32_t)S, (uint32_t)( S >> 32 ) };
    const uint32_t key[2] = { (uint32_t)seed, (uint32_t)( seed >> 32 ) };
    uint32_t w[4];
    double z[2];
    impair_ref_philox(ctr, key, w);
    if ( ( n & 3 ) < 2 )
	impair_ref_pair(w[0], w[1], z);
    else
	impair_ref_pair(w[2], w[3], z);
    return z[n & 1];
}

/* out[i] = z(seed, S, n0 + i), i < count; n0 % 4 == 0 */
void impair_ref_field( uint64_t seed, uint64_t S, uint64_t n0, uint64_t count, double *out )
{
    const uint32_t key[2] = { (uint32_t)seed, (uint32_t)( seed >> 32 ) };
    for ( uint64_t i = 0; i < count; i += 4 ) {
	const uint64_t j = ( n0 + i ) >> 2;
	const uint32_t ctr[4] = { (uint32_t)j, (uint32_t)( j >> 32 ), (uint32_t)S, (uint32_t)( S >> 32 ) };
	uint32_t w[4];
	double z[4];
	impair_ref_philox(ctr, key, w);
	impair_ref_pair(w[0], w[1], z);
	impair_ref_pair(w[2], w[3], z + 2);
	for ( uint64_t u = 0; u < 4 && i + u < count; u++ )
	    out[i + u] = z[u];
    }
}

/* the PCM16 write conversion (mux_ref.c's): a NaN gives 0 */
int16_t impair_ref_s16( float v )
{
    float t = v * 32767.0f;
    if ( t > 32767.0f ) t = 32767.0f;
    if ( t < -32768.0f ) t = -32768.0f;
    if ( t != t )
	return 0;
    return (int16_t)lrintf(t);
}

/* The whole entry on host arrays: x (NULL: noise rows) is nstreams rows of `kind` stream_stride
 * elements apart, len (NULL: all = nsamples) the rows' lengths, out nstreams rows of `out_kind`
 * out_stride elements apart; gain_v / sigma_v / dc_v per-row arrays or NULL for the scalars.
 * Every element of out is written: zero from W_s on. */
void impair_ref_rows( const void *x, uint64_t stream_stride, const uint32_t *len, uint32_t nsamples, int nstreams,
	uint32_t kind, uint32_t out_kind, void *out, uint64_t out_stride, uint64_t seed, uint64_t first_stream,
	uint64_t first_sample, const float *gain_v, const float *sigma_v, const float *dc_v, float gain, float sigma,
	float dc )
{
    for ( int s = 0; s < nstreams; s++ ) {
	uint64_t W = len ? len[s] : nsamples;
	if ( x && W > stream_stride )
	    W = stream_stride;
	if ( W > out_stride )
	    W = out_stride;
	const double g = (double)( gain_v ? gain_v[s] : gain ), sg = (double)( sigma_v ? sigma_v[s] : sigma ),
		     d = (double)( dc_v ? dc_v[s] : dc );
	for ( uint64_t i = 0; i < out_stride; i++ ) {
	    float o = 0.0f;
	    if ( i < W ) {
		double xv = 0.0;
		if ( x ) {
		    if ( kind == IMPAIR_REF_S16 )
			xv = (double)( (float)( (const int16_t *)x )[(uint64_t)s * stream_stride + i] / 32768.0f );
		    else
			xv = (double)( (const float *)x )[(uint64_t)s * stream_stride + i];
		}
		double v = fma(g, xv, d);
		v = fma(sg, impair_ref_z(seed, first_stream + (uint64_t)s, first_sample + i), v);
		o = (float)v;
	    }
	    if ( out_kind == IMPAIR_REF_S16 )
		( (int16_t *)out )[(uint64_t)s * out_stride + i] = i < W ? impair_ref_s16(o) : 0;
	    else
		( (float *)out )[(uint64_t)s * out_stride + i] = o;
	}
    }
}
