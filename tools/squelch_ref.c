/* squelch_ref.c -- the power squelch's definition (include/mifsk/squelch.h: mifsk_fm_squelch_batch,
 * mifsk_fm_squelch_level) restated for the host from the header comment and nothing else,
 * as plain serial loops: one element after the other, the window closed when its last element has come,
 * the gate stepped as the header's machine, the audio zeroed under the gate of that moment.  It is the
 * yardstick the device kernels are compared with (tests/_squelch.py compiles it into a temporary shared
 * object with -O2 -ffp-contract=off; tests/test_squelch_ref.py, tests/test_gpu_squelch.py).  Never linked
 * into libmifsk.so.
 *
 *   cc -O2 -ffp-contract=off -shared -fPIC -o squelch_ref.so tools/squelch_ref.c -lm
 */
#include <math.h>
#include <stdint.h>

#define SQUELCH_REF_S16 1		/* MIFSK_FEED_S16 */

typedef struct squelch_ref_state {
    uint64_t	seen, acc, span_first;
    uint32_t	open, low;
} squelch_ref_state;

/* the energy of a sample of power p: 40 fractional bits, full scale from 256 on and for a NaN */
uint64_t squelch_ref_scale( double p )
{
    if ( p < 256.0 )
	return (uint64_t)rint(p * 0x1p40);
    return (uint64_t)1 << 48;
}

/* the energy of one sample */
uint64_t squelch_ref_energy( float i, float q )
{
    const double a = (double)i, b = (double)q;
    const double bb = b * b;
    const double p = fma(a, a, bb);
    return squelch_ref_scale(p);
}

/* out[n] = the energy of (iq[2 n], iq[2 n + 1]) */
void squelch_ref_energies( const float *iq, uint64_t n, uint64_t *out )
{
    for ( uint64_t k = 0; k < n; k++ )
	out[k] = squelch_ref_energy(iq[2 * k], iq[2 * k + 1]);
}

/* the window energy of B samples at dbfs */
uint64_t squelch_ref_level( double dbfs, uint32_t B )
{
    if ( B == 0 )
	return 0;
    const double top = (double)B * 0x1p48;
    const double v = rint(pow(10.0, dbfs / 10.0) * 0x1p40 * (double)B);
    if ( !( v >= 1.0 ) )
	return 1;
    if ( v >= top )
	return (uint64_t)B << 48;
    return (uint64_t)v;
}

/* scalar j (0: I, 1: Q) of element i of a row, as a float */
static float scalar_at( const void *row, uint32_t kind, uint64_t i, int j )
{
    if ( kind == SQUELCH_REF_S16 )
	return (float)( (const int16_t *)row )[2 * i + j] / 32768.0f;
    return ( (const float *)row )[2 * i + j];
}

/* The squelch on host arrays: x is nstreams rows of interleaved I, Q of `kind`, stream_stride complex
 * elements apart; len (NULL: all = nsamples) the rows' lengths; state (or NULL: zeros) and state_out (or
 * NULL; it may be state) [nstreams]; energy and gate (or NULL) rows of win_stride entries; nwindows
 * [nstreams]; spans (or NULL) [nstreams][span_cap][2], nspans (or NULL) [nstreams]; audio (or NULL) rows of
 * audio_stride floats.  Only what the header says is written is written. */
void squelch_ref_rows( const void *x, uint64_t stream_stride, const uint32_t *len, uint32_t nsamples, int nstreams,
	uint32_t kind, uint32_t B, uint32_t hang, uint64_t open_level, uint64_t close_level,
	const squelch_ref_state *state, squelch_ref_state *state_out, uint64_t *energy, uint8_t *gate,
	uint64_t win_stride, uint32_t *nwindows, uint64_t *spans, uint32_t *nspans, uint32_t span_cap, float *audio,
	uint64_t audio_stride )
{
    const uint64_t scalar_bytes = kind == SQUELCH_REF_S16 ? 2 : 4;
    for ( int s = 0; s < nstreams; s++ ) {
	uint64_t W = len ? len[s] : nsamples;
	if ( W > stream_stride )
	    W = stream_stride;
	const void *row = (const char *)x + (uint64_t)s * stream_stride * 2 * scalar_bytes;
	uint64_t seen = 0, acc = 0, span_first = 0, low = 0;
	int open = 0;
	if ( state ) {
	    seen = state[s].seen;
	    acc = state[s].acc;
	    span_first = state[s].span_first;
	    open = state[s].open != 0;
	    low = open ? state[s].low : 0;			/* a closed gate counts nothing */
	}
	uint32_t nw = 0, count = 0;
	int in_span = 0;
	for ( uint64_t i = 0; i < W; i++ ) {
	    if ( audio && !open )				/* the gate of this moment */
		audio[(uint64_t)s * audio_stride + i] = 0.0f;
	    acc += squelch_ref_energy(scalar_at(row, kind, i, 0), scalar_at(row, kind, i, 1));
	    seen += 1;
	    if ( seen % B != 0 )
		continue;
	    /* the window is complete */
	    const uint64_t w = seen / B - 1, E = acc;
	    acc = 0;
	    if ( E >= open_level ) {
		if ( !open )
		    span_first = w;
		open = 1;
		low = 0;
	    } else if ( open ) {
		if ( E >= close_level ) {
		    low = 0;
		} else {
		    low += 1;
		    if ( low > hang ) {
			open = 0;
			low = 0;
		    }
		}
	    }
	    if ( energy )
		energy[(uint64_t)s * win_stride + nw] = E;
	    if ( gate )
		gate[(uint64_t)s * win_stride + nw] = (uint8_t)open;
	    nw += 1;
	    if ( open ) {
		if ( !in_span ) {
		    in_span = 1;
		    count += 1;
		    if ( spans && count <= span_cap )
			spans[2 * ( (uint64_t)s * span_cap + count - 1 )] = span_first;
		}
		if ( spans && count <= span_cap )
		    spans[2 * ( (uint64_t)s * span_cap + count - 1 ) + 1] = w + 1;
	    } else {
		in_span = 0;
	    }
	}
	nwindows[s] = nw;
	if ( nspans )
	    nspans[s] = count;
	if ( state_out ) {
	    state_out[s].seen = seen;
	    state_out[s].acc = acc;
	    state_out[s].span_first = span_first;
	    state_out[s].open = (uint32_t)open;
	    state_out[s].low = (uint32_t)low;
	}
    }
}
