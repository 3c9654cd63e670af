/* tools/gauss_check.c -- minimodem_amd/csrc/mifsk_gauss.h (the transform of the channel model's
 * noise field, as the device compiles it) against the C library: R(w) with sqrtl(-2 logl((w + 1) /
 * 2^32)) and C(w), S(w) with cosl, sinl of 2 pi w / 2^32, over every `stride`-th of the 2^32 words
 * (stride 1 = all of them).
 *     gcc -O2 -mfma -ffp-contract=off -o /tmp/gauss_check tools/gauss_check.c -lm
 *     /tmp/gauss_check [stride]     prints the largest differences; exit status 0 iff both are
 *                                   at most 2^-40
 * As a shared object (tests/_impair.py) it also hands the header's functions to a caller:
 * gauss_check_words, gauss_check_field. */
#include <stdio.h>
#include <stdlib.h>
#include "../minimodem_amd/csrc/mifsk_gauss.h"

/* n pairs of words [n][2] -> rcs[n][3] = R(w[0]), C(w[1]), S(w[1]) and z[n][2]; either may be NULL */
void gauss_check_words( const uint32_t *words, uint64_t n, double *rcs, double *z )
{
    for ( uint64_t i = 0; i < n; i++ ) {
	if ( rcs ) {
	    rcs[3 * i] = mifsk_gauss_r(words[2 * i]);
	    mifsk_gauss_cs(words[2 * i + 1], &rcs[3 * i + 1], &rcs[3 * i + 2]);
	}
	if ( z )
	    mifsk_gauss_pair(words[2 * i], words[2 * i + 1], &z[2 * i], &z[2 * i + 1]);
    }
}

/* words[4] of counter (j, S) under seed, and out[i] = z(seed, S, 4 j0 + i) for i < 4 * nblocks */
void gauss_check_field( uint64_t seed, uint64_t S, uint64_t j0, uint64_t nblocks, uint32_t *words, double *out )
{
    if ( words )
	mifsk_gauss_words(seed, S, j0, words);
    for ( uint64_t b = 0; out && b < nblocks; b++ )
	mifsk_gauss_block(seed, S, j0 + b, out + 4 * b);
}

/* the sweep: max[0] = max |R - libm|, max[1] = max |C, S - libm| */
void gauss_check_sweep( uint64_t stride, double *max )
{
    const long double pi = 3.14159265358979323846264338327950288L;
    long double mr = 0.0L, ma = 0.0L;
    for ( uint64_t u = 0; u <= 0xFFFFFFFFull; u += stride ) {
	const uint32_t w = (uint32_t)u;
	const long double r = sqrtl(-2.0L * logl(( (long double)w + 1.0L ) * 0x1p-32L));
	const long double ang = ( (long double)w * 0x1p-31L ) * pi;
	double c, s;
	mifsk_gauss_cs(w, &c, &s);
	long double d = fabsl((long double)mifsk_gauss_r(w) - r);
	if ( d > mr ) mr = d;
	d = fabsl((long double)c - cosl(ang));
	if ( d > ma ) ma = d;
	d = fabsl((long double)s - sinl(ang));
	if ( d > ma ) ma = d;
    }
    max[0] = (double)mr;
    max[1] = (double)ma;
}

int main( int argc, char **argv )
{
    const uint64_t stride = argc > 1 ? strtoull(argv[1], NULL, 0) : 1;
    double max[2];
    gauss_check_sweep(stride ? stride : 1, max);
    printf("stride %llu: max |R - libm| = %.3g, max |C, S - libm| = %.3g (bound 2^-40 = %.3g)\n",
	   (unsigned long long)( stride ? stride : 1 ), max[0], max[1], 0x1p-40);
    return !( max[0] <= 0x1p-40 && max[1] <= 0x1p-40 );
}
