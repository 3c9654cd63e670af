/* tools/angle_check.c -- minimodem_amd/csrc/mifsk_angle.h (the FM stage's angle, as the device
 * compiles it) for the host, against the C library: mifsk_turn(y, x) with atan2l(y, x) / (2 pi) on
 * `n` pseudo-random finite pairs.
 *     gcc -O2 -ffp-contract=off -o /tmp/angle_check tools/angle_check.c -lm
 *     /tmp/angle_check [n]          prints the largest difference; exit status 0 iff it is at most
 *                                   4e-12 turns (the series' 1.7e-12 and the rounding)
 * As a shared object (tests/_fm.py) it also hands the header's function to a caller:
 * angle_check_turns. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../minimodem_amd/csrc/mifsk_angle.h"

/* out[i] = mifsk_turn(y[i], x[i]) */
void angle_check_turns( const double *y, const double *x, uint64_t n, double *out )
{
    for ( uint64_t i = 0; i < n; i++ )
	out[i] = mifsk_turn(y[i], x[i]);
}

/* the largest |mifsk_turn - atan2l / (2 pi)| over n pairs of a 64-bit LCG in [-1, 1)^2 */
double angle_check_sweep( uint64_t n )
{
    const long double two_pi = 6.28318530717958647692528676655900577L;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    long double worst = 0.0L;
    for ( uint64_t i = 0; i < n; i++ ) {
	state = state * 6364136223846793005ull + 1442695040888963407ull;
	const double x = (double)(int64_t)state * 0x1p-63;
	state = state * 6364136223846793005ull + 1442695040888963407ull;
	const double y = (double)(int64_t)state * 0x1p-63;
	const long double d = fabsl((long double)mifsk_turn(y, x) - atan2l((long double)y, (long double)x) / two_pi);
	if ( d > worst )
	    worst = d;
    }
    return (double)worst;
}

int main( int argc, char **argv )
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], NULL, 0) : 10000000ull;
    const double worst = angle_check_sweep(n);
    printf("%llu pairs: max |turn - atan2 / (2 pi)| = %.3g turns (bound 4e-12)\n", (unsigned long long)n, worst);
    return !( worst <= 4e-12 );
}
