/*
 * mifsk_angle.h -- the angle of the FM stage (include/mifsk.h: mifsk_fm_demod_batch, DESIGN.md
 * 4.17): mifsk_turn(y, x), the argument of x + i y in TURNS, [-0.5, 0.5], from exact operations,
 * for the device kernel (mifsk_fm.hip, mifsk_selftest.hip) and for the library's host side alike.
 *
 * Every operation below is a comparison, a selection, a change of sign or ONE IEEE double
 * operation: +, -, *, / and fma, each rounded once.  Every a * b + c that the definition fuses is
 * written as fma(); nothing else may be fused, so both sides compile with -ffp-contract=off.  The
 * series' constants are single double divisions that the compiler folds (correctly rounded, on
 * both sides).  f64 division is correctly rounded on gfx950 (mifsk_devmath.h).
 *   The larger of |x|, |y| goes below the line, so the quotient lies in [0, 1]; above tan(pi/8)
 * it is turned back by pi/4 -- (mn - mx) / (mn + mx) = tan(atan(mn / mx) - pi/4) -- so that ONE
 * division leaves |u| <= tan(pi/8), where the odd series to u^23 is off by u^25 / 25 at most:
 * 1.7e-12 turns.  Nothing is special-cased: a NaN or Inf / Inf comes out as a NaN because the
 * arithmetic says so (y a NaN beside x = +-0.0 excepted: the largest magnitude is then 0.0 by the
 * comparisons, and the answer 0.0).
 * PINNED: tools/fm_ref.c restates the definition from the header comment without this file;
 * tests/test_fm_ref.py compares the two on the host bit for bit (tools/angle_check.c is this
 * file compiled for the host) and with atan2, tests/test_gpu_fm.py compares the device with the
 * restatement (mifsk_selftest_turn).
 */
#ifndef MIFSK_ANGLE_H
#define MIFSK_ANGLE_H

#include <math.h>

#ifndef MIFSK_HD
#ifdef __HIPCC__
#define MIFSK_HD __host__ __device__ __forceinline__
#else
#define MIFSK_HD static inline
#endif
#endif

MIFSK_HD double mifsk_turn( double y, double x )
{
    const double ax = fabs(x), ay = fabs(y);
    const int sw = ay > ax;
    const double mx = sw ? ay : ax, mn = sw ? ax : ay;
    double a = 0.0;
    if ( !( mx == 0.0 ) ) {
	const int big = mn > mx * 0x1.a827999fcef32p-2;		/* tan(pi/8) */
	const double num = big ? mn - mx : mn, den = big ? mn + mx : mx;
	const double u = num / den;
	const double v = u * u;
	double p = -1.0 / 23.0;
	p = fma(p, v, 1.0 / 21.0);
	p = fma(p, v, -1.0 / 19.0);
	p = fma(p, v, 1.0 / 17.0);
	p = fma(p, v, -1.0 / 15.0);
	p = fma(p, v, 1.0 / 13.0);
	p = fma(p, v, -1.0 / 11.0);
	p = fma(p, v, 1.0 / 9.0);
	p = fma(p, v, -1.0 / 7.0);
	p = fma(p, v, 1.0 / 5.0);
	p = fma(p, v, -1.0 / 3.0);
	p = fma(p, v, 1.0 / 1.0);
	const double r = u * p;
	a = fma(r, 0x1.45f306dc9c883p-3, big ? 0.125 : 0.0);	/* 1 / (2 pi) */
    }
    if ( sw )
	a = 0.25 - a;
    if ( x < 0.0 )
	a = 0.5 - a;
    if ( y < 0.0 )
	a = -a;
    return a;
}

#endif /* MIFSK_ANGLE_H */
