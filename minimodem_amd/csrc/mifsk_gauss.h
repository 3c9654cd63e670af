/*
 * mifsk_gauss.h -- the noise field of mifsk_impair_batch (include/mifsk.h):
 * Philox4x32-10 and the Box-Muller transform from exact operations, for the device kernel
 * (mifsk_impair.hip) and for the library's host side alike -- the one place both take them from.
 *
 * Every operation below is an integer operation or ONE IEEE double operation: +, -, *, /, sqrt
 * and fma, each rounded once.  Every a * b + c that the definition fuses is written as fma();
 * nothing else may be fused, so both sides compile with -ffp-contract=off.  The constants are
 * single double divisions that the compiler folds (correctly rounded, on both sides).  f64
 * division and square root are correctly rounded on gfx950 (mifsk_devmath.h).
 * PINNED: tools/impair_ref.c restates the definition from the header comment without this file;
 * tests/test_impair_ref.py compares the two on the host bit for bit, tools/gauss_check.c compares
 * R, C and S with the C library over all 2^32 words, and tests/test_gpu_impair.py compares the
 * device with the restatement (mifsk_selftest_gauss for the transform's corners).
 */
#ifndef MIFSK_GAUSS_H
#define MIFSK_GAUSS_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef MIFSK_HD
#ifdef __HIPCC__
#define MIFSK_HD __host__ __device__ __forceinline__
#else
#define MIFSK_HD static inline
#endif
#endif

/* Philox4x32-10 (Salmon et al., SC'11): counter c[4] -> words c[4] under key (k0, k1) */
MIFSK_HD void mifsk_philox4x32_10( uint32_t c[4], uint32_t k0, uint32_t k1 )
{
    for ( int round = 0; round < 10; round++ ) {
	const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
	const uint32_t n0 = (uint32_t)( p1 >> 32 ) ^ c[1] ^ k0, n2 = (uint32_t)( p0 >> 32 ) ^ c[3] ^ k1;
	c[0] = n0;
	c[1] = (uint32_t)p1;
	c[2] = n2;
	c[3] = (uint32_t)p0;
	k0 += 0x9E3779B9u;
	k1 += 0xBB67AE85u;
    }
}

/* the words of block j of stream S under `seed`: the normals of samples 4 j .. 4 j + 3 */
MIFSK_HD void mifsk_gauss_words( uint64_t seed, uint64_t S, uint64_t j, uint32_t w[4] )
{
    w[0] = (uint32_t)j;
    w[1] = (uint32_t)( j >> 32 );
    w[2] = (uint32_t)S;
    w[3] = (uint32_t)( S >> 32 );
    mifsk_philox4x32_10(w, (uint32_t)seed, (uint32_t)( seed >> 32 ));
}

/* R(w) = sqrt(-2 ln u), u = (w + 1) / 2^32: ln of t = w + 1 = m 2^e with m in (sqrt(1/2), sqrt 2]
 * as 2 atanh(s), s = (m - 1) / (m + 1), by its odd series to s^23 */
MIFSK_HD double mifsk_gauss_r( uint32_t w )
{
    const double t = (double)( (uint64_t)w + 1u );		/* exact: 1 .. 2^32 */
    uint64_t bits;
    memcpy(&bits, &t, sizeof(bits));
    int e = (int)( bits >> 52 ) - 1023;				/* floor(log2 t) */
    bits = ( bits & 0x000FFFFFFFFFFFFFull ) | 0x3FF0000000000000ull;
    double m;							/* t 2^-e, in [1, 2) */
    memcpy(&m, &bits, sizeof(m));
    if ( m > 0x1.6a09e667f3bcdp+0 ) {
	m = m * 0.5;
	e = e + 1;
    }
    const double f = m - 1.0;
    const double s = f / ( 2.0 + f );
    const double y = s * s;
    double p = 1.0 / 23.0;
    p = fma(p, y, 1.0 / 21.0);
    p = fma(p, y, 1.0 / 19.0);
    p = fma(p, y, 1.0 / 17.0);
    p = fma(p, y, 1.0 / 15.0);
    p = fma(p, y, 1.0 / 13.0);
    p = fma(p, y, 1.0 / 11.0);
    p = fma(p, y, 1.0 / 9.0);
    p = fma(p, y, 1.0 / 7.0);
    p = fma(p, y, 1.0 / 5.0);
    p = fma(p, y, 1.0 / 3.0);
    p = fma(p, y, 1.0 / 1.0);
    const double lnm = ( 2.0 * s ) * p;
    const double ln = fma((double)( e - 32 ), 0x1.62e42fefa39efp-1, lnm);
    return sqrt(-2.0 * ln);
}

/* C(w), S(w) = cos, sin of 2 pi w / 2^32: the octant q = w >> 29, the angle folded into [0, pi/4],
 * both Taylor series (to phi^19 and phi^20) */
MIFSK_HD void mifsk_gauss_cs( uint32_t w, double *c_out, double *s_out )
{
    const uint32_t q = w >> 29, fr = w & 0x1FFFFFFFu;
    const uint32_t a = ( q & 1u ) ? 0x20000000u - fr : fr;
    const double phi = 0x1.921fb54442d18p-1 * ( (double)a * 0x1p-29 );
    const double y = phi * phi;
    double ps = -1.0 / 121645100408832000.0;			/* 19! */
    ps = fma(ps, y, 1.0 / 355687428096000.0);			/* 17! */
    ps = fma(ps, y, -1.0 / 1307674368000.0);			/* 15! */
    ps = fma(ps, y, 1.0 / 6227020800.0);			/* 13! */
    ps = fma(ps, y, -1.0 / 39916800.0);				/* 11! */
    ps = fma(ps, y, 1.0 / 362880.0);				/* 9! */
    ps = fma(ps, y, -1.0 / 5040.0);				/* 7! */
    ps = fma(ps, y, 1.0 / 120.0);				/* 5! */
    ps = fma(ps, y, -1.0 / 6.0);				/* 3! */
    ps = fma(ps, y, 1.0 / 1.0);					/* 1! */
    const double sn = phi * ps;
    double pc = 1.0 / 2432902008176640000.0;			/* 20! */
    pc = fma(pc, y, -1.0 / 6402373705728000.0);			/* 18! */
    pc = fma(pc, y, 1.0 / 20922789888000.0);			/* 16! */
    pc = fma(pc, y, -1.0 / 87178291200.0);			/* 14! */
    pc = fma(pc, y, 1.0 / 479001600.0);				/* 12! */
    pc = fma(pc, y, -1.0 / 3628800.0);				/* 10! */
    pc = fma(pc, y, 1.0 / 40320.0);				/* 8! */
    pc = fma(pc, y, -1.0 / 720.0);				/* 6! */
    pc = fma(pc, y, 1.0 / 24.0);				/* 4! */
    pc = fma(pc, y, -1.0 / 2.0);				/* 2! */
    pc = fma(pc, y, 1.0 / 1.0);					/* 0! */
    const double cs = pc;
    /* (C, S) for q = 0 .. 7: (cs, sn) (sn, cs) (-sn, cs) (-cs, sn) (-cs, -sn) (-sn, -cs) (sn, -cs) (cs, -sn) */
    const int swap = (int)( ( q + 1u ) & 2u ), cneg = (int)( ( q + 2u ) & 4u ), sneg = (int)( q & 4u );
    const double cv = swap ? sn : cs, sv = swap ? cs : sn;
    *c_out = cneg ? -cv : cv;
    *s_out = sneg ? -sv : sv;
}

/* the two normals of the word pair (wr, wa): R(wr) C(wa), R(wr) S(wa) */
MIFSK_HD void mifsk_gauss_pair( uint32_t wr, uint32_t wa, double *z0, double *z1 )
{
    const double r = mifsk_gauss_r(wr);
    double c, s;
    mifsk_gauss_cs(wa, &c, &s);
    *z0 = r * c;
    *z1 = r * s;
}

/* z[0..3]: the normals of samples 4 j .. 4 j + 3 of stream S */
MIFSK_HD void mifsk_gauss_block( uint64_t seed, uint64_t S, uint64_t j, double z[4] )
{
    uint32_t w[4];
    mifsk_gauss_words(seed, S, j, w);
    mifsk_gauss_pair(w[0], w[1], &z[0], &z[1]);
    mifsk_gauss_pair(w[2], w[3], &z[2], &z[3]);
}

#endif /* MIFSK_GAUSS_H */
