/*
 * include/llz_levinson.h -- Levinson-Durbin and Toeplitz solvers, C ABI of libllzfilter_hip.so (reference
 * libllzfilter/llz_levinson.h:20-27, llz_levinson.c:29-176).  Host `double` arrays, O(p^2) work: computed on the host in the
 * reference's operation order with contraction off, bit-identical to the reference.
 *
 * Defined where the reference is not: orders above LLZ_LEVINSON_ORDER_MAX (the reference's stack arrays overflow), orders
 * below 0 and NULL arrays are refused -- llz_hip_last_error() says why, the outputs are left untouched, llz_atlvs returns -1.
 */
#ifndef LLZ_LEVINSON_H
#define LLZ_LEVINSON_H

#ifdef __cplusplus
extern "C" {
#endif

#define LLZ_LEVINSON_ORDER_MAX 64     /* llz_levinson.h:20 */

/* Levinson-Durbin on r[0..p]: acof[0..p] (acof[0] = 1), kcof[0..p-1], *err = the order-p prediction error
 * (llz_levinson.c:29-67).  When r[0] == 0 it writes acof[1..p] = kcof[1..p] = 0 and *err = 0 and leaves acof[0] and
 * kcof[0] as they were (so kcof needs p + 1 entries in that case) -- the reference's behaviour, kept. */
void llz_levinson(double *r, int p, double *acof, double *kcof, double *err);
/* the same recursion in the other sign convention (llz_levinson.c:73-120): acof[1..p] are the NEGATED coefficients of
 * llz_levinson, kcof the same.  Where the reference reads an uninitialised error (r[0] == 0, or p == 0), *err is defined
 * here: 0 when r[0] == 0, r[0] when p == 0. */
void llz_levinson1(double *r, int p, double *acof, double *kcof, double *err);
/* solves the symmetric Toeplitz system T(r[0..n-1]) x = b (llz_levinson.c:123-176): x[0..n-1],
 * kcof[0..n-2], *err; returns 0, or -1 when the system is singular (|a| + 1 == 1 at any step; outputs then partly written,
 * as in the reference) or the arguments are refused (1 <= n <= 64). */
int  llz_atlvs(double *r, int n, double *b, double *x, double *kcof, double *err);

#ifdef __cplusplus
}
#endif
#endif
