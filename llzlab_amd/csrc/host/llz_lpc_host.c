/*
 * llz_lpc_host.c -- linear prediction: the reference's Levinson-Durbin / Toeplitz solvers and LPC handle
 * (reference libllzfilter/llz_levinson.c:29-176, llz_lpc.c:19-95) and the float32 batch extension llz_lpc_mc.
 *
 * The solvers take host double arrays and do O(p^2) work, so they run here on the host (as the final step of llz_corr_cof
 * does), restated in the reference's operation order; this file is built with -ffp-contract=off, so every product and
 * every sum is rounded on its own and the results are the reference's bit for bit.
 */
#include <math.h>
#include <stdlib.h>
#include "../../../include/llz_levinson.h"
#include "../../../include/llz_lpc.h"
#include "llz_host.h"

/* ---- Part 1: reference symbols ---- */

static int lev_args_ok(const double *r, int p, const void *a, const void *k, const void *e, const char *who)
{
    if (!r || !a || !k || !e || p < 0 || p > LLZ_LEVINSON_ORDER_MAX) {
        llzs_set_error("%s: bad arguments (p=%d; 0 <= p <= %d, no NULL arrays)", who, p, LLZ_LEVINSON_ORDER_MAX);
        return 0;
    }
    return 1;
}

void llz_levinson(double *r, int p, double *acof, double *kcof, double *err)
{
    if (!lev_args_ok(r, p, acof, kcof, err, "llz_levinson")) return;
    if (r[0] == 0.0) {                                   /* llz_levinson.c:38-43: acof[0] and kcof[0] are not written */
        for (int i = 1; i <= p; i++) acof[i] = kcof[i] = 0.0;
        *err = 0.0;
        return;
    }
    acof[0] = 1.0;
    double e = r[0];
    for (int i = 1; i <= p; i++) {
        double acc = r[i];                               /* r[i] + a[1] r[i-1] + ... + a[i-1] r[1], left to right */
        for (int j = 1; j < i; j++) acc += acof[j] * r[i - j];
        const double k = -acc / e;
        kcof[i - 1] = k;
        acof[i] = k;
        /* a[j] += k a_old[i-j] for j = 1 .. i-1: the pair (j, i-j) read before either is written is the reference's copy
         * into tmp, value for value */
        for (int j = 1, m = i - 1; j <= m; j++, m--) {
            const double aj = acof[j], am = acof[m];
            acof[j] = aj + k * am;
            if (m != j) acof[m] = am + k * aj;
        }
        e *= 1 - k * k;
    }
    *err = e;
}

void llz_levinson1(double *r, int p, double *acof, double *kcof, double *err)
{
    if (!lev_args_ok(r, p, acof, kcof, err, "llz_levinson1")) return;
    if (r[0] == 0.0) {                                   /* llz_levinson.c:82-86; the reference's *err is undefined here */
        for (int i = 1; i <= p; i++) kcof[i] = acof[i] = 0.0;
        *err = 0.0;
        return;
    }
    for (int i = 0; i <= p; i++) acof[i] = 0.0;
    acof[0] = 1.0;
    double e = r[0];                                     /* p == 0: the reference's *err is undefined; r[0] here */
    for (int m = 1; m <= p; m++) {
        double s = 0.0;                                  /* a[1] r[m-1] + ... + a[m-1] r[1], from zero */
        for (int k = 1; k < m; k++) s += acof[k] * r[m - k];
        const double km = (r[m] - s) / e;
        kcof[m - 1] = -km;
        acof[m] = km;
        for (int j = 1, q = m - 1; j <= q; j++, q--) {   /* a[k] = a_old[k] - km a_old[m-k], pairwise as above */
            const double aj = acof[j], aq = acof[q];
            acof[j] = aj - km * aq;
            if (q != j) acof[q] = aq - km * aj;
        }
        e = (1 - km * km) * e;
    }
    *err = e;
}

static int atlvs_tiny(double a) { return fabs(a) + 1.0 == 1.0; }

int llz_atlvs(double *r, int n, double *b, double *x, double *kcof, double *err)
{
    if (!r || !b || !x || !kcof || !err || n < 1 || n > LLZ_LEVINSON_ORDER_MAX) {
        llzs_set_error("llz_atlvs: bad arguments (n=%d; 1 <= n <= %d, no NULL arrays)", n, LLZ_LEVINSON_ORDER_MAX);
        return -1;
    }
    double y[LLZ_LEVINSON_ORDER_MAX] = {0}, s[LLZ_LEVINSON_ORDER_MAX] = {0};
    double a = r[0];
    if (atlvs_tiny(a)) return -1;
    y[0] = 1.0;
    x[0] = b[0] / a;
    for (int k = 1; k < n; k++) {
        double beta = 0.0, q = 0.0;                      /* two running sums over j = 0 .. k-1 */
        for (int j = 0; j < k; j++) {
            beta = beta + y[j] * r[j + 1];
            q = q + x[j] * r[k - j];
        }
        if (atlvs_tiny(a)) return -1;
        const double c = -beta / a;
        kcof[k - 1] = c;
        s[0] = c * y[k - 1];
        y[k] = y[k - 1];
        for (int i = 1; i < k; i++) s[i] = y[i - 1] + c * y[k - 1 - i];
        a = a + c * beta;
        if (atlvs_tiny(a)) return -1;
        const double h = (b[k] - q) / a;
        for (int i = 0; i < k; i++) {
            x[i] = x[i] + h * s[i];
            y[i] = s[i];
        }
        x[k] = h * y[k];
    }
    *err = a;
    return 0;
}

#define LLZ_TAG_LPC1 0x4c5a4c31

typedef struct {
    llz_head_t head;                                     /* device -1, no stream: the calls run where the caller is */
    int p;
    double *r, *acof, *kcof, err;                        /* llz_lpc.c:19-27: the state that outlives a call */
    double *d_r;
    llz_stage_t st_x;
} lpc1_t;

static void lpc1_destroy(lpc1_t *f)
{
    llzs_free(f->d_r);
    llz_stage_release(&f->st_x);
    free(f->r); free(f->acof); free(f->kcof);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_lpc_init(int p)
{
    if (p < 0 || p > LLZ_LEVINSON_ORDER_MAX) {
        llzs_set_error("llz_lpc_init: p=%d (0 <= p <= %d)", p, LLZ_LEVINSON_ORDER_MAX);
        return LLZ_BAD_HANDLE;
    }
    lpc1_t *f = (lpc1_t *)llz_handle_new(sizeof(*f), LLZ_TAG_LPC1, 0);
    if (!f) return LLZ_BAD_HANDLE;
    f->p = p;
    f->r = (double *)calloc((size_t)p + 1, sizeof(double));         /* zeroed, as llz_lpc.c:38-43 */
    f->acof = (double *)calloc((size_t)p + 1, sizeof(double));
    f->kcof = (double *)calloc((size_t)p + 1, sizeof(double));
    f->d_r = (double *)llzs_malloc(sizeof(double) * ((size_t)p + 1));  /* NULL without a GPU: no CPU path */
    if (!f->r || !f->acof || !f->kcof || !f->d_r) {
        lpc1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_lpc_uninit(unsigned long handle)
{
    lpc1_t *f = (lpc1_t *)llz_handle(handle, LLZ_TAG_LPC1, NULL);
    if (f) lpc1_destroy(f);
}

double llz_lpc(unsigned long handle, double *x, int x_len, double *lpc_cof, double *kcof, double *err)
{
    lpc1_t *f = (lpc1_t *)llz_handle(handle, LLZ_TAG_LPC1, NULL);
    if (!f || !x || !lpc_cof || !kcof || !err || x_len < 1) {
        llzs_set_error("llz_lpc: bad handle or arguments (x_len=%d)", x_len);
        return 0.0;
    }
    const int p = f->p;
    /* llz_autocorr (llz_corr.c:33-42) on the device in its own summation order, into the handle's r */
    const size_t xb = sizeof(double) * (size_t)x_len, rb = sizeof(double) * ((size_t)p + 1);
    double *d_x = (double *)llz_stage_reserve(&f->st_x, xb);
    if (!d_x || llzs_h2d(d_x, x, xb, NULL) != LLZ_OK || llzs_corr_exact_f64(d_x, d_x, x_len, p, f->d_r, NULL) != LLZ_OK ||
        llzs_d2h(f->r, f->d_r, rb, NULL) != LLZ_OK)
        return 0.0;                                      /* message set by the shim; outputs untouched */
    llz_levinson(f->r, p, f->acof, f->kcof, &f->err);
    *err = f->err / x_len;
    for (int k = 0; k <= p; k++) {                       /* all p + 1 entries of both, stale ones included */
        lpc_cof[k] = f->acof[k];
        kcof[k] = f->kcof[k];
    }
    return f->err > 0 ? f->r[0] / f->err : 0.0;
}

/* ---- Part 2: batch extension ---- */

int llz_lpc_mc(const float *x, const float *win, float *acof, float *kcof, float *err, float *gain, float *r,
               int frames, int n, int p, void *stream)
{
    if (!x || !acof || frames < 1 || n < 1 || p < 0 || p > LLZ_LEVINSON_ORDER_MAX || p >= n) {
        llzs_set_error("llz_lpc_mc: frames %d n %d p %d (frames >= 1, 0 <= p <= %d, p < n, x and acof not NULL)", frames,
                       n, p, LLZ_LEVINSON_ORDER_MAX);
        return LLZ_ERR_ARG;
    }
    const size_t F = (size_t)frames, P1 = (size_t)p + 1, fb = sizeof(float);
    enum { BX, BW, BA, BK, BE, BG, BR, BXW, BRS, NB };
    llz_bind_t b[NB] = {{"x", x, fb * F * n, LLZ_BIND_IN, NULL, 0, 0}, {"win", win, fb * n, LLZ_BIND_IN, NULL, 0, 0},
                        {"acof", acof, fb * F * P1, LLZ_BIND_OUT, NULL, 0, 0}, {"kcof", kcof, fb * F * p, LLZ_BIND_OUT, NULL, 0, 0},
                        {"err", err, fb * F, LLZ_BIND_OUT, NULL, 0, 0}, {"gain", gain, fb * F, LLZ_BIND_OUT, NULL, 0, 0},
                        {"r", r, fb * F * P1, LLZ_BIND_OUT, NULL, 0, 0},
                        {"x * win", NULL, 0, LLZ_BIND_SCRATCH, NULL, 0, 0}, {"r", NULL, 0, LLZ_BIND_SCRATCH, NULL, 0, 0}};
    const int split = p > 32 || llzs_tune(LLZS_TUNE_LPC_SPLIT) == 1;
    int rc = llz_bind("llz_lpc_mc", b, NB, stream);
    if (rc == LLZ_OK) b[BRS].staged = 1;    /* a call has always returned synchronised: llz_bind_finish waits even where nothing was staged */
    if (rc == LLZ_OK && !split) {
        rc = llzs_lpc_fused_f32((const float *)b[BX].dev, (const float *)b[BW].dev, (float *)b[BA].dev, (float *)b[BK].dev,
                                (float *)b[BE].dev, (float *)b[BG].dev, (float *)b[BR].dev, frames, n, p, stream);
    } else if (rc == LLZ_OK) {
        /* llz_autocorr_mc's kernel (on x*win when a window is given), then the recursion */
        const float *xin = (const float *)b[BX].dev;
        float *rr = (float *)b[BR].dev;
        if (b[BW].dev) {
            float *xw = (float *)llz_bind_scratch(&b[BXW], fb * F * n, &rc);
            if (xw) rc = llzs_window_f32(xin, (const float *)b[BW].dev, xw, frames, n, stream);
            xin = xw;
        }
        if (!rr) rr = (float *)llz_bind_scratch(&b[BRS], fb * F * P1, &rc);
        if (rc == LLZ_OK) rc = llzs_autocorr_mc_f32(xin, rr, frames, n, p, stream);
        if (rc == LLZ_OK)
            rc = llzs_levinson_f32(rr, (float *)b[BA].dev, (float *)b[BK].dev, (float *)b[BE].dev, (float *)b[BG].dev, frames, n,
                                   p, stream);
    }
    return llz_bind_finish(b, NB, stream, rc);
}
