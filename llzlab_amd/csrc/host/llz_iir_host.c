/*
 * llz_iir_host.c -- handle layer of the IIR path: the reference's single-channel direct-form-I symbols
 * (reference libllzfilter/llz_iir.c:37-156) and the multi-channel biquad-cascade extension.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_iir.h"
#include "llz_host.h"

/* ---- Part 1: single channel, double, exact order (k_iir_df1_f64_exact) ---- */

typedef struct {
    int tag;
    int M, N;
    double *d_a, *d_b, *d_xs, *d_ys;     /* coefficients and delay lines live on the device between calls */
    llz_stage_t st_in, st_out;
} iir1_t;

static void iir1_destroy(iir1_t *f)
{
    if (!f) return;
    llzs_free(f->d_a); llzs_free(f->d_b); llzs_free(f->d_xs); llzs_free(f->d_ys);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->tag = 0;
    free(f);
}

unsigned long llz_iir_filter_init(int M, double *a, int N, double *b)
{
    if (M < 0 || N < 0 || M > 1024 || N > 1024 || !a) {
        llzs_set_error("llz_iir_filter_init: M=%d N=%d (0..1024) or NULL a", M, N);
        return LLZ_BAD_HANDLE;
    }
    iir1_t *f = (iir1_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_IIR1;
    f->M = M; f->N = N;
    double *bz = (double *)calloc((size_t)N + 1, sizeof(double));      /* b == NULL -> zeros (llz_iir.c:54-59) */
    int rc = bz ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        if (b) memcpy(bz, b, sizeof(double) * ((size_t)N + 1));
        f->d_a = (double *)llzs_malloc(sizeof(double) * ((size_t)M + 1));
        f->d_b = (double *)llzs_malloc(sizeof(double) * ((size_t)N + 1));
        f->d_xs = (double *)llzs_malloc(sizeof(double) * ((size_t)N + 1));
        f->d_ys = (double *)llzs_malloc(sizeof(double) * ((size_t)M + 1));
        if (!f->d_a || !f->d_b || !f->d_xs || !f->d_ys) rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_a, a, sizeof(double) * ((size_t)M + 1), NULL);
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_b, bz, sizeof(double) * ((size_t)N + 1), NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_xs, 0, sizeof(double) * ((size_t)N + 1), NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_ys, 0, sizeof(double) * ((size_t)M + 1), NULL);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    free(bz);
    if (rc != LLZ_OK) {
        iir1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_iir_filter_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, iir1_t, LLZ_TAG_IIR1))
        iir1_destroy((iir1_t *)handle);
}

static int iir1_run(iir1_t *f, const double *x, double *y, int n)
{
    const size_t bytes = sizeof(double) * (size_t)n;
    double *d_in = (double *)llz_stage_reserve(&f->st_in, bytes);
    double *d_out = (double *)llz_stage_reserve(&f->st_out, bytes);
    if (!d_in || !d_out) return LLZ_ERR_NOMEM;
    int rc = x ? llzs_h2d(d_in, x, bytes, NULL) : llzs_memset(d_in, 0, bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_iir_df1_f64(d_in, d_out, f->d_a, f->d_b, f->d_xs, f->d_ys, f->M, f->N, n, NULL);
    if (rc == LLZ_OK) rc = llzs_d2h(y, d_out, bytes, NULL);
    return rc;
}

int llz_iir_filter(unsigned long handle, double *x, double *y, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, iir1_t, LLZ_TAG_IIR1) || !x || !y || frame_len < 0) {
        llzs_set_error("llz_iir_filter: bad handle or buffer");
        return LLZ_ERR_ARG;
    }
    if (frame_len == 0) return 0;
    const int rc = iir1_run((iir1_t *)handle, x, y, frame_len);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_iir_filter_flush(unsigned long handle, double *y)
{
    if (!LLZ_HANDLE_OK(handle, iir1_t, LLZ_TAG_IIR1) || !y) {
        llzs_set_error("llz_iir_filter_flush: bad handle or buffer");
        return LLZ_ERR_ARG;
    }
    iir1_t *f = (iir1_t *)handle;
    if (f->N == 0) return 0;
    const int rc = iir1_run(f, NULL, y, f->N);            /* N samples of x = 0 (llz_iir.c:147-156) */
    return rc == LLZ_OK ? f->N : rc;
}

/* ---- Part 2: multi-channel biquad cascade (k_iir_cascade_f32) ---- */

#define IIRM_PIPE (-1)   /* the stage pipeline, next to the wave forms LLZS_IIR_WAVE*: what iirm_path chooses between */

typedef struct {
    int tag;
    int channels, stages;
    void *d_tab[10];     /* every coefficient table, in upload order; the views below point into them */
    int ntab;
    const double *d_coef;    /* stages x {b0,b1,b2,a1,a2} */
    /* per wave form: the tables its kernel reads (llz_shim.h), pl == NULL where the form was not built.  WAVE16_F64 reads the
     * stage pipeline's own: coef, pd [S][6][4], pl [S][64][12] */
    llzs_iir_wave_tables wave[LLZS_IIR_WAVE_FORMS];
    double *d_state;     /* [channels][stages][x1,x2,y1,y2]: the current state */
    double *d_state_alt; /* where a time-segmented launch writes the frame's end state (then the two swap) */
    int warm_chunks;     /* 1024-sample chunks after which any state error has decayed below 1e-13 (0: unknown / too long) */
    int float32_ok;      /* every section's rounding-noise gain is small enough for float32 arithmetic */
    void *stream;
    int device;          /* the device the handle's buffers live on: every call binds it */
    llz_stage_t st_in, st_out;
    /* Part 4, the bank (tag LLZ_TAG_IIRB): d_coef and the tables of wave[LLZS_IIR_BANK16_*] hold a row per channel, float32_ok
     * and warm_chunks are the handle's verdicts over all channels, and the host keeps what llz_iir_bank_mc_set_coef needs */
    double *h_c5;            /* [channels][stages][5] */
    unsigned char *h_f32ok;  /* per channel: iirm_float32_ok */
    int *h_warm;             /* per channel: iirm_memory_chunks */
    int f32_rows;            /* the float tables hold every channel's current set */
} iirm_t;

static void iirm_destroy(iirm_t *f)
{
    if (!f) return;
    free(f->h_c5); free(f->h_f32ok); free(f->h_warm);
    for (int i = 0; i < f->ntab; i++) llzs_free(f->d_tab[i]);
    llzs_free(f->d_state); llzs_free(f->d_state_alt);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->tag = 0;
    free(f);
}

/* allocate the device tables of one group, then upload them in order (llzs_h2d_table: a sharded init pairs them by index),
 * or fail; the handle owns whatever was allocated */
typedef struct {
    const void **dev;
    const void *host;
    size_t bytes;
} iirm_up_t;

static int iirm_upload(iirm_t *f, const iirm_up_t *u, int n)
{
    int rc = LLZ_OK;
    for (int i = 0; i < n; i++) {
        void *d = llzs_malloc(u[i].bytes);
        if (d) f->d_tab[f->ntab++] = d; else rc = LLZ_ERR_NOMEM;
        *u[i].dev = d;
    }
    for (int i = 0; i < n && rc == LLZ_OK; i++) rc = llzs_h2d_table((void *)*u[i].dev, u[i].host, u[i].bytes);
    return rc;
}

static void mat2_mul(const double *a, const double *b, double *o)
{
    const double r0 = a[0] * b[0] + a[1] * b[2], r1 = a[0] * b[1] + a[1] * b[3];
    const double r2 = a[2] * b[0] + a[3] * b[2], r3 = a[2] * b[1] + a[3] * b[3];
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
}

/* Powers of a section's transition matrix P = A^run, A = [[-a1,-a2],[1,0]]: the feedback recurrence (y[n-1], y[n-2]) ->
 * `run` samples later (one lane's samples).  p2 = P^(2^d) for the lane scan, pw = P^0 .. P^64, pl = per lane P^lane,
 * P^(lane%16+1), P^(lane%32+1): see k_iir_cascade_pipe_f32.  All 2 x 2 row major. */
typedef struct {
    double p2[6][4], pw[65][4], pl[64][12];
} iirm_pow_t;

static void iirm_powers(double a1, double a2, int run, iirm_pow_t *o)
{
    const double A[4] = {-a1, -a2, 1.0, 0.0};
    double P[4] = {1.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < run; i++) mat2_mul(A, P, P);
    memcpy(o->p2[0], P, sizeof(P));
    for (int d = 1; d < 6; d++) mat2_mul(o->p2[d - 1], o->p2[d - 1], o->p2[d]);
    o->pw[0][0] = 1.0; o->pw[0][1] = 0.0; o->pw[0][2] = 0.0; o->pw[0][3] = 1.0;
    for (int k = 1; k <= 64; k++) mat2_mul(P, o->pw[k - 1], o->pw[k]);
    for (int lane = 0; lane < 64; lane++) {
        memcpy(o->pl[lane], o->pw[lane], sizeof(P));
        memcpy(o->pl[lane] + 4, o->pw[lane % 16 + 1], sizeof(P));
        memcpy(o->pl[lane] + 8, o->pw[lane % 32 + 1], sizeof(P));
    }
}

/* the homogeneous responses h[2k], h[2k+1] = y[k] from (y[-1], y[-2]) = (1,0) and (0,1) with zero input, k < K */
static void iirm_h_responses(double a1, double a2, int K, float *h)
{
    double p1 = 1.0, p2 = 0.0, q1 = 0.0, q2 = 1.0;
    for (int k = 0; k < K; k++) {
        const double h1 = -a1 * p1 - a2 * p2, h2 = -a1 * q1 - a2 * q2;
        h[2 * k] = (float)h1; h[2 * k + 1] = (float)h2;
        p2 = p1; p1 = h1; q2 = q1; q1 = h2;
    }
}

/* May the b0 gains be folded out of the sections (b' = b / b0, states scaled by xfac_s = prod_{t >= s} b0_t)?  Every b0 must
 * be usable as a divisor and the partial products must stay inside the arithmetic's range; fills xfac[0..S] when so. */
typedef struct {
    double b0_min, xfac_min, xfac_max, ratio_max;
} iirm_fold_t;
/* (float32: the scaled states and the scaled input must stay clear of the denormals: signals down to 1e-10 of full scale
 *  times a partial product of 1e-20 are still 1e-30) */
static const iirm_fold_t IIRM_FOLD32 = {1e-12, 1e-20, 1e20, 1e4}, IIRM_FOLD64 = {1e-30, 1e-150, 1e150, 1e6};

static int iirm_fold(const double *c5, int S, const iirm_fold_t *lim, double *xfac)
{
    xfac[S] = 1.0;
    for (int s = S - 1; s >= 0; s--) {
        const double b0 = c5[5 * s];
        xfac[s] = xfac[s + 1] * b0;
        if (!(fabs(b0) > lim->b0_min) || !(fabs(xfac[s]) > lim->xfac_min && fabs(xfac[s]) < lim->xfac_max) ||
            !(fabs(c5[5 * s + 1] / b0) < lim->ratio_max) || !(fabs(c5[5 * s + 2] / b0) < lim->ratio_max)) return 0;
    }
    return 1;
}

/* one cascade's tables for 16 samples per lane: pd [S][6][4], pl [S][64][12] in double and their float copies pd32 [S][16],
 * pl32 [S][64][12] with cf32 [S][24] = the h responses and the coefficients (layouts: llz_shim.h) */
static void iirm_run16_rows(const double *c5, size_t S, double *pd, double *pl, float *pd32, float *pl32, float *ph32)
{
    for (size_t s = 0; s < S; s++) {
        iirm_pow_t w;
        iirm_powers(c5[5 * s + 3], c5[5 * s + 4], 16, &w);
        memcpy(pd + 24 * s, w.p2, sizeof(w.p2));
        memcpy(pl + 768 * s, w.pl, sizeof(w.pl));
        for (int i = 0; i < 16; i++) pd32[16 * s + i] = (float)pd[24 * s + i];
        for (int i = 0; i < 768; i++) pl32[768 * s + i] = (float)pl[768 * s + i];
        iirm_h_responses(c5[5 * s + 3], c5[5 * s + 4], 8, ph32 + 24 * s);
        for (int k = 0; k < 8; k++) ph32[24 * s + 16 + k] = k < 5 ? (float)c5[5 * s + k] : 0.f;
    }
}

/* 16 samples per lane: the stage pipeline's double tables (any section count; WAVE16_F64 reads them too) and, where float32
 * arithmetic is good enough, float copies with the h responses and the coefficients for WAVE16_F32 */
static int iirm_build_run16(iirm_t *f, const double *c5)
{
    const size_t S = (size_t)f->stages;
    double *pd = (double *)malloc(sizeof(double) * S * (24 + 768));
    float *pd32 = (float *)malloc(sizeof(float) * S * (16 + 768 + 24));
    int rc = (pd && pd32) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        double *pl = pd + 24 * S;
        float *pl32 = pd32 + 16 * S, *ph32 = pl32 + 768 * S;
        iirm_run16_rows(c5, S, pd, pl, pd32, pl32, ph32);
        llzs_iir_wave_tables *d = &f->wave[LLZS_IIR_WAVE16_F64], *d32 = &f->wave[LLZS_IIR_WAVE16_F32];
        const iirm_up_t up[2] = {{&d->pd, pd, sizeof(double) * 24 * S}, {&d->pl, pl, sizeof(double) * 768 * S}};
        const iirm_up_t up32[3] = {{&d32->pd, pd32, sizeof(float) * 16 * S}, {&d32->pl, pl32, sizeof(float) * 768 * S},
                                   {&d32->cf, ph32, sizeof(float) * 24 * S}};
        d->cf = f->d_coef;
        rc = iirm_upload(f, up, 2);
        if (rc == LLZ_OK && f->float32_ok) rc = iirm_upload(f, up32, 3);
    }
    free(pd); free(pd32);
    return rc;
}

/* 32 samples per lane, b0 folded out, float32 (WAVE32_F32; layouts: llz_shim.h).  Not built when the gains cannot be folded:
 * the 16-sample form runs. */
static int iirm_build_run32(iirm_t *f, const double *c5)
{
    const size_t S = (size_t)f->stages;
    double xfac[9];
    if (S > 8 || !f->float32_ok || !iirm_fold(c5, (int)S, &IIRM_FOLD32, xfac)) return LLZ_OK;
    float *pd = (float *)calloc(S * (16 + 768 + 40), sizeof(float));
    if (!pd) return LLZ_ERR_NOMEM;
    float *pl = pd + 16 * S, *ph = pl + 768 * S;
    for (size_t s = 0; s < S; s++) {
        const double b0 = c5[5 * s], a1 = c5[5 * s + 3], a2 = c5[5 * s + 4];
        iirm_pow_t w;
        iirm_powers(a1, a2, 32, &w);
        const double *p2 = &w.p2[0][0], *wl = &w.pl[0][0];
        for (int i = 0; i < 16; i++) pd[16 * s + i] = (float)p2[i];
        for (int i = 0; i < 768; i++) pl[768 * s + i] = (float)wl[i];
        iirm_h_responses(a1, a2, 16, ph + 40 * s);
        const float c[7] = {1.f, (float)(c5[5 * s + 1] / b0), (float)(c5[5 * s + 2] / b0), (float)a1, (float)a2,
                            (float)xfac[s], (float)xfac[s + 1]};
        memcpy(ph + 40 * s + 32, c, sizeof(c));
    }
    llzs_iir_wave_tables *d = &f->wave[LLZS_IIR_WAVE32_F32];
    const iirm_up_t up[3] = {{&d->pd, pd, sizeof(float) * 16 * S}, {&d->pl, pl, sizeof(float) * 768 * S},
                             {&d->cf, ph, sizeof(float) * 40 * S}};
    d->in_gain = xfac[0];
    const int rc = iirm_upload(f, up, 3);
    free(pd);
    return rc;
}

/* the same in double for the cascades float32 arithmetic is not good enough for (WAVE32_F64) */
static int iirm_build_run32d(iirm_t *f, const double *c5)
{
    const size_t S = (size_t)f->stages;
    double xfac[9];
    if (S > 8 || f->float32_ok || !iirm_fold(c5, (int)S, &IIRM_FOLD64, xfac)) return LLZ_OK;
    double *cw = (double *)calloc(S * (8 + 16 + 448), sizeof(double));
    if (!cw) return LLZ_ERR_NOMEM;
    double *pd = cw + 8 * S, *pl = pd + 16 * S;
    for (size_t s = 0; s < S; s++) {
        const double b0 = c5[5 * s];
        iirm_pow_t w;
        iirm_powers(c5[5 * s + 3], c5[5 * s + 4], 32, &w);
        const double c[6] = {c5[5 * s + 1] / b0, c5[5 * s + 2] / b0, c5[5 * s + 3], c5[5 * s + 4], xfac[s], xfac[s + 1]};
        memcpy(cw + 8 * s, c, sizeof(c));
        memcpy(pd + 16 * s, w.p2, sizeof(double) * 16);
        memcpy(pl + 448 * s, &w.pw[0][0], sizeof(double) * 4 * 64);           /* P^lane */
        memcpy(pl + 448 * s + 256, &w.pw[1][0], sizeof(double) * 4 * 16);     /* P^(i+1), i < 16 */
        memcpy(pl + 448 * s + 320, &w.pw[1][0], sizeof(double) * 4 * 32);     /* P^(i+1), i < 32 */
    }
    llzs_iir_wave_tables *d = &f->wave[LLZS_IIR_WAVE32_F64];
    const iirm_up_t up[3] = {{&d->cf, cw, sizeof(double) * 8 * S}, {&d->pd, pd, sizeof(double) * 16 * S},
                             {&d->pl, pl, sizeof(double) * 448 * S}};
    d->in_gain = xfac[0];
    const int rc = iirm_upload(f, up, 3);
    free(cw);
    return rc;
}

/* How long does the cascade remember?  The pipelined kernel may split a channel along time when there are too few
 * channels to fill the chip; a later segment then starts `warm` chunks early from the zero state.  That is sound when the
 * homogeneous response (the response to any initial state) has died out by then.  Measured here on the cascade itself:
 * unit initial outputs planted in each section in turn, zero input, the largest magnitude at any section output per
 * 1024-sample chunk; the first chunk count after which it stays below 1e-13 of its peak, or 0 if that takes more than 64
 * chunks (or the filter does not decay at all). */
static int iirm_memory_chunks(const double *c5, int S)
{
    enum { MAXC = 64, CH = 1024 };
    double env[MAXC];
    for (int k = 0; k < MAXC; k++) env[k] = 0.0;
    for (int s0 = 0; s0 < S; s0++) {
        double x1[16] = {0}, x2[16] = {0}, y1[16] = {0}, y2[16] = {0};
        y1[s0] = 1.0; y2[s0] = 1.0;
        for (int k = 0; k < MAXC; k++) {
            double m = 0.0;
            for (int i = 0; i < CH; i++) {
                double v = 0.0;
                for (int s = 0; s < S; s++) {
                    double acc = c5[5 * s] * v + c5[5 * s + 1] * x1[s] + c5[5 * s + 2] * x2[s]
                                 - c5[5 * s + 3] * y1[s] - c5[5 * s + 4] * y2[s];
                    x2[s] = x1[s]; x1[s] = v; y2[s] = y1[s]; y1[s] = acc;
                    v = acc;
                    const double a = fabs(acc);
                    if (a > m) m = a;
                }
            }
            if (!(m < 1e300)) return 0;                              /* unstable or NaN */
            if (m > env[k]) env[k] = m;
        }
    }
    double peak = 1.0;
    for (int k = 0; k < MAXC; k++) if (env[k] > peak) peak = env[k];
    int last_loud = -1;
    for (int k = 0; k < MAXC; k++) if (env[k] >= 1e-13 * peak) last_loud = k;
    if (last_loud >= MAXC - 2) return 0;                             /* still audible at the end of the probe */
    return last_loud + 2;                                            /* one chunk of margin */
}

/* May the pipelined kernel work in float32?  A rounding error e made at a section's output is filtered by the section's
 * own 1/A(z) before it reaches the next section, so float32 arithmetic adds noise of relative size eps32 * sqrt(sum g^2)
 * per section, g = impulse response of 1/A(z).  With eps32 = 6e-8 and at most 16 sections, sum g^2 <= 16 keeps the total
 * near 1e-6, a tenth of the 1e-5 tolerance (0.44-radius poles: 1.2; 0.9-radius: 30; 0.99-radius: 290 -> double).
 * Measured on each section's actual recurrence, not estimated from pole radii; anything that does not converge within
 * 4096 samples is left in double. */
static int iirm_float32_ok(const double *c5, int S)
{
    for (int s = 0; s < S; s++) {
        const double a1 = c5[5 * s + 3], a2 = c5[5 * s + 4];
        double y1 = 0.0, y2 = 0.0, energy = 0.0, tail = 0.0;
        for (int n = 0; n < 4096; n++) {
            const double y = (n == 0 ? 1.0 : 0.0) - a1 * y1 - a2 * y2;
            y2 = y1; y1 = y;
            energy += y * y;
            if (n >= 4096 - 64) tail += y * y;
        }
        if (!(energy <= 16.0) || !(tail <= 1e-20 * energy)) return 0;
        /* the feed-forward gain must not hide a cancellation either: |b| terms of ordinary size */
        if (!(fabs(c5[5 * s]) + fabs(c5[5 * s + 1]) + fabs(c5[5 * s + 2]) <= 64.0)) return 0;
    }
    return 1;
}

unsigned long llz_iir_cascade_mc_init(int channels, int stages, const double *coef)
{
    if (channels < 1 || stages < 1 || stages > 16 || !coef) {
        llzs_set_error("llz_iir_cascade_mc_init: channels %d stages %d (1..16)", channels, stages);
        return LLZ_BAD_HANDLE;
    }
    iirm_t *f = (iirm_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_IIRM;
    f->device = llzs_device_get();
    f->channels = channels; f->stages = stages;
    double *c5 = (double *)malloc(sizeof(double) * 5 * (size_t)stages);
    const size_t st_bytes = sizeof(double) * 4 * (size_t)stages * (size_t)channels;
    int rc = c5 ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        for (int s = 0; s < stages; s++) {                 /* {b0,b1,b2,a0,a1,a2} -> {b0,b1,b2,a1,a2}; a0 taken as 1 */
            c5[5 * s + 0] = coef[6 * s + 0]; c5[5 * s + 1] = coef[6 * s + 1]; c5[5 * s + 2] = coef[6 * s + 2];
            c5[5 * s + 3] = coef[6 * s + 4]; c5[5 * s + 4] = coef[6 * s + 5];
        }
        f->d_tab[f->ntab++] = llzs_malloc(sizeof(double) * 5 * (size_t)stages);
        f->d_coef = (const double *)f->d_tab[0];
        f->d_state = (double *)llzs_malloc(st_bytes);
        f->d_state_alt = (double *)llzs_malloc(st_bytes);
        if (!f->d_coef || !f->d_state || !f->d_state_alt) rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_tab[0], c5, sizeof(double) * 5 * (size_t)stages);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_state, 0, st_bytes, NULL);
    if (rc == LLZ_OK) f->float32_ok = iirm_float32_ok(c5, stages) && llzs_tune(LLZS_TUNE_IIR_F64) != 1;
    if (rc == LLZ_OK) rc = iirm_build_run16(f, c5);
    if (rc == LLZ_OK && llzs_tune(LLZS_TUNE_IIR_UNPACKED) < 1) rc = iirm_build_run32(f, c5);
    if (rc == LLZ_OK && llzs_tune(LLZS_TUNE_IIR_UNPACKED) < 1) rc = iirm_build_run32d(f, c5);
    if (rc == LLZ_OK) f->warm_chunks = iirm_memory_chunks(c5, stages);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    free(c5);
    if (rc != LLZ_OK) {
        iirm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

int llz_iir_cascade_mc_precision(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRM)) return LLZ_ERR_ARG;
    return ((iirm_t *)handle)->float32_ok ? 32 : 64;
}

void llz_iir_cascade_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRM)) {
        const int prev = llzs_device_enter(((iirm_t *)handle)->device);
        llzs_sync(((iirm_t *)handle)->stream);
        iirm_destroy((iirm_t *)handle);
        llzs_device_leave(prev);
    }
}

int llz_iir_cascade_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRM)) return LLZ_ERR_ARG;
    ((iirm_t *)handle)->stream = stream;
    return LLZ_OK;
}

static int iirm_process(iirm_t *f, const char *who, const float *x, float *y, int frame_len);

int llz_iir_cascade_mc(unsigned long handle, const float *x, float *y, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRM) || !x || !y || frame_len < 1) {
        llzs_set_error("llz_iir_cascade_mc: bad handle, buffer or frame_len");
        return LLZ_ERR_ARG;
    }
    iirm_t *f = (iirm_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = iirm_process(f, "llz_iir_cascade_mc", x, y, frame_len);
    llzs_device_leave(prev);
    return rc;
}

/* Which kernel takes the frame's whole chunks (n_fast samples): the stage pipeline, or for short-memory cascades of up to 8
 * sections a wave per (channel, time segment) with all sections in registers (float32, packed: 3.65 -> 2.3 ms on config 4;
 * double: 4.76 -> 3.75 ms on the 0.99-radius set).  That needs enough (channel, segment) items to fill most of the chip with
 * segments at least 8 x the warm-up long; measured crossover, tools/iir_xover.sh: 1024 items pipeline, 2048 items wave form.
 * Of the wave forms the one in the cascade's precision with 32 samples per lane (b0 folded out) where it was built and the
 * frame holds a 2048-sample chunk, else the one with 16. */
static int iirm_path(const iirm_t *f, int n_fast)
{
    const long seg_items = f->warm_chunks > 0 ? (long)f->channels * (n_fast / LLZS_IIR_PIPE_CHUNK / (8 * f->warm_chunks)) : 0;
    const int min_items = llzs_tune(LLZS_TUNE_IIR_WAVE_MIN_ITEMS) >= 0 ? llzs_tune(LLZS_TUNE_IIR_WAVE_MIN_ITEMS) : 2048;
    const int bank = f->tag == LLZ_TAG_IIRB;      /* its own 16-sample forms, and no 32-sample ones: wave[w32].pl stays NULL */
    const int w16 = f->float32_ok ? (bank ? LLZS_IIR_BANK16_F32 : LLZS_IIR_WAVE16_F32) : LLZS_IIR_WAVE16_F64;
    const int w32 = f->float32_ok ? LLZS_IIR_WAVE32_F32 : LLZS_IIR_WAVE32_F64;
    /* (a bank with a channel that never decays has no warm-up: the wave forms take none such, whatever the crossover is tuned to) */
    if (f->stages > 8 || seg_items < min_items || llzs_tune(LLZS_TUNE_IIR_PIPE) == 1 || !f->wave[w16].pl ||
        (bank && (f->warm_chunks < 1 || !f->float32_ok)))     /* a bank in double: the pipeline measured faster */
        return IIRM_PIPE;
    return (f->wave[w32].pl && n_fast >= LLZS_IIR_WAVE_CHUNK(w32)) ? w32 : w16;
}

/* The frame's main launch: the path's kernel and the samples it takes of the n_fast in whole 1024-sample chunks (a 32-sample
 * form: the whole 2048-sample chunks).  The call and the plan query both start here. */
static int iirm_main_launch(const iirm_t *f, int n_fast, int *n)
{
    const int path = iirm_path(f, n_fast);
    *n = LLZS_IIR_WAVE_IS32(path) ? n_fast - n_fast % LLZS_IIR_WAVE_CHUNK(path) : n_fast;
    return path;
}

/* the samples of a frame that whole 1024-sample chunks take, given rows the chunked kernels can read (16-byte aligned) */
static int iirm_fast_samples(int frame_len, int rows_aligned)
{
    return (rows_aligned && frame_len % 4 == 0) ? frame_len - frame_len % LLZS_IIR_PIPE_CHUNK : 0;
}

static int iirm_plan(const iirm_t *f, int frame_len, int out[5])
{
    int n = 0, p[3] = {0, 0, 0}, rc = LLZ_OK;
    const int path = iirm_main_launch(f, iirm_fast_samples(frame_len, 1), &n);
    if (n > 0) {
        const int prev = llzs_device_enter(f->device);      /* a wave form's first choice asks how many waves this chip holds */
        rc = llzs_iir_cascade_plan(path, f->channels, n, f->stages, f->warm_chunks, p);
        llzs_device_leave(prev);
    }
    out[0] = path == IIRM_PIPE ? LLZ_IIR_FORM_PIPE : LLZS_IIR_WAVE_IS32(path) ? LLZ_IIR_FORM_WAVE32 : LLZ_IIR_FORM_WAVE16;
    out[1] = f->float32_ok ? 32 : 64;
    out[2] = p[0]; out[3] = p[1]; out[4] = p[2];
    return rc;
}

int llz_iir_cascade_mc_plan(unsigned long handle, int frame_len, int out[5])
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRM) || !out || frame_len < 1) {
        llzs_set_error("llz_iir_cascade_mc_plan: bad handle, NULL out or frame_len");
        return LLZ_ERR_ARG;
    }
    return iirm_plan((const iirm_t *)handle, frame_len, out);
}

/* every launch reads d_state and writes d_state_alt (segments of one launch are not ordered), which then swap */
static int iirm_launch(iirm_t *f, int path, const float *d_in, float *d_out, int n, int pitch)
{
    const int bank = f->tag == LLZ_TAG_IIRB;
    const llzs_iir_wave_tables *pipe = &f->wave[LLZS_IIR_WAVE16_F64];     /* the pipeline's tables, shared or per channel */
    const int rc = path == IIRM_PIPE
        ? (bank ? llzs_iir_bank_pipe_f32 : llzs_iir_cascade_pipe_f32)(
              d_in, d_out, f->d_coef, (const double *)pipe->pd, (const double *)pipe->pl, f->d_state, f->d_state_alt,
              f->channels, n, pitch, pitch, f->stages, f->warm_chunks, f->float32_ok, f->stream)
        : llzs_iir_cascade_wave(path, &f->wave[path], d_in, d_out, f->d_state, f->d_state_alt, f->channels, n, pitch, pitch,
                                f->stages, f->warm_chunks, f->stream);
    if (rc == LLZ_OK) {
        double *t = f->d_state; f->d_state = f->d_state_alt; f->d_state_alt = t;
    }
    return rc;
}

static int iirm_process(iirm_t *f, const char *who, const float *x, float *y, int frame_len)
{
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len;
    const int in_dev = llzs_is_device_ptr(x), out_dev = llzs_is_device_ptr(y);
    if (in_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;            /* a buffer of another GPU: refused, message set */
    /* a later time segment reads its warm-up chunks from x while the segment before it writes them to y */
    if (llz_refuse_device_overlap(who, "x", x, bytes, in_dev, "y", y, bytes, out_dev)) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = llz_stage_in(&f->st_in, x, bytes, in_dev, f->stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, y, bytes, out_dev, &rc);
    /* whole 1024-sample chunks go through the path's kernel (needs 16-byte aligned rows): with a 32-sample form the whole
     * 2048-sample chunks, then its 16-sample counterpart what is left; the ragged remainder through the one-lane-per-channel
     * kernel.  All read and write the same per-section state. */
    const int n_fast = iirm_fast_samples(frame_len, ((size_t)d_in | (size_t)d_out) % 16 == 0);
    int main_n = 0, done = 0, path = iirm_main_launch(f, n_fast, &main_n);
    if (rc == LLZ_OK && LLZS_IIR_WAVE_IS32(path)) {
        done = main_n;
        rc = iirm_launch(f, path, d_in, d_out, done, frame_len);
        path = path == LLZS_IIR_WAVE32_F32 ? LLZS_IIR_WAVE16_F32 : LLZS_IIR_WAVE16_F64;
    }
    if (rc == LLZ_OK && n_fast > done) rc = iirm_launch(f, path, d_in + done, d_out + done, n_fast - done, frame_len);
    if (rc == LLZ_OK && n_fast < frame_len)
        rc = (f->tag == LLZ_TAG_IIRB ? llzs_iir_bank_f32 : llzs_iir_cascade_f32)(
                 d_in + n_fast, d_out + n_fast, f->d_coef, f->d_state, f->channels, frame_len - n_fast, frame_len, frame_len,
                 f->stages, f->stream);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(y, d_out, bytes, f->stream);
    return rc == LLZ_OK ? frame_len : rc;
}


/* ---- Part 4: the biquad bank: a coefficient set per channel (include/llz_iir.h).  An iirm_t with its own tag: staging, state
 * ping-pong, path choice, plan and process are the shared handle's; the tables hold a row per channel. ---- */

/* iirm_memory_chunks for a bank of many sets: the same number by less work.  For the plant in section s0 only the sections
 * s >= s0 are stepped (the earlier ones see zero input from zero state: their outputs are zeros, which neither raise a
 * maximum nor change a later section's sums).  And a plant's run ends once the state, i <= 1024 samples into a chunk, equals
 * bit for bit the state at the chunk's start: with zero input the cascade is a deterministic map of its state, so from
 * there on the outputs repeat with period i, the chunk's remaining samples and every later chunk (1024 >= i consecutive
 * samples: every phase) have exactly the maximum of these i samples.  That covers the state that has decayed to exactly
 * 0.0 (period 1, maximum 0) and the cycles among the smallest subnormals that round-to-nearest leaves a decaying section
 * in, where the plain probe spends the rest of its 64 chunks in subnormal arithmetic (0.17 s for 8 low-Q sections, 0.3 s
 * for 8 of radius 0.99).  All of it holds for finite coefficients only (0 x inf is not 0): any other set goes to the probe
 * itself. */
static int iirm_memory_chunks_bank(const double *c5, int S)
{
    enum { MAXC = 64, CH = 1024 };
    for (int i = 0; i < 5 * S; i++) if (!(fabs(c5[i]) < INFINITY)) return iirm_memory_chunks(c5, S);
    double env[MAXC];
    for (int k = 0; k < MAXC; k++) env[k] = 0.0;
    for (int s0 = 0; s0 < S; s0++) {
        double x1[16] = {0}, x2[16] = {0}, y1[16] = {0}, y2[16] = {0}, was[4][16];
        const size_t live = sizeof(double) * (size_t)(S - s0);
        y1[s0] = 1.0; y2[s0] = 1.0;
        for (int k = 0; k < MAXC; k++) {
            double m = 0.0;
            int repeats = 0;
            memcpy(was[0], x1, sizeof(x1)); memcpy(was[1], x2, sizeof(x2)); memcpy(was[2], y1, sizeof(y1)); memcpy(was[3], y2, sizeof(y2));
            for (int i = 0; i < CH && !repeats; i++) {
                double v = 0.0;
                for (int s = s0; s < S; s++) {
                    double acc = c5[5 * s] * v + c5[5 * s + 1] * x1[s] + c5[5 * s + 2] * x2[s]
                                 - c5[5 * s + 3] * y1[s] - c5[5 * s + 4] * y2[s];
                    x2[s] = x1[s]; x1[s] = v; y2[s] = y1[s]; y1[s] = acc;
                    v = acc;
                    const double a = fabs(acc);
                    if (a > m) m = a;
                }
                repeats = !memcmp(was[2] + s0, y1 + s0, live) && !memcmp(was[3] + s0, y2 + s0, live) &&
                          !memcmp(was[0] + s0, x1 + s0, live) && !memcmp(was[1] + s0, x2 + s0, live);
            }
            if (!(m < 1e300)) return 0;                              /* unstable */
            if (m > env[k]) env[k] = m;
            if (repeats) {
                for (int j = k + 1; j < MAXC; j++) if (m > env[j]) env[j] = m;
                break;
            }
        }
    }
    double peak = 1.0;
    for (int k = 0; k < MAXC; k++) if (env[k] > peak) peak = env[k];
    int last_loud = -1;
    for (int k = 0; k < MAXC; k++) if (env[k] >= 1e-13 * peak) last_loud = k;
    if (last_loud >= MAXC - 2) return 0;
    return last_loud + 2;
}

/* the two verdicts of channels [first, first + count), each distinct coefficient set examined once (equal rows are common
 * in a bank): an open-addressed table of the channels whose sets have been examined, keyed by the row's bytes */
static int iirb_verdicts(iirm_t *f, int first, int count)
{
    const size_t row = 5 * (size_t)f->stages;
    size_t cap = 16;
    while (cap < 2 * (size_t)count) cap *= 2;
    int *seen = (int *)malloc(sizeof(int) * cap);
    if (!seen) return LLZ_ERR_NOMEM;
    for (size_t i = 0; i < cap; i++) seen[i] = -1;
    for (int c = first; c < first + count; c++) {
        const double *c5 = f->h_c5 + row * (size_t)c;
        const unsigned char *b = (const unsigned char *)c5;
        unsigned long long h = 1469598103934665603ULL;                /* FNV-1a */
        for (size_t i = 0; i < row * sizeof(double); i++) h = (h ^ b[i]) * 1099511628211ULL;
        size_t at = (size_t)h & (cap - 1);
        while (seen[at] >= 0 && memcmp(f->h_c5 + row * (size_t)seen[at], c5, row * sizeof(double)) != 0) at = (at + 1) & (cap - 1);
        if (seen[at] >= 0) {
            f->h_f32ok[c] = f->h_f32ok[seen[at]]; f->h_warm[c] = f->h_warm[seen[at]];
        } else {
            seen[at] = c;
            f->h_f32ok[c] = (unsigned char)iirm_float32_ok(c5, f->stages);
            f->h_warm[c] = iirm_memory_chunks_bank(c5, f->stages);
        }
    }
    free(seen);
    return LLZ_OK;
}

/* the handle's precision and warm-up from the channels': float32 only if every set passes, the longest memory, and no split
 * along time at all if one channel's probe gave 0 */
static void iirb_handle_verdicts(iirm_t *f)
{
    int ok = llzs_tune(LLZS_TUNE_IIR_F64) != 1, warm = f->h_warm[0];
    for (int c = 0; c < f->channels; c++) {
        ok = ok && f->h_f32ok[c];
        if (warm > 0) warm = f->h_warm[c] == 0 ? 0 : (f->h_warm[c] > warm ? f->h_warm[c] : warm);
    }
    f->float32_ok = ok; f->warm_chunks = warm;
}

/* build the table rows of channels [first, first + count) with the shared handle's builder and copy them to the device,
 * ordered on the handle's stream; with32: the float tables too.  Batches of 16 channels bound the host buffer. */
static int iirb_upload_rows(iirm_t *f, int first, int count, int with32)
{
    enum { BATCH = 16 };
    const size_t S = (size_t)f->stages;
    double *pd = (double *)malloc(sizeof(double) * BATCH * S * (24 + 768));
    float *pd32 = (float *)malloc(sizeof(float) * BATCH * S * (16 + 768 + 24));
    int rc = (pd && pd32) ? LLZ_OK : LLZ_ERR_NOMEM;
    const llzs_iir_wave_tables *d = &f->wave[LLZS_IIR_WAVE16_F64], *d32 = &f->wave[LLZS_IIR_BANK16_F32];
    for (int c0 = first; c0 < first + count && rc == LLZ_OK; c0 += BATCH) {
        const size_t nb = (size_t)(first + count - c0 < BATCH ? first + count - c0 : BATCH);
        double *pl = pd + 24 * S * nb;
        float *pl32 = pd32 + 16 * S * nb, *ph32 = pl32 + 768 * S * nb;
        for (size_t k = 0; k < nb; k++)
            iirm_run16_rows(f->h_c5 + 5 * S * ((size_t)c0 + k), S, pd + 24 * S * k, pl + 768 * S * k, pd32 + 16 * S * k,
                            pl32 + 768 * S * k, ph32 + 24 * S * k);
        const size_t at = (size_t)c0 * S;
        rc = llzs_h2d((double *)f->d_coef + 5 * at, f->h_c5 + 5 * at, sizeof(double) * 5 * S * nb, f->stream);
        if (rc == LLZ_OK) rc = llzs_h2d((double *)d->pd + 24 * at, pd, sizeof(double) * 24 * S * nb, f->stream);
        if (rc == LLZ_OK) rc = llzs_h2d((double *)d->pl + 768 * at, pl, sizeof(double) * 768 * S * nb, f->stream);
        if (rc == LLZ_OK && with32) rc = llzs_h2d((float *)d32->pd + 16 * at, pd32, sizeof(float) * 16 * S * nb, f->stream);
        if (rc == LLZ_OK && with32) rc = llzs_h2d((float *)d32->pl + 768 * at, pl32, sizeof(float) * 768 * S * nb, f->stream);
        if (rc == LLZ_OK && with32) rc = llzs_h2d((float *)d32->cf + 24 * at, ph32, sizeof(float) * 24 * S * nb, f->stream);
    }
    free(pd); free(pd32);
    return rc;
}

/* the float tables exist once a float32 handle needs them; a handle in double keeps the double tables only */
static int iirb_alloc32(iirm_t *f)
{
    llzs_iir_wave_tables *d32 = &f->wave[LLZS_IIR_BANK16_F32];
    if (d32->pl) return LLZ_OK;
    const size_t rows = (size_t)f->channels * (size_t)f->stages;
    void *pd = llzs_malloc(sizeof(float) * 16 * rows), *pl = llzs_malloc(sizeof(float) * 768 * rows);
    void *cf = llzs_malloc(sizeof(float) * 24 * rows);
    if (!pd || !pl || !cf) {
        llzs_free(pd); llzs_free(pl); llzs_free(cf);
        return LLZ_ERR_NOMEM;
    }
    f->d_tab[f->ntab++] = pd; f->d_tab[f->ntab++] = pl; f->d_tab[f->ntab++] = cf;
    d32->pd = pd; d32->pl = pl; d32->cf = cf;
    return LLZ_OK;
}

/* after the verdicts of [first, first + count) changed: the rows given, or every row when the float tables have to be
 * (re)built because the handle is in float32 and they do not hold every channel's current set */
static int iirb_refresh(iirm_t *f, int first, int count)
{
    int rc = LLZ_OK;
    iirb_handle_verdicts(f);
    if (f->float32_ok && !f->f32_rows) {
        rc = iirb_alloc32(f);
        if (rc == LLZ_OK) rc = iirb_upload_rows(f, 0, f->channels, 1);
        f->f32_rows = rc == LLZ_OK;
    } else {
        rc = iirb_upload_rows(f, first, count, f->float32_ok);
        if (!f->float32_ok) f->f32_rows = 0;
    }
    return rc;
}

static void iirb_rows_from_coef(iirm_t *f, int first, int count, const double *coef)
{
    const size_t rows = (size_t)count * (size_t)f->stages;
    double *c5 = f->h_c5 + 5 * (size_t)first * (size_t)f->stages;
    for (size_t r = 0; r < rows; r++) {                    /* {b0,b1,b2,a0,a1,a2} -> {b0,b1,b2,a1,a2}; a0 taken as 1 */
        c5[5 * r + 0] = coef[6 * r + 0]; c5[5 * r + 1] = coef[6 * r + 1]; c5[5 * r + 2] = coef[6 * r + 2];
        c5[5 * r + 3] = coef[6 * r + 4]; c5[5 * r + 4] = coef[6 * r + 5];
    }
}

unsigned long llz_iir_bank_mc_init(int channels, int stages, const double *coef)
{
    if (channels < 1 || stages < 1 || stages > 16 || !coef) {
        llzs_set_error("llz_iir_bank_mc_init: channels %d (at least 1), stages %d (1..16) or NULL coef", channels, stages);
        return LLZ_BAD_HANDLE;
    }
    iirm_t *f = (iirm_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_IIRB;
    f->device = llzs_device_get();
    f->channels = channels; f->stages = stages;
    const size_t rows = (size_t)channels * (size_t)stages, st_bytes = sizeof(double) * 4 * rows;
    llzs_iir_wave_tables *d = &f->wave[LLZS_IIR_WAVE16_F64];
    f->h_c5 = (double *)malloc(sizeof(double) * 5 * rows);
    f->h_f32ok = (unsigned char *)malloc((size_t)channels);
    f->h_warm = (int *)malloc(sizeof(int) * (size_t)channels);
    int rc = (f->h_c5 && f->h_f32ok && f->h_warm) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {                                    /* the device first: without one, fail before the probes run */
        f->d_tab[f->ntab++] = llzs_malloc(sizeof(double) * 5 * rows);
        f->d_tab[f->ntab++] = llzs_malloc(sizeof(double) * 24 * rows);
        f->d_tab[f->ntab++] = llzs_malloc(sizeof(double) * 768 * rows);
        f->d_coef = (const double *)f->d_tab[0];
        d->cf = f->d_coef; d->pd = f->d_tab[1]; d->pl = f->d_tab[2];
        f->d_state = (double *)llzs_malloc(st_bytes);
        f->d_state_alt = (double *)llzs_malloc(st_bytes);
        if (!d->cf || !d->pd || !d->pl || !f->d_state || !f->d_state_alt) rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = llzs_memset(f->d_state, 0, st_bytes, NULL);
    if (rc == LLZ_OK) {
        iirb_rows_from_coef(f, 0, channels, coef);
        rc = iirb_verdicts(f, 0, channels);
    }
    if (rc == LLZ_OK) rc = iirb_refresh(f, 0, channels);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        iirm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_iir_bank_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB)) {
        const int prev = llzs_device_enter(((iirm_t *)handle)->device);
        llzs_sync(((iirm_t *)handle)->stream);
        iirm_destroy((iirm_t *)handle);
        llzs_device_leave(prev);
    }
}

int llz_iir_bank_mc(unsigned long handle, const float *x, float *y, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB) || !x || !y || frame_len < 1) {
        llzs_set_error("llz_iir_bank_mc: bad handle, buffer or frame_len");
        return LLZ_ERR_ARG;
    }
    iirm_t *f = (iirm_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = iirm_process(f, "llz_iir_bank_mc", x, y, frame_len);
    llzs_device_leave(prev);
    return rc;
}

int llz_iir_bank_mc_set_coef(unsigned long handle, int first, int count, const double *coef)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB) || !coef) {
        llzs_set_error("llz_iir_bank_mc_set_coef: bad handle or NULL coef");
        return LLZ_ERR_ARG;
    }
    iirm_t *f = (iirm_t *)handle;
    if (first < 0 || count < 1 || count > f->channels || first > f->channels - count) {
        llzs_set_error("llz_iir_bank_mc_set_coef: channels %d .. %d of a bank of %d", first, first + count - 1, f->channels);
        return LLZ_ERR_ARG;
    }
    /* the rows' host copies and verdicts as they were: a call that fails part-way puts them back, so that the handle's
     * precision and warm-up still describe sets it has run with (the device rows given may then hold either version) */
    const size_t row = sizeof(double) * 5 * (size_t)f->stages;
    double *was = (double *)malloc(row * (size_t)count + (sizeof(int) + 1) * (size_t)count);
    if (!was) {
        llzs_set_error("llz_iir_bank_mc_set_coef: out of host memory");
        return LLZ_ERR_NOMEM;
    }
    int *was_warm = (int *)((char *)was + row * (size_t)count);
    unsigned char *was_ok = (unsigned char *)(was_warm + count);
    memcpy(was, f->h_c5 + 5 * (size_t)f->stages * (size_t)first, row * (size_t)count);
    memcpy(was_warm, f->h_warm + first, sizeof(int) * (size_t)count);
    memcpy(was_ok, f->h_f32ok + first, (size_t)count);
    const int prev = llzs_device_enter(f->device);
    iirb_rows_from_coef(f, first, count, coef);
    int rc = iirb_verdicts(f, first, count);
    if (rc == LLZ_OK) rc = iirb_refresh(f, first, count);
    if (rc != LLZ_OK) {
        memcpy(f->h_c5 + 5 * (size_t)f->stages * (size_t)first, was, row * (size_t)count);
        memcpy(f->h_warm + first, was_warm, sizeof(int) * (size_t)count);
        memcpy(f->h_f32ok + first, was_ok, (size_t)count);
        iirb_handle_verdicts(f);
        f->f32_rows = 0;                                    /* the next successful call rebuilds every float row */
    }
    llzs_device_leave(prev);
    free(was);
    return rc;
}

int llz_iir_bank_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB)) {
        llzs_set_error("llz_iir_bank_mc_set_stream: bad handle");
        return LLZ_ERR_ARG;
    }
    ((iirm_t *)handle)->stream = stream;
    return LLZ_OK;
}

int llz_iir_bank_mc_precision(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB)) {
        llzs_set_error("llz_iir_bank_mc_precision: bad handle");
        return LLZ_ERR_ARG;
    }
    return ((iirm_t *)handle)->float32_ok ? 32 : 64;
}

int llz_iir_bank_mc_plan(unsigned long handle, int frame_len, int out[5])
{
    if (!LLZ_HANDLE_OK(handle, iirm_t, LLZ_TAG_IIRB) || !out || frame_len < 1) {
        llzs_set_error("llz_iir_bank_mc_plan: bad handle, NULL out or frame_len");
        return LLZ_ERR_ARG;
    }
    return iirm_plan((const iirm_t *)handle, frame_len, out);
}


/* =====================================================================================================
 * Part 3: multi-channel GENERAL direct form I (any orders M, N up to llzs_iir_df1_mc_max_order()): the batch form of
 * llz_iir_filter itself (reference llz_iir.c:103-156), float32 in / out, double arithmetic in the reference's order.
 * ===================================================================================================== */
#define LLZ_TAG_IIRG 0x4c5a4947

typedef struct {
    int tag, device, channels, M, N, ord;
    int warm;                       /* samples after which the filter has forgotten its state to 1e-13 (0: never split time) */
    double *d_ab;                   /* a[0..ord], b[0..ord], zero padded */
    double *d_state[2];             /* [channels][2][ord + 1] delay lines, ping-pong */
    int cur;
    float *d_zero;                  /* N zeros per channel for the flush */
    llz_stage_t st_in, st_out;
    void *stream;
} iirg_t;

static void iirg_destroy(iirg_t *f)
{
    if (!f) return;
    llzs_free(f->d_ab); llzs_free(f->d_state[0]); llzs_free(f->d_state[1]); llzs_free(f->d_zero);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->tag = 0;
    free(f);
}

/* how long the recurrence remembers: run 1/A(z) on the host from the worst unit state (every y delay = 1) with zero input
 * and find the last sample whose magnitude exceeds 1e-13 of the largest seen; 0 when it has not died out within `limit` */
static int iirg_probe_memory(int M, const double *a, int limit)
{
    if (M == 0) return 1;
    double y[64];
    for (int k = 0; k < M; k++) y[k] = 1.0;
    double peak = 1.0;
    int last = 0;
    for (int t = 0; t < limit; t++) {
        double acc = 0.0;
        for (int k = 1; k <= M; k++) acc -= a[k] * y[k - 1];
        for (int k = M - 1; k >= 1; k--) y[k] = y[k - 1];
        y[0] = acc;
        const double m = fabs(acc);
        if (!(m < 1e300)) return 0;                                 /* unstable */
        if (m > peak) peak = m;
        if (m > 1e-13 * peak) last = t;
    }
    return last < limit - limit / 8 ? last + 1 : 0;
}

unsigned long llz_iir_mc_init(int channels, int M, const double *a, int N, const double *b)
{
    const int ord = llzs_iir_df1_mc_max_order();
    if (channels < 1 || M < 0 || N < 0 || M > ord || N > ord || !a) {
        llzs_set_error("llz_iir_mc_init: channels %d M %d N %d (orders 0..%d) or NULL a", channels, M, N, ord);
        return LLZ_BAD_HANDLE;
    }
    iirg_t *f = (iirg_t *)calloc(1, sizeof(*f));
    double *ab = (double *)calloc(2 * ((size_t)ord + 1), sizeof(double));
    int rc = (f && ab) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        f->tag = LLZ_TAG_IIRG; f->device = llzs_device_get(); f->channels = channels; f->M = M; f->N = N; f->ord = ord;
        for (int k = 0; k <= M; k++) ab[k] = a[k];
        for (int k = 0; b && k <= N; k++) ab[ord + 1 + k] = b[k];                  /* b == NULL -> zeros (llz_iir.c:54-59) */
        const int mem = iirg_probe_memory(M, a, 1 << 16);
        f->warm = mem ? mem + N : 0;
        const size_t sbytes = sizeof(double) * (size_t)channels * 2 * ((size_t)ord + 1);
        f->d_ab = (double *)llzs_malloc(sizeof(double) * 2 * ((size_t)ord + 1));
        f->d_state[0] = (double *)llzs_malloc(sbytes);
        f->d_state[1] = (double *)llzs_malloc(sbytes);
        f->d_zero = (float *)llzs_malloc(sizeof(float) * (size_t)channels * (size_t)(N > 0 ? N : 1));
        if (!f->d_ab || !f->d_state[0] || !f->d_state[1] || !f->d_zero || f->device < 0) rc = LLZ_ERR_NOMEM;
        if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_ab, ab, sizeof(double) * 2 * ((size_t)ord + 1));
        if (rc == LLZ_OK) rc = llzs_memset(f->d_state[0], 0, sbytes, NULL);
        if (rc == LLZ_OK) rc = llzs_memset(f->d_state[1], 0, sbytes, NULL);
        if (rc == LLZ_OK) rc = llzs_memset(f->d_zero, 0, sizeof(float) * (size_t)channels * (size_t)(N > 0 ? N : 1), NULL);
        if (rc == LLZ_OK) rc = llzs_sync(NULL);
    }
    free(ab);
    if (rc != LLZ_OK) {
        if (f && f->tag) iirg_destroy(f); else free(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_iir_mc_uninit(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, iirg_t, LLZ_TAG_IIRG)) return;
    iirg_t *f = (iirg_t *)handle;
    const int prev = llzs_device_enter(f->device);
    llzs_sync(f->stream);
    iirg_destroy(f);
    llzs_device_leave(prev);
}

int llz_iir_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, iirg_t, LLZ_TAG_IIRG)) return LLZ_ERR_ARG;
    ((iirg_t *)handle)->stream = stream;
    return LLZ_OK;
}

/* time segments of an n-sample launch: enough (channel, segment) lanes to fill the chip (~64 K), each at least 8 x the filter's
 * memory long; what the launcher is asked for */
static int iirg_segs(const iirg_t *f, int n)
{
    int segs = 1;
    if (f->warm > 0) {
        const int tune = llzs_tune(LLZS_TUNE_IIR_SEGS);
        const long want = tune > 0 ? tune : (65536 + f->channels - 1) / f->channels;
        const long most = (long)n / (8L * f->warm);
        segs = (int)(want < most ? want : most);
        if (segs < 1) segs = 1;
    }
    return segs;
}

int llz_iir_mc_segments(unsigned long handle, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, iirg_t, LLZ_TAG_IIRG) || frame_len < 1) {
        llzs_set_error("llz_iir_mc_segments: bad handle or frame_len %d", frame_len);
        return LLZ_ERR_ARG;
    }
    const iirg_t *f = (const iirg_t *)handle;
    return llzs_iir_df1_mc_segments(frame_len, iirg_segs(f, frame_len), f->warm);     /* the launcher's own last word */
}

static int iirg_launch(iirg_t *f, const float *d_in, float *d_out, int n)
{
    const int segs = iirg_segs(f, n);
    const int rc = llzs_iir_df1_mc_f32(d_in, d_out, f->d_ab, f->d_state[f->cur], f->d_state[f->cur ^ 1], f->channels, n, n, n,
                                       f->M, f->N, segs, f->warm, f->stream);
    if (rc == LLZ_OK) f->cur ^= 1;
    return rc;
}

int llz_iir_mc(unsigned long handle, const float *x, float *y, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, iirg_t, LLZ_TAG_IIRG) || !x || !y || frame_len < 1 || x == y) {
        llzs_set_error("llz_iir_mc: bad handle, NULL buffer, in-place call or frame_len %d", frame_len);
        return LLZ_ERR_ARG;
    }
    iirg_t *f = (iirg_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len;
    const int in_dev = llzs_is_device_ptr(x), out_dev = llzs_is_device_ptr(y);
    int rc = (in_dev < 0 || out_dev < 0) ? LLZ_ERR_ARG : LLZ_OK;
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap("llz_iir_mc", "x", x, bytes, in_dev, "y", y, bytes, out_dev);
    const float *d_in = llz_stage_in(&f->st_in, x, bytes, in_dev, f->stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, y, bytes, out_dev, &rc);
    if (rc == LLZ_OK) rc = iirg_launch(f, d_in, d_out, frame_len);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(y, d_out, bytes, f->stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frame_len : rc;
}

/* N more samples of x = 0 per channel (llz_iir.c:147-156); returns N */
int llz_iir_mc_flush(unsigned long handle, float *y)
{
    if (!LLZ_HANDLE_OK(handle, iirg_t, LLZ_TAG_IIRG) || !y) {
        llzs_set_error("llz_iir_mc_flush: bad handle or buffer");
        return LLZ_ERR_ARG;
    }
    iirg_t *f = (iirg_t *)handle;
    if (f->N == 0) return 0;
    const int prev = llzs_device_enter(f->device);
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)f->N;
    const int out_dev = llzs_is_device_ptr(y);
    int rc = out_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;
    float *d_out = llz_stage_out(&f->st_out, y, bytes, out_dev, &rc);
    if (rc == LLZ_OK) rc = iirg_launch(f, f->d_zero, d_out, f->N);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(y, d_out, bytes, f->stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? f->N : rc;
}
