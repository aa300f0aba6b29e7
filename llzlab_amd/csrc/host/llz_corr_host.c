/*
 * llz_corr_host.c -- handle layer of the correlation functions: the reference's symbols
 * (reference libllzfilter/llz_corr.c:38-177) and the float32 batch extension.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_corr.h"
#include "../../../include/llz_fft.h"
#include "llz_host.h"

/* ---- Part 1: reference symbols, exact order on the device ---- */

static void corr_exact(const double *x, const double *y, int n, int p, double *r, const char *who)
{
    if (!x || !y || !r || n < 1 || p < 0) {
        llzs_set_error("%s: bad arguments", who);
        return;                                                     /* void in the reference ABI */
    }
    const size_t nb = sizeof(double) * (size_t)n, rb = sizeof(double) * ((size_t)p + 1);
    double *d_x = (double *)llzs_malloc(nb);
    double *d_y = (x == y) ? d_x : (double *)llzs_malloc(nb);
    double *d_r = (double *)llzs_malloc(rb);
    if (d_x && d_y && d_r && llzs_h2d(d_x, x, nb, NULL) == LLZ_OK &&
        (x == y || llzs_h2d(d_y, y, nb, NULL) == LLZ_OK) &&
        llzs_corr_exact_f64(d_x, d_y, n, p, d_r, NULL) == LLZ_OK)
        (void)llzs_d2h(r, d_r, rb, NULL);
    if (d_y != d_x) llzs_free(d_y);
    llzs_free(d_x);
    llzs_free(d_r);
}

void llz_autocorr(double *x, int n, int p, double *r) { corr_exact(x, x, n, p, r, "llz_autocorr"); }

void llz_crosscorr(double *x, double *y, int n, int p, double *r) { corr_exact(x, y, n, p, r, "llz_crosscorr"); }

double llz_corr_cof(double *a, double *b, int len)
{
    /* the three running sums of llz_corr.c:70-74 are lag-0 correlations; the final division and square root run on
     * the host's libm exactly as in the reference */
    double ab = 0, aa = 0, bb = 0;
    corr_exact(a, b, len, 0, &ab, "llz_corr_cof");
    corr_exact(a, a, len, 0, &aa, "llz_corr_cof");
    corr_exact(b, b, len, 0, &bb, "llz_corr_cof");
    return ab / sqrt(aa * bb);
}

typedef struct {
    llz_head_t head;            /* no device memory of its own: the llz_fft handle's */
    int n, fft_len;
    unsigned long h_fft;
    double *b1, *b2;
} acf1_t;

#define LLZ_TAG_ACF1 0x4c5a4131
#define LLZ_TAG_ACFM 0x4c5a414d
#define LLZ_TAG_XCFM 0x4c5a584d

static int acf_fft_len(int n)
{
    int level = (int)log2((double)(2 * n));                        /* llz_corr.c:81-93, 106 */
    if ((1 << level) < 2 * n) level += 1;
    return 1 << level;
}

unsigned long llz_autocorr_fast_init(int n)
{
    if (n < 1 || acf_fft_len(n) > 4096) {
        llzs_set_error("llz_autocorr_fast_init: n=%d (1..2048)", n);
        return LLZ_BAD_HANDLE;
    }
    acf1_t *f = (acf1_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ACF1, 0);
    if (!f) return LLZ_BAD_HANDLE;
    f->n = n; f->fft_len = acf_fft_len(n);
    f->h_fft = llz_fft_init(f->fft_len);
    f->b1 = (double *)calloc(2 * (size_t)f->fft_len, sizeof(double));
    f->b2 = (double *)calloc(2 * (size_t)f->fft_len, sizeof(double));
    if (f->h_fft == LLZ_BAD_HANDLE || !f->b1 || !f->b2) {
        if (f->h_fft != LLZ_BAD_HANDLE) llz_fft_uninit(f->h_fft);
        free(f->b1); free(f->b2); free(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_autocorr_fast_uninit(unsigned long handle)
{
    acf1_t *f = (acf1_t *)llz_handle(handle, LLZ_TAG_ACF1, NULL);
    if (!f) return;
    llz_fft_uninit(f->h_fft);
    free(f->b1); free(f->b2);
    f->head.tag = 0;
    free(f);
}

void llz_autocorr_fast(unsigned long handle, double *x, int n, int p, double *r)
{
    acf1_t *f = (acf1_t *)llz_handle(handle, LLZ_TAG_ACF1, NULL);
    if (!f || !x || !r || n < 1 || p < 0) {
        llzs_set_error("llz_autocorr_fast: bad handle or arguments");
        return;
    }
    if (n > f->fft_len / 2 || p >= f->fft_len) {
        llzs_set_error("llz_autocorr_fast: n=%d / p=%d do not fit fft_len %d", n, p, f->fft_len);
        return;
    }
    /* llz_corr.c:155-177 with both transforms on the device (exact-order double FFT): same bits as the reference */
    memset(f->b1, 0, sizeof(double) * 2 * (size_t)f->fft_len);
    for (int i = 0; i < n; i++) f->b1[2 * i] = x[i];
    llz_fft(f->h_fft, f->b1);
    memset(f->b2, 0, sizeof(double) * 2 * (size_t)f->fft_len);
    for (int i = 0; i < n; i++)                                     /* only the first n bins: the reference's quirk */
        f->b2[2 * i] = f->b1[2 * i] * f->b1[2 * i] + f->b1[2 * i + 1] * f->b1[2 * i + 1];
    llz_ifft(f->h_fft, f->b2);
    for (int i = 0; i <= p; i++) r[i] = f->b2[2 * i] * 2;
}

/* ---- Part 2: batch extension ---- */

int llz_autocorr_mc(const float *x, float *r, int frames, int n, int p, void *stream)
{
    if (!x || !r || frames < 1 || n < 1 || p < 0 || p >= n || p > 255) {
        llzs_set_error("llz_autocorr_mc: frames %d n %d p %d (p < n, p <= 255)", frames, n, p);
        return LLZ_ERR_ARG;
    }
    const size_t xb = sizeof(float) * (size_t)frames * n, rb = sizeof(float) * (size_t)frames * (p + 1);
    llz_bind_t b[2] = {{"x", x, xb, LLZ_BIND_IN, NULL, 0, 0}, {"r", r, rb, LLZ_BIND_OUT, NULL, 0, 0}};
    int rc = llz_bind("llz_autocorr_mc", b, 2, stream);
    if (rc == LLZ_OK) rc = llzs_autocorr_mc_f32((const float *)b[0].dev, (float *)b[1].dev, frames, n, p, stream);
    return llz_bind_finish(b, 2, stream, rc);
}

int llz_crosscorr_mc(const float *x, const float *y, float *r, int frames, int n, int p, int two_sided, void *stream)
{
    if (!x || !y || !r || frames < 1 || n < 1 || p < 0 || p >= n || p > 255 || (two_sided != 0 && two_sided != 1)) {
        llzs_set_error("llz_crosscorr_mc: x %p y %p r %p frames %d n %d p %d two_sided %d (p < n, p <= 255, two_sided 0 or 1)",
                       (const void *)x, (const void *)y, (void *)r, frames, n, p, two_sided);
        return LLZ_ERR_ARG;
    }
    const size_t xb = sizeof(float) * (size_t)frames * n;
    const size_t rb = sizeof(float) * (size_t)frames * (two_sided ? 2 * (size_t)p + 1 : (size_t)p + 1);
    llz_bind_t b[3] = {{"x", x, xb, LLZ_BIND_IN, NULL, 0, 0}, {"y", y, xb, LLZ_BIND_IN, NULL, 0, 0},
                       {"r", r, rb, LLZ_BIND_OUT, NULL, 0, 0}};
    int rc = llz_bind("llz_crosscorr_mc", b, 3, stream);
    if (rc == LLZ_OK)
        rc = llzs_crosscorr_mc_f32((const float *)b[0].dev, (const float *)b[1].dev, (float *)b[2].dev, frames, n, p, two_sided,
                                   stream);
    return llz_bind_finish(b, 3, stream, rc);
}

int llz_corr_cof_mc(const float *a, const float *b, float *c, int frames, int n, void *stream)
{
    if (!a || !b || !c || frames < 1 || n < 1) {
        llzs_set_error("llz_corr_cof_mc: a %p b %p c %p frames %d n %d", (const void *)a, (const void *)b, (void *)c, frames, n);
        return LLZ_ERR_ARG;
    }
    const size_t ab = sizeof(float) * (size_t)frames * n, cb = sizeof(float) * (size_t)frames;
    llz_bind_t v[3] = {{"a", a, ab, LLZ_BIND_IN, NULL, 0, 0}, {"b", b, ab, LLZ_BIND_IN, NULL, 0, 0},
                       {"c", c, cb, LLZ_BIND_OUT, NULL, 0, 0}};
    int rc = llz_bind("llz_corr_cof_mc", v, 3, stream);
    if (rc == LLZ_OK) rc = llzs_corr_cof_mc_f32((const float *)v[0].dev, (const float *)v[1].dev, (float *)v[2].dev, frames, n, stream);
    return llz_bind_finish(v, 3, stream, rc);
}

typedef struct {
    llz_head_t head;
    int frames, n, fft_len;
    float *d_cs;            /* fft_len cos then fft_len sin */
    llz_stage_t st_in, st_out;
} acfm_t;

static void acfm_destroy(void *p)
{
    acfm_t *f = (acfm_t *)p;
    llzs_free(f->d_cs);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_autocorr_fast_mc_init(int frames, int n)
{
    if (frames < 1 || n < 1 || acf_fft_len(n) > 4096 || acf_fft_len(n) < 8) {
        llzs_set_error("llz_autocorr_fast_mc_init: frames %d n %d (4..2048)", frames, n);
        return LLZ_BAD_HANDLE;
    }
    acfm_t *f = (acfm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ACFM, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->frames = frames; f->n = n; f->fft_len = acf_fft_len(n);
    f->d_cs = llz_host_cs_f32(f->fft_len);
    if (!f->d_cs) {
        acfm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_autocorr_fast_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_ACFM, acfm_destroy); }

int llz_autocorr_fast_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_ACFM, "llz_autocorr_fast_mc_set_stream", stream);
}

int llz_autocorr_fast_mc(unsigned long handle, const float *x, float *r, int p)
{
    acfm_t *f = (acfm_t *)llz_handle(handle, LLZ_TAG_ACFM, NULL);
    if (!f || !x || !r || p < 0) {
        llzs_set_error("llz_autocorr_fast_mc: bad handle or arguments");
        return LLZ_ERR_ARG;
    }
    if (p >= f->fft_len) {
        llzs_set_error("llz_autocorr_fast_mc: p=%d >= fft_len %d", p, f->fft_len);
        return LLZ_ERR_ARG;
    }
    const size_t xb = sizeof(float) * (size_t)f->frames * f->n, rb = sizeof(float) * (size_t)f->frames * (p + 1);
    const int prev = llzs_device_enter(f->head.device);
    const int x_dev = llzs_is_device_ptr(x), r_dev = llzs_is_device_ptr(r);
    int rc = (x_dev < 0 || r_dev < 0) ? LLZ_ERR_ARG : LLZ_OK;     /* a buffer of another GPU: refused, message set */
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap("llz_autocorr_fast_mc", "x", x, xb, x_dev, "r", r, rb, r_dev);
    const float *d_x = llz_stage_in(&f->st_in, x, xb, x_dev, f->head.stream, &rc);
    float *d_r = llz_stage_out(&f->st_out, r, rb, r_dev, &rc);
    /* pack -> FFT -> |X|^2 (first n bins) -> IFFT -> 2 Re, fused in LDS */
    if (rc == LLZ_OK) rc = llzs_acf_fused_f32(d_x, d_r, f->frames, f->n, p, f->fft_len, f->d_cs, f->head.stream);
    if (rc == LLZ_OK && !r_dev) rc = llzs_d2h(r, d_r, rb, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

/* ---- FFT cross-correlation: z = x + i y through ONE forward transform per frame pair, conj(X) Y, one inverse ---- */

#define XCF_SCRATCH_BYTES ((size_t)256 << 20)      /* spectra scratch: at most this much, walked in slabs of frames */

typedef struct {
    llz_head_t head;
    int frames, n, fft_len, slab;                   /* slab: frames per walk of the scratch */
    float *d_cs;            /* fft_len cos then fft_len sin */
    float *d_z;             /* slab x fft_len complex */
    llz_stage_t st_x, st_y, st_out;
} xcfm_t;

static void xcfm_destroy(void *p)
{
    xcfm_t *f = (xcfm_t *)p;
    llzs_free(f->d_cs);
    llzs_free(f->d_z);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_y); llz_stage_release(&f->st_out);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_crosscorr_fast_mc_init(int frames, int n)
{
    if (frames < 1 || n < 4 || n > 2048) {
        llzs_set_error("llz_crosscorr_fast_mc_init: frames %d n %d (frames >= 1, n in 4..2048)", frames, n);
        return LLZ_BAD_HANDLE;
    }
    xcfm_t *f = (xcfm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_XCFM, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->frames = frames; f->n = n; f->fft_len = acf_fft_len(n);
    const size_t per_frame = sizeof(float) * 2 * (size_t)f->fft_len;
    f->slab = (size_t)frames * per_frame <= XCF_SCRATCH_BYTES ? frames : (int)(XCF_SCRATCH_BYTES / per_frame);
    f->d_cs = llz_host_cs_f32(f->fft_len);
    if (f->d_cs) f->d_z = (float *)llzs_malloc((size_t)f->slab * per_frame);
    if (!f->d_z) {
        xcfm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_crosscorr_fast_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_XCFM, xcfm_destroy); }

int llz_crosscorr_fast_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_XCFM, "llz_crosscorr_fast_mc_set_stream", stream);
}

int llz_crosscorr_fast_mc(unsigned long handle, const float *x, const float *y, float *r, int p, int two_sided)
{
    xcfm_t *f = (xcfm_t *)llz_handle(handle, LLZ_TAG_XCFM, "llz_crosscorr_fast_mc");
    if (!f) return LLZ_ERR_ARG;
    if (!x || !y || !r || p < 0 || p >= f->n || (two_sided != 0 && two_sided != 1)) {
        llzs_set_error("llz_crosscorr_fast_mc: x %p y %p r %p p %d two_sided %d (0 <= p < n = %d, two_sided 0 or 1)",
                       (const void *)x, (const void *)y, (void *)r, p, two_sided, f->n);
        return LLZ_ERR_ARG;
    }
    const int width = two_sided ? 2 * p + 1 : p + 1, F = f->fft_len;
    const size_t xb = sizeof(float) * (size_t)f->frames * f->n, rb = sizeof(float) * (size_t)f->frames * width;
    const int prev = llzs_device_enter(f->head.device);
    const int x_dev = llzs_is_device_ptr(x), y_dev = llzs_is_device_ptr(y), r_dev = llzs_is_device_ptr(r);
    int rc = (x_dev < 0 || y_dev < 0 || r_dev < 0) ? LLZ_ERR_ARG : LLZ_OK;   /* a buffer of another GPU: refused, message set */
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap("llz_crosscorr_fast_mc", "x", x, xb, x_dev, "r", r, rb, r_dev);
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap("llz_crosscorr_fast_mc", "y", y, xb, y_dev, "r", r, rb, r_dev);
    const float *d_x = llz_stage_in(&f->st_x, x, xb, x_dev, f->head.stream, &rc);
    /* an autocorrelation from host memory (y == x) is staged once */
    const float *d_y = y == x ? d_x : llz_stage_in(&f->st_y, y, xb, y_dev, f->head.stream, &rc);
    float *d_r = llz_stage_out(&f->st_out, r, rb, r_dev, &rc);
    /* per slab of frames: pack -> FFT -> conj(X) Y -> IFFT -> lags; the launches of a slab follow the previous slab's on the stream */
    for (int f0 = 0; rc == LLZ_OK && f0 < f->frames; f0 += f->slab) {
        const int cnt = f->frames - f0 < f->slab ? f->frames - f0 : f->slab;
        rc = llzs_xcf_pack(d_x + (size_t)f0 * f->n, d_y + (size_t)f0 * f->n, f->d_z, cnt, f->n, F, f->head.stream);
        if (rc == LLZ_OK) rc = llzs_fft_f32(f->d_z, cnt, F, f->d_cs, 0, f->head.stream);
        if (rc == LLZ_OK) rc = llzs_xcf_product(f->d_z, cnt, F, f->head.stream);
        if (rc == LLZ_OK) rc = llzs_fft_f32(f->d_z, cnt, F, f->d_cs, 1, f->head.stream);
        if (rc == LLZ_OK) rc = llzs_xcf_extract(f->d_z, d_r + (size_t)f0 * width, cnt, p, two_sided, F, f->head.stream);
    }
    if (rc == LLZ_OK && !r_dev) rc = llzs_d2h(r, d_r, rb, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}
