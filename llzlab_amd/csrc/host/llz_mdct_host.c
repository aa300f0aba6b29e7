/*
 * llz_mdct_host.c -- handle layer of the MDCT: the reference's symbols
 * (reference libllzfilter/llz_mdct.c:97-620) and the float32 batch extension.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_mdct.h"
#include "llz_host.h"

#define LLZ_TAG_MDCT 0x4c5a4d31
#define LLZ_TAG_MDCB 0x4c5a4d42

/* ---- windows (host, llz_mdct.c:97-182) ---- */

int llz_mdct_sine(double *w, int N)
{
    for (int n = 0; n < N; n++) {
        const double tmp = (M_PI / N) * (n + 0.5);
        w[n] = sin(tmp);
    }
    return N;
}

static double mdct_bessel(double x)
{
    double xh = (double)0.5 * x, sum = 1.0, pw = 1.0, ds = 1.0;
    int k = 0;
    while (ds > sum * 1E-16) {
        ++k;
        pw = pw * (xh / k);
        ds = pw * pw;
        sum = sum + ds;
    }
    return sum;
}

int llz_mdct_kbd(double *w, int N, double alpha)
{
    const int N2 = N >> 1, K = N2 + 1;
    double *w1 = (double *)malloc(sizeof(double) * (size_t)K);
    if (!w1) return -1;
    const double beta = alpha * M_PI;
    for (int i = 0; i < K; i++) {                                   /* kaiser_beta(w1, N2+1, alpha*pi) */
        const double Ib = mdct_bessel(beta);
        const double x = (double)((2. * i / (K - 1)) - 1);
        const double Ia = mdct_bessel(beta * (double)sqrt(1. - x * x));
        w1[i] = (double)(Ia / Ib);
    }
    double sum = 0.0, tmp = 0.0;
    for (int i = 0; i < K; i++) sum += w1[i];
    sum = 1.0 / sum;
    for (int i = 0, j = N - 1; i < N2; i++, j--) {
        tmp += w1[i];
        w[i] = w[j] = sqrt(tmp * sum);
    }
    free(w1);
    return N;
}

/* ---- Part 1: reference symbols ----
 * All three algorithms of llz_mdct.c run on the device in the reference's rounding order.  A frame travels host -> device
 * once, goes through (twiddle step, exact-order transform, twiddle step) or the defining sums, and comes back once; the
 * host only builds the angle tables (llz_tables.c: libm, the reference's angle expressions, so that the table values are the
 * reference's to the last bit) and moves the frame. */

typedef struct {
    llz_head_t head;
    int form, length;               /* form: MDCT_ORIGIN (defining sums), MDCT_FFT (N-point), MDCT_FFT4 (N/4-point) */
    int fft_size;                   /* points of the transform inside the FFT forms */
    double norm;                    /* 1 / sqrt(length): the N/4-point form's inverse scale */
    double *d_sum_fwd, *d_sum_inv;  /* MDCT_ORIGIN: [N/2][N] and [N][N/2] cosine kernels */
    double *d_rot[4];               /* FFT forms: (cos, sin) pair tables of the four twiddle steps */
    double *d_fft_cs;               /* fft_size cos then fft_size sin of 2 pi i / fft_size (llz_fft.c:222-229) */
    double *d_frame, *d_bins, *d_work;   /* N time samples, N/2 coefficients, up to N complex points */
} mdct1_t;

static void mdct1_destroy(void *p)
{
    mdct1_t *f = (mdct1_t *)p;
    llzs_free(f->d_sum_fwd); llzs_free(f->d_sum_inv);
    for (int t = 0; t < 4; t++) {
        int shared = 0;
        for (int u = 0; u < t; u++) shared |= (f->d_rot[u] == f->d_rot[t]);
        if (!shared) llzs_free(f->d_rot[t]);
    }
    llzs_free(f->d_fft_cs); llzs_free(f->d_frame); llzs_free(f->d_bins); llzs_free(f->d_work);
    f->head.tag = 0;
    free(f);
}

static int mdct1_build_fft_form(mdct1_t *f)
{
    const int N = f->length;
    f->fft_size = f->form == MDCT_FFT ? N : N >> 2;
    if (f->form == MDCT_FFT) {
        f->d_rot[LLZ_ROT_FWD_PRE] = llz_host_mdct_rot_f64(0, LLZ_ROT_FWD_PRE, N, N);
        f->d_rot[LLZ_ROT_FWD_POST] = llz_host_mdct_rot_f64(0, LLZ_ROT_FWD_POST, N >> 1, N);
        f->d_rot[LLZ_ROT_INV_PRE] = llz_host_mdct_rot_f64(0, LLZ_ROT_INV_PRE, N, N);
        f->d_rot[LLZ_ROT_INV_POST] = llz_host_mdct_rot_f64(0, LLZ_ROT_INV_POST, N, N);
    } else {
        double *t = llz_host_mdct_rot_f64(1, 0, N >> 2, N);             /* one table serves all four steps */
        for (int s = 0; s < 4; s++) f->d_rot[s] = t;
        f->norm = 1. / sqrt(N);
    }
    for (int s = 0; s < 4; s++)
        if (!f->d_rot[s]) return LLZ_ERR_NOMEM;
    f->d_fft_cs = llz_host_cs_f64(f->fft_size);
    f->d_work = (double *)llzs_malloc(sizeof(double) * 2 * (size_t)f->fft_size);
    return f->d_fft_cs && f->d_work ? LLZ_OK : LLZ_ERR_NOMEM;
}

unsigned long llz_mdct_init(int type, int size)
{
    if (size < 4 || (type != MDCT_ORIGIN && type != MDCT_FFT && type != MDCT_FFT4)) {
        llzs_set_error("llz_mdct_init: type %d len %d", type, size);
        return LLZ_BAD_HANDLE;
    }
    int log2len = (int)(log(size) / log(2));                        /* next power of two, as llz_mdct.c:375-379 */
    if ((1 << log2len) < size) log2len += 1;
    const int length = 1 << log2len;
    const int limit = type == MDCT_ORIGIN ? 2048 : (type == MDCT_FFT ? 4096 : 16384);
    if (length > limit || (type == MDCT_FFT4 && length < 8)) {
        llzs_set_error("llz_mdct_init: length %d out of range for type %d (at most %d)", length, type, limit);
        return LLZ_BAD_HANDLE;
    }
    mdct1_t *f = (mdct1_t *)llz_handle_new(sizeof(*f), LLZ_TAG_MDCT, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->form = type; f->length = length;
    f->d_frame = (double *)llzs_malloc(sizeof(double) * (size_t)length);
    f->d_bins = (double *)llzs_malloc(sizeof(double) * (size_t)length);
    int rc = (f->d_frame && f->d_bins) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK)
        rc = type == MDCT_ORIGIN ? llz_host_mdct_sums_f64(length, &f->d_sum_fwd, &f->d_sum_inv) : mdct1_build_fft_form(f);
    if (rc != LLZ_OK) {
        mdct1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_mdct_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_MDCT, mdct1_destroy); }

/* one direction of one frame between two DEVICE buffers (the frame handles of llz_asmodel_host.c chain this with their own
 * windowing kernels; d_src is not modified, d_dst != d_src) */
static int mdct1_on_device(mdct1_t *f, const double *d_src, double *d_dst, int inverse)
{
    const int N = f->length, K = N >> 1;
    const int n_src = inverse ? K : N, n_dst = inverse ? N : K;
    int rc;
    if (f->form == MDCT_ORIGIN) {                                    /* llz_mdct.c:185-222: the defining sums */
        rc = llzs_matvec_exact_f64(inverse ? f->d_sum_inv : f->d_sum_fwd, d_src, d_dst, n_dst, n_src, NULL);
        if (rc == LLZ_OK && inverse) rc = llzs_scale_4_over_n_f64(d_dst, N, (double)N, NULL);   /* llz_mdct.c:219-220 */
        return rc;
    }
    const int quarter = f->form == MDCT_FFT4;
    /* the N-point form inverts with the inverse transform (llz_mdct.c:258); the N/4-point form uses the FORWARD
     * transform in both directions (llz_mdct.c:291, :328) */
    const int fft_inverse = inverse && !quarter;
    rc = llzs_mdct_rot_f64(quarter, 0, d_src, f->d_work, f->d_rot[inverse ? LLZ_ROT_INV_PRE : LLZ_ROT_FWD_PRE], N, inverse,
                           f->norm, NULL);
    if (rc == LLZ_OK) rc = llzs_fft_f64(f->d_work, f->fft_size, f->d_fft_cs, fft_inverse, NULL);
    if (rc == LLZ_OK)
        rc = llzs_mdct_rot_f64(quarter, 1, f->d_work, d_dst, f->d_rot[inverse ? LLZ_ROT_INV_POST : LLZ_ROT_FWD_POST], N,
                               inverse, f->norm, NULL);
    return rc;
}

int llz_host_mdct_on_device(unsigned long handle, const double *d_src, double *d_dst, int inverse)
{
    mdct1_t *f = (mdct1_t *)llz_handle(handle, LLZ_TAG_MDCT, NULL);
    if (!f || !d_src || !d_dst || d_src == d_dst) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = mdct1_on_device(f, d_src, d_dst, inverse);
    llzs_device_leave(prev);
    return rc;
}

/* the reference's symbols: a frame travels host -> device once and back once */
static void mdct1_run(unsigned long handle, const double *src, double *dst, int inverse, const char *who)
{
    mdct1_t *f = (mdct1_t *)llz_handle(handle, LLZ_TAG_MDCT, NULL);
    if (!f || !src || !dst) {
        llzs_set_error("%s: bad handle or arguments", who);
        return;                                                     /* void in the reference ABI */
    }
    const int N = f->length, K = N >> 1;
    const int n_src = inverse ? K : N, n_dst = inverse ? N : K;
    double *d_src = inverse ? f->d_bins : f->d_frame, *d_dst = inverse ? f->d_frame : f->d_bins;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(d_src, src, sizeof(double) * (size_t)n_src, NULL);
    if (rc == LLZ_OK) rc = mdct1_on_device(f, d_src, d_dst, inverse);
    if (rc == LLZ_OK) rc = llzs_d2h(dst, d_dst, sizeof(double) * (size_t)n_dst, NULL);
    llzs_device_leave(prev);
}

void llz_mdct(unsigned long handle, double *x, double *X) { mdct1_run(handle, x, X, 0, "llz_mdct"); }
void llz_imdct(unsigned long handle, double *X, double *x) { mdct1_run(handle, X, x, 1, "llz_imdct"); }

/* ---- Part 2: batch extension ---- */

typedef struct {
    llz_head_t head;
    int length;
    float *d_tc, *d_ts, *d_cs;
    llz_stage_t st_in, st_out;
} mdcb_t;

static void mdcb_destroy(void *p)
{
    mdcb_t *f = (mdcb_t *)p;
    llzs_free(f->d_tc); llzs_free(f->d_ts); llzs_free(f->d_cs);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_mdct_batch_init(int len)
{
    if (len < 32 || len > 8192 || (len & (len - 1))) {
        llzs_set_error("llz_mdct_batch_init: len %d must be a power of two in 32..8192", len);
        return LLZ_BAD_HANDLE;
    }
    mdcb_t *f = (mdcb_t *)llz_handle_new(sizeof(*f), LLZ_TAG_MDCB, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->length = len;
    int rc = llz_host_mdct_pretwiddles_f32(len, &f->d_tc, &f->d_ts);
    if (rc == LLZ_OK && !(f->d_cs = llz_host_cs_f32(len >> 2))) rc = LLZ_ERR_NOMEM;    /* llz_fft.c:222-229 for size N/4 */
    if (rc != LLZ_OK) {
        mdcb_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_mdct_batch_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_MDCB, mdcb_destroy); }

int llz_mdct_batch_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_MDCB, "llz_mdct_batch_set_stream", stream);
}

static int mdcb_run(unsigned long handle, const float *in, float *out, int count, int inverse, const char *who)
{
    mdcb_t *f = (mdcb_t *)llz_handle(handle, LLZ_TAG_MDCB, NULL);
    if (!f || !in || !out || count < 1) {
        llzs_set_error("%s: bad handle or arguments", who);
        return LLZ_ERR_ARG;
    }
    const int prev = llzs_device_enter(f->head.device);
    const size_t full = sizeof(float) * (size_t)count * f->length, half = full / 2;
    const size_t ib = inverse ? half : full, ob = inverse ? full : half;
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    int rc = (in_dev < 0 || out_dev < 0) ? LLZ_ERR_ARG : LLZ_OK;
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap(who, "in", in, ib, in_dev, "out", out, ob, out_dev);
    const float *d_in = (const float *)llz_vec_stage_in(&f->st_in, in, ib, in_dev, f->head.stream, &rc);
    float *d_out = (float *)llz_vec_stage_out(&f->st_out, out, ob, out_dev, &rc);
    if (rc == LLZ_OK)
        rc = llzs_mdct4_f32(d_in, d_out, count, f->length, f->d_tc, f->d_ts, f->d_cs, inverse, f->head.stream);
    llz_vec_stage_back(out, d_out, ob, out_dev, f->head.stream, &rc);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? count : rc;
}

int llz_mdct_batch(unsigned long handle, const float *x, float *X, int count)
{
    return mdcb_run(handle, x, X, count, 0, "llz_mdct_batch");
}

int llz_imdct_batch(unsigned long handle, const float *X, float *x, int count)
{
    return mdcb_run(handle, X, x, count, 1, "llz_imdct_batch");
}
