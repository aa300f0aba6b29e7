/*
 * llz_dft_host.c -- handle layer of the DFT of any length and the zoom transform (include/llz_dft.h; kernels/dft.hip): the
 * chirp tables in double (llz_host_dft_tables, the one place they are built), the choice between the fused and the composed
 * form, the refusals of a call, the staging of host buffers whose rows are a pitch apart, and the composed form's walk over
 * `count` in slabs under the scratch cap.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_dft.h"
#include "llz_host.h"

#define LLZ_DFT_MAX_N 1048576
#define LLZ_DFT_FUSED_MAX_M 4096
#define LLZ_DFT_SCRATCH_MB 256
enum { DFT_CPX = 0, DFT_REAL = 1, DFT_HERM = 2 };       /* the kernels' modes (llz_shim.h) */

typedef struct {
    llz_head_t head;
    int n, k, m, zoom, form;
    int scratch_mb;                                     /* cap of the composed form's scratch in MiB */
    double f0, df;
    float *d_cs, *d_twb;
    float *d_pre[2], *d_v[2], *d_post[2];               /* [0] forward, [1] inverse (not for a zoom) */
    llz_stage_t st_in, st_out, st_z;
} dftm_t;

int llz_host_dft_m(int n, int k)
{
    int m = 8;
    while (m < n + k - 1) m *= 2;
    return m;
}

/* the chirp's phase at index i in turns, in [0, 1): exact integer reduction for the DFT, the fractional part in double for the
 * zoom (i < 4096: the argument stays below 2^23 turns) */
static double dft_chirp_turns(int n, int zoom, double df, long i)
{
    if (!zoom) return (double)((i * i) % (2 * (long)n)) / (double)(2 * (long)n);
    const double t = df * (double)(i * i) / 2.0;
    return t - floor(t);
}

/* cos and sin of `turns` turns.  sincos() by name: a compiler merges a cos / sin pair of one argument into it where it can, and
 * its last bit is not always theirs -- the tables must not depend on that choice (tests/dft_checks.py restates them bit for bit) */
static void dft_cs(double turns, double *c, double *s) { sincos(2 * M_PI * turns, s, c); }

/* dst[i] = scale e^{-+ 2 pi i turns}: minus for the forward tables, plus (conj) for the conjugate ones */
static void dft_put(float *dst, size_t i, double turns, int conj, double scale)
{
    double c, s;
    dft_cs(turns, &c, &s);
    dst[2 * i] = (float)(scale * c);
    dst[2 * i + 1] = (float)(scale * (conj ? s : -s));
}

int llz_host_dft_tables(int n, int k, int zoom, double f0, double df, int inverse, int natural, const float *w, float *pre,
                        float *v, float *post)
{
    const int m = llz_host_dft_m(n, k);
    /* pre[i] = c(i) (forward: times w[i], zoom: times e^{-2 pi i f0 i}); the inverse takes conj c */
    for (int i = 0; pre && i < n; i++) {
        double turns = dft_chirp_turns(n, zoom, df, i);
        if (zoom) {
            const double u = f0 * (double)i;
            turns += u - floor(u);
            turns -= floor(turns);
        }
        dft_put(pre, (size_t)i, turns, inverse, !inverse && w ? (double)w[i] : 1.0);
    }
    /* post[j] = c(j); the inverse: conj c(j) w[j] / n */
    for (int j = 0; post && j < k; j++)
        dft_put(post, (size_t)j, dft_chirp_turns(n, zoom, df, j), inverse, inverse ? (w ? (double)w[j] : 1.0) / (double)n : 1.0);
    if (!v) return LLZ_OK;
    /* v[i] = conj c(i), i < k, and v[m - i] = conj c(i), 1 <= i < n (the inverse: c); V = FFT_m(v) */
    double *z = (double *)calloc(2 * (size_t)m, sizeof(double)), *cs = (double *)malloc(sizeof(double) * 2 * (size_t)m);
    if (!z || !cs) {
        free(z); free(cs);
        llzs_set_error("llz_dft: no host memory for the tables of %d points", m);
        return LLZ_ERR_NOMEM;
    }
    llz_host_cs_table(cs, m);
    for (int i = 0; i < (k > n ? k : n); i++) {
        double c, s;
        dft_cs(dft_chirp_turns(n, zoom, df, i), &c, &s);
        if (inverse) s = -s;
        if (i < k) { z[2 * i] = c; z[2 * i + 1] = s; }
        if (i >= 1 && i < n) { z[2 * (m - i)] = c; z[2 * (m - i) + 1] = s; }
    }
    llz_host_dif_f64(z, m, cs);
    int bits = 0;
    while ((1 << bits) < m) bits++;
    for (int e = 0; e < m; e++) {
        /* entry e is bin bitrev(e): the fused kernel's image order, with the transforms' 1 / m; the composed form reads natural
         * order and leaves the 1 / m to the library's inverse transform */
        if (!natural) {
            v[2 * e] = (float)(z[2 * e] / m);
            v[2 * e + 1] = (float)(z[2 * e + 1] / m);
        } else {
            size_t b = 0;
            for (int q = 0; q < bits; q++) b |= (size_t)((e >> q) & 1) << (bits - 1 - q);
            v[2 * b] = (float)z[2 * e];
            v[2 * b + 1] = (float)z[2 * e + 1];
        }
    }
    free(z); free(cs);
    return LLZ_OK;
}

static void dftm_destroy(void *p)
{
    dftm_t *f = (dftm_t *)p;
    llzs_free(f->d_cs); llzs_free(f->d_twb);
    for (int d = 0; d < 2; d++) { llzs_free(f->d_pre[d]); llzs_free(f->d_v[d]); llzs_free(f->d_post[d]); }
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out); llz_stage_release(&f->st_z);
    f->head.tag = 0;
    free(f);
}

/* the tables `what` of one direction through host memory to the device: at init all three on the default stream; from
 * set_window the one the window is folded into, from configure V in the new form's order, on the handle's stream */
enum { DFT_T_PRE = 1, DFT_T_V = 2, DFT_T_POST = 4, DFT_T_ALL = 7 };
static int dft_load(dftm_t *f, const char *who, int inverse, const float *w, int what, void *stream)
{
    const size_t pb = sizeof(float) * 2 * (size_t)f->n, vb = sizeof(float) * 2 * (size_t)f->m, qb = sizeof(float) * 2 * (size_t)f->k;
    const int want_pre = what & DFT_T_PRE, with_v = what & DFT_T_V, want_post = what & DFT_T_POST;
    float *host = (float *)malloc(pb + vb + qb);
    if (!host) {
        llzs_set_error("%s: no host memory for %zu bytes of tables", who, pb + vb + qb);
        return LLZ_ERR_NOMEM;
    }
    float *pre = host, *v = host + 2 * (size_t)f->n, *post = v + 2 * (size_t)f->m;
    int rc = llz_host_dft_tables(f->n, f->k, f->zoom, f->f0, f->df, inverse, f->form == LLZ_DFT_COMPOSED, w, want_pre ? pre : NULL,
                                 with_v ? v : NULL, want_post ? post : NULL);
    if (rc == LLZ_OK && want_pre) rc = llzs_h2d(f->d_pre[inverse], pre, pb, stream);
    if (rc == LLZ_OK && with_v) rc = llzs_h2d(f->d_v[inverse], v, vb, stream);
    if (rc == LLZ_OK && want_post) rc = llzs_h2d(f->d_post[inverse], post, qb, stream);
    free(host);
    return rc;
}

static unsigned long dft_new(const char *who, int n, int k, int zoom, double f0, double df)
{
    dftm_t *f = (dftm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_DFTM, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle", who);
        return LLZ_BAD_HANDLE;
    }
    f->n = n; f->k = k; f->zoom = zoom; f->f0 = f0; f->df = df;
    f->m = llz_host_dft_m(n, k);
    f->form = f->m <= LLZ_DFT_FUSED_MAX_M ? LLZ_DFT_FUSED : LLZ_DFT_COMPOSED;
    f->scratch_mb = LLZ_DFT_SCRATCH_MB;
    const int dirs = zoom ? 1 : 2;
    int ok = 1;
    for (int d = 0; d < dirs; d++) {
        f->d_pre[d] = (float *)llzs_malloc(sizeof(float) * 2 * (size_t)n);
        f->d_v[d] = (float *)llzs_malloc(sizeof(float) * 2 * (size_t)f->m);
        f->d_post[d] = (float *)llzs_malloc(sizeof(float) * 2 * (size_t)k);
        ok = ok && f->d_pre[d] && f->d_v[d] && f->d_post[d];
    }
    f->d_cs = llz_host_cs_f32(f->m);
    const size_t twb = f->m > 4096 ? (size_t)llzs_fft_large_twb_bytes(f->m) : 0;
    if (f->m > 4096) f->d_twb = (float *)llzs_malloc(twb);
    int rc = ok && f->d_cs && (f->m <= 4096 || f->d_twb) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc != LLZ_OK)
        llzs_set_error("%s: device allocation failed (n %d k %d: %d x 3 tables of %d, %d and %d complex floats)", who, n, k, dirs,
                       n, f->m, k);
    if (rc == LLZ_OK && f->d_twb) rc = llzs_fft_large_twb(f->d_twb, f->m, f->d_cs, NULL);
    for (int d = 0; d < dirs && rc == LLZ_OK; d++) rc = dft_load(f, who, d, NULL, DFT_T_ALL, NULL);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        dftm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_dft_mc_init(int n)
{
    if (n < 2 || n > LLZ_DFT_MAX_N) {
        llzs_set_error("llz_dft_mc_init: n %d outside 2..%d", n, LLZ_DFT_MAX_N);
        return LLZ_BAD_HANDLE;
    }
    return dft_new("llz_dft_mc_init", n, n, 0, 0.0, 0.0);
}

unsigned long llz_czt_mc_init(int n, int k, double f0, double df)
{
    if (n < 1 || k < 1 || (long)n + k - 1 > LLZ_DFT_FUSED_MAX_M) {
        llzs_set_error("llz_czt_mc_init: n %d k %d (n >= 1, k >= 1, n + k - 1 <= %d)", n, k, LLZ_DFT_FUSED_MAX_M);
        return LLZ_BAD_HANDLE;
    }
    if (!isfinite(f0) || !isfinite(df) || fabs(df) > 0.5) {
        llzs_set_error("llz_czt_mc_init: f0 %g df %g (both finite, |df| <= 0.5 cycles per sample)", f0, df);
        return LLZ_BAD_HANDLE;
    }
    return dft_new("llz_czt_mc_init", n, k, 1, f0, df);
}

void llz_dft_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_DFTM, dftm_destroy); }

int llz_dft_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_DFTM, "llz_dft_mc_set_stream", stream);
}

int llz_dft_mc_set_window(unsigned long h, const float *w)
{
    static const char who[] = "llz_dft_mc_set_window";
    dftm_t *f = (dftm_t *)llz_handle(h, LLZ_TAG_DFTM, who);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    int rc = dft_load(f, who, 0, w, DFT_T_PRE, f->head.stream);
    if (rc == LLZ_OK && !f->zoom) rc = dft_load(f, who, 1, w, DFT_T_POST, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_dft_mc_configure(unsigned long h, int composed, int scratch_mb)
{
    static const char who[] = "llz_dft_mc_configure";
    dftm_t *f = (dftm_t *)llz_handle(h, LLZ_TAG_DFTM, who);
    if (!f) return LLZ_ERR_ARG;
    if (composed < 0 || composed > 1 || scratch_mb > 65536) {
        llzs_set_error("%s: composed %d scratch_mb %d (0 or 1; at most 65536, negative for the library's %d)", who, composed,
                       scratch_mb, LLZ_DFT_SCRATCH_MB);
        return LLZ_ERR_ARG;
    }
    const int form = f->m <= LLZ_DFT_FUSED_MAX_M && !composed ? LLZ_DFT_FUSED : LLZ_DFT_COMPOSED, old = f->form;
    int rc = LLZ_OK;
    if (form != old) {                                  /* V in the other form's order and scale; the window's tables stay */
        const int prev = llzs_device_enter(f->head.device);
        f->form = form;
        for (int d = 0; d < (f->zoom ? 1 : 2) && rc == LLZ_OK; d++) rc = dft_load(f, who, d, NULL, DFT_T_V, f->head.stream);
        if (rc != LLZ_OK) f->form = old;                /* (a table half loaded: the next configure loads both again) */
        llzs_device_leave(prev);
    }
    if (rc == LLZ_OK) f->scratch_mb = scratch_mb < 0 ? LLZ_DFT_SCRATCH_MB : scratch_mb;
    return rc;
}

/* rows of the composed form's slab under the scratch cap: one at least, `count` at the most */
static int dft_slab_rows(const dftm_t *f, int count)
{
    const size_t cap = (size_t)f->scratch_mb << 20, row = sizeof(float) * 2 * (size_t)f->m;
    const size_t rows = cap / row;
    return rows < 1 ? 1 : rows > (size_t)count ? count : (int)rows;
}

int llz_dft_mc_plan(unsigned long h, int count, int *out)
{
    static const char who[] = "llz_dft_mc_plan";
    dftm_t *f = (dftm_t *)llz_handle(h, LLZ_TAG_DFTM, who);
    if (!f) return LLZ_ERR_ARG;
    if (count < 1 || !out) {
        llzs_set_error("%s: count %d out %p (count >= 1, five ints)", who, count, (void *)out);
        return LLZ_ERR_ARG;
    }
    int wg[2] = {0, 0};
    if (f->form == LLZ_DFT_FUSED && llzs_dft_plan(f->m, count, wg) != LLZ_OK) return LLZ_ERR_ARG;
    const int rows = dft_slab_rows(f, count);
    out[0] = f->form; out[1] = f->m; out[2] = wg[0]; out[3] = wg[1];
    out[4] = f->form == LLZ_DFT_FUSED ? 1 : (count + rows - 1) / rows;
    return LLZ_OK;
}

/* the composed form on device memory: pack, forward, product, inverse, extract, slab by slab */
static int dft_composed(dftm_t *f, const char *who, const float *d_in, float *d_out, long in_pitch, long out_pitch, int count,
                        int inverse, int mode, int kout)
{
    const int rows = dft_slab_rows(f, count);
    const size_t in_el = mode == DFT_REAL ? 1 : 2, out_el = mode == DFT_HERM ? 1 : 2;
    float *z = (float *)llz_stage_reserve(&f->st_z, sizeof(float) * 2 * (size_t)f->m * (size_t)rows);
    if (!z) {
        llzs_set_error("%s: no device memory for the scratch of %d transforms of %d points", who, rows, f->m);
        return LLZ_ERR_NOMEM;
    }
    int rc = LLZ_OK;
    for (int r0 = 0; r0 < count && rc == LLZ_OK; r0 += rows) {
        const int cnt = count - r0 < rows ? count - r0 : rows;
        rc = llzs_dft_pack_f32(d_in + in_el * (size_t)r0 * (size_t)in_pitch, z, f->d_pre[inverse], cnt, f->n, f->m, in_pitch, mode,
                               f->head.stream);
        for (int back = 0; back < 2 && rc == LLZ_OK; back++) {
            rc = f->m <= 4096 ? llzs_fft_f32(z, cnt, f->m, f->d_cs, back, f->head.stream)
                              : llzs_fft_large_f32(z, cnt, f->m, f->d_cs, f->d_twb, back, f->head.stream);
            if (rc == LLZ_OK && !back) rc = llzs_dft_mul_f32(z, f->d_v[inverse], cnt, f->m, f->head.stream);
        }
        if (rc == LLZ_OK)
            rc = llzs_dft_extract_f32(z, d_out + out_el * (size_t)r0 * (size_t)out_pitch, f->d_post[inverse], cnt, kout, f->m,
                                      out_pitch, mode, f->head.stream);
    }
    return rc;
}

/* every transform: the refusals, the staged buffers, one form */
static int dft_run(unsigned long h, const char *who, int zoom, int inverse, int mode, const float *in, long in_pitch, float *out,
                   long out_pitch, int count)
{
    dftm_t *f = (dftm_t *)llz_handle(h, LLZ_TAG_DFTM, who);
    if (!f) return LLZ_ERR_ARG;
    if (f->zoom != zoom) {
        llzs_set_error("%s: the handle is %s", who, f->zoom ? "a zoom handle (llz_czt_mc_init)" : "a DFT handle (llz_dft_mc_init)");
        return LLZ_ERR_ARG;
    }
    if (!in || !out) {
        llzs_set_error("%s: %s NULL", who, !in ? "in" : "out");
        return LLZ_ERR_ARG;
    }
    const int half = f->n / 2 + 1;
    const int in_len = mode == DFT_HERM ? half : f->n;
    const int out_len = mode == DFT_HERM ? f->n : mode == DFT_REAL && !zoom ? half : f->k;
    if (count < 1 || in_pitch < 1 || in_pitch > 0x3fffffffL || out_pitch > 0x3fffffffL) {
        llzs_set_error("%s: count %d in_pitch %ld out_pitch %ld (count >= 1, in_pitch >= 1, pitches below 2^30)", who, count, in_pitch,
                       out_pitch);
        return LLZ_ERR_ARG;
    }
    if (out_pitch < out_len) {
        llzs_set_error("%s: out_pitch %ld below the output row's %d elements", who, out_pitch, out_len);
        return LLZ_ERR_ARG;
    }
    const size_t in_sz = sizeof(float) * (mode == DFT_REAL ? 1 : 2), out_sz = sizeof(float) * (mode == DFT_HERM ? 1 : 2);
    const size_t ib = in_sz * ((size_t)(count - 1) * (size_t)in_pitch + (size_t)in_len);
    const size_t ob = out_sz * ((size_t)(count - 1) * (size_t)out_pitch + (size_t)out_len);
    const int prev = llzs_device_enter(f->head.device);
    const int i_dev = llzs_is_device_ptr(in), o_dev = llzs_is_device_ptr(out);
    int rc = i_dev < 0 || o_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;                /* a buffer of another GPU: refused, message set */
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap(who, "in", in, ib, i_dev, "out", out, ob, o_dev);
    if (rc != LLZ_OK) {
        llzs_device_leave(prev);
        return rc;
    }
    const float *d_in = (const float *)llz_stage_in(&f->st_in, in, ib, i_dev, f->head.stream, &rc);
    /* a host output with gaps between its rows goes up first, so that the gaps come back as they were */
    float *d_out = !o_dev && out_pitch != out_len ? (float *)llz_stage_in(&f->st_out, out, ob, 0, f->head.stream, &rc)
                                                  : (float *)llz_stage_out(&f->st_out, out, ob, o_dev, &rc);
    if (rc == LLZ_OK)
        rc = f->form == LLZ_DFT_FUSED
                 ? llzs_dft_fused_f32(d_in, d_out, f->d_pre[inverse], f->d_v[inverse], f->d_post[inverse], f->d_cs, count, f->n,
                                      out_len, f->m, in_pitch, out_pitch, mode, f->head.stream)
                 : dft_composed(f, who, d_in, d_out, in_pitch, out_pitch, count, inverse, mode, out_len);
    if (rc == LLZ_OK && !o_dev) rc = llzs_d2h(out, d_out, ob, f->head.stream);
    else if (rc == LLZ_OK && !i_dev) rc = llzs_sync(f->head.stream);         /* the stage may be reused by the next call */
    llzs_device_leave(prev);
    return rc;
}

int llz_dft_mc_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_dft_mc_forward", 0, 0, DFT_CPX, in, in_pitch, out, out_pitch, count);
}

int llz_dft_mc_inverse(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_dft_mc_inverse", 0, 1, DFT_CPX, in, in_pitch, out, out_pitch, count);
}

int llz_dft_mc_real_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_dft_mc_real_forward", 0, 0, DFT_REAL, in, in_pitch, out, out_pitch, count);
}

int llz_dft_mc_real_inverse(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_dft_mc_real_inverse", 0, 1, DFT_HERM, in, in_pitch, out, out_pitch, count);
}

int llz_czt_mc_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_czt_mc_forward", 1, 0, DFT_CPX, in, in_pitch, out, out_pitch, count);
}

int llz_czt_mc_real_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count)
{
    return dft_run(h, "llz_czt_mc_real_forward", 1, 0, DFT_REAL, in, in_pitch, out, out_pitch, count);
}
