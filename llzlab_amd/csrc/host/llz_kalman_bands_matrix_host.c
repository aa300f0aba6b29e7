/* llz_kalman_bands_matrix_host.c -- include/llz_kalman_bands_matrix.h: llz_kalman_bands_matrix_mc, the multi-reference Kalman
 * filter per band (kernel K4n, kalman_bands_matrix.hip).  The head is llz_util.c's, the staged call, the counter, the range
 * checks, the copies and the flag upload llz_bands_core.c's.  What is this file's own: the state -- weights and variances
 * [outputs][inputs][taps][bins], noise powers [outputs][bins] -- in the layout of the set_* and get_* calls, so all of them are
 * plain copies on the stream (one per output for a sub-matrix of the inputs); the adapt flags; the float32 constants of the
 * recursion; and the history [inputs][taps - 1][bins], which every output's lanes read and which a launch therefore never updates
 * in place.  There are TWO history buffers, as in llz_adapt_bands_matrix_host.c: a launch reads d_h[cur] and writes d_h[cur ^ 1]
 * in full, and cur flips behind a launch that was issued -- never behind an empty or a refused call. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_kalman_bands_matrix.h"

#define MKAL_MAX_INPUTS 8
#define MKAL_MAX_OUTPUTS 4096
#define MKAL_MAX_TAPS 32
#define MKAL_MAX_ENTRIES 32
#define MKAL_NLMS_ENTRIES 64            /* llz_adapt_bands_matrix_mc's ceiling, which the entries' refusal points to */

typedef struct {
    llz_bands_t b;
    int inputs, outputs, bins, taps, hist;  /* hist = max(taps - 1, 1) rows of history per input */
    float p0;
    float consts[5];                    /* A2 = a a, 1 - A2, lam, 1 - lam, delta: each formed once, in float32 */
    int *d_on;                          /* device [outputs]: 1 = the output adapts */
    float *d_w[2];                      /* re, im: [outputs][inputs][taps][bins] weights */
    float *d_p, *d_psi;                 /* [outputs][inputs][taps][bins] variances, [outputs][bins] noise powers */
    float *d_h[2][2];                   /* [buffer][re, im]: [inputs][hist][bins] history */
    int cur;                            /* the history buffer the next launch reads */
} mkal_t;

static void mkal_destroy(void *p)
{
    mkal_t *f = (mkal_t *)p;
    for (int k = 0; k < 2; k++) {
        llzs_free(f->d_w[k]);
        llzs_free(f->d_h[0][k]);
        llzs_free(f->d_h[1][k]);
    }
    llzs_free(f->d_p);
    llzs_free(f->d_psi);
    llzs_free(f->d_on);
    llz_bands_release(&f->b);
    f->b.head.tag = 0;
    free(f);
}

static size_t mkal_path(const mkal_t *f) { return (size_t)f->taps * (size_t)f->bins; }          /* floats of one path's weights */
static size_t mkal_wrow(const mkal_t *f) { return (size_t)f->inputs * mkal_path(f); }           /* ... of an output's */
static size_t mkal_hsize(const mkal_t *f) { return (size_t)f->inputs * (size_t)f->hist * (size_t)f->bins; }

static int mkal_refuse(const char *who, int inputs, int outputs, int bins, int taps, float a, float lam, float p0, float delta)
{
    if (llz_bands_refuse_count(who, "inputs", inputs, 1, MKAL_MAX_INPUTS) ||
        llz_bands_refuse_count(who, "outputs", outputs, 1, MKAL_MAX_OUTPUTS) ||
        llz_bands_refuse_count(who, "bins", bins, 1, LLZ_BANDS_MAX_BINS) || llz_bands_refuse_count(who, "taps", taps, 1, MKAL_MAX_TAPS))
        return 1;
    if (inputs * taps > MKAL_MAX_ENTRIES) {
        llzs_set_error("%s: inputs x taps = %d x %d = %d entries: above %d the weights, the regressor and the variances of a band "
                       "no longer fit a lane's registers (llz_adapt_bands_matrix_mc takes up to %d entries)", who, inputs, taps,
                       inputs * taps, MKAL_MAX_ENTRIES, MKAL_NLMS_ENTRIES);
        return 1;
    }
    if (!(a > 0.f && a <= 1.f)) {                                                               /* a NaN fails both */
        llzs_set_error("%s: a %g is not above 0 and at most 1", who, (double)a);
        return 1;
    }
    if (!(lam >= 0.f && lam < 1.f)) {
        llzs_set_error("%s: lam %g is not at least 0 and below 1", who, (double)lam);
        return 1;
    }
    if (!(p0 > 0.f) || !isfinite(p0)) {
        llzs_set_error("%s: p0 %g is not a finite variance above 0", who, (double)p0);
        return 1;
    }
    return llz_adapt_refuse_delta(who, delta);
}

/* zeros in both history buffers and the counter at 0, ordered on the handle's stream */
static int mkal_clear(mkal_t *f)
{
    int rc = llz_bands_zero_pair(f->d_h[0], mkal_hsize(f), f->b.head.stream);
    if (rc == LLZ_OK) rc = llz_bands_zero_pair(f->d_h[1], mkal_hsize(f), f->b.head.stream);
    if (rc == LLZ_OK) f->b.frames = 0;
    return rc;
}

/* w = 0, P = p0, psi = 0 */
static int mkal_clear_state(mkal_t *f)
{
    const size_t count = (size_t)f->outputs * mkal_wrow(f);
    int rc = llz_bands_zero_pair(f->d_w, count, f->b.head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_psi, 0, sizeof(float) * (size_t)f->outputs * (size_t)f->bins, f->b.head.stream);
    if (rc == LLZ_OK) rc = llzs_fill_f32(f->d_p, f->p0, count, f->b.head.stream);
    return rc;
}

unsigned long llz_kalman_bands_matrix_mc_init(int inputs, int outputs, int bins, int taps, float a, float lam, float p0,
                                              float delta)
{
    const char *who = "llz_kalman_bands_matrix_mc_init";
    if (mkal_refuse(who, inputs, outputs, bins, taps, a, lam, p0, delta)) return LLZ_BAD_HANDLE;
    mkal_t *f = (mkal_t *)llz_handle_new(sizeof(*f), LLZ_TAG_KALX, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->inputs = inputs; f->outputs = outputs; f->bins = bins; f->taps = taps; f->hist = taps > 1 ? taps - 1 : 1; f->p0 = p0;
    const float A2 = a * a;                                                                     /* float32 products and differences */
    f->consts[0] = A2; f->consts[1] = 1.f - A2; f->consts[2] = lam; f->consts[3] = 1.f - lam; f->consts[4] = delta;
    const size_t wbytes = sizeof(float) * (size_t)outputs * mkal_wrow(f);
    const size_t hbytes = sizeof(float) * mkal_hsize(f);
    const size_t nbytes = sizeof(float) * (size_t)outputs * (size_t)bins, obytes = sizeof(int) * (size_t)outputs;
    int rc = f->b.head.device < 0 ? LLZ_ERR_DEVICE : LLZ_OK;
    if (rc == LLZ_OK) {
        int ok = 1;
        for (int k = 0; k < 2; k++) {
            f->d_w[k] = (float *)llzs_malloc(wbytes);
            f->d_h[0][k] = (float *)llzs_malloc(hbytes);
            f->d_h[1][k] = (float *)llzs_malloc(hbytes);
            ok = ok && f->d_w[k] && f->d_h[0][k] && f->d_h[1][k];
        }
        f->d_p = (float *)llzs_malloc(wbytes);
        f->d_psi = (float *)llzs_malloc(nbytes);
        f->d_on = (int *)llzs_malloc(obytes);
        if (!ok || !f->d_p || !f->d_psi || !f->d_on) {
            llzs_set_error("%s: no device memory for the weights and variances, the two histories, the noise powers and the flags: "
                           "3 x %zu B, 4 x %zu B, %zu B and %zu B asked for (%d outputs x %d inputs x %d taps x %d bins)", who, wbytes,
                           hbytes, nbytes, obytes, outputs, inputs, taps, bins);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_bands_flags(&f->b, who, "adapt flags", f->d_on, 0, outputs, NULL);
    if (rc == LLZ_OK) rc = mkal_clear_state(f);
    if (rc == LLZ_OK) rc = mkal_clear(f);                                                       /* cur = 0: the first launch reads buffer 0 */
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        mkal_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_kalman_bands_matrix_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_KALX, mkal_destroy); }

int llz_kalman_bands_matrix_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                               float *eim, float *yre, float *yim, int frames)
{
    const char *who = "llz_kalman_bands_matrix_mc";
    mkal_t *f = (mkal_t *)llz_handle(h, LLZ_TAG_KALX, who);
    if (!f || llz_bands_refuse_call(who, frames, f->bins, yre, yim)) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const size_t plane = sizeof(float) * (size_t)frames * (size_t)f->bins;
    const llz_bands_buf_t buf[] = LLZ_BANDS_XDEY(plane * (size_t)f->inputs, plane * (size_t)f->outputs);
    void *const *dev = f->b.io.dev;
    int rc = llz_bands_begin(&f->b, who, buf, 8, 4, 2);
    if (rc == LLZ_OK)
        rc = llzs_mkalman_bands_f32(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], f->d_w[0], f->d_w[1],
                                    f->d_h[f->cur][0], f->d_h[f->cur][1], f->d_h[f->cur ^ 1][0], f->d_h[f->cur ^ 1][1], f->d_p,
                                    f->d_psi, f->d_on, f->consts, f->inputs, f->outputs, f->bins, f->taps, frames,
                                    f->b.head.stream);
    if (rc == LLZ_OK) f->cur ^= 1;                                              /* the launch is issued: its hout is the history now */
    return llz_bands_end(&f->b, rc, frames);
}

/* the handle and an output range inside it, or NULL with a message naming who */
static mkal_t *mkal_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    mkal_t *f = (mkal_t *)llz_handle(h, LLZ_TAG_KALX, who);
    return f && !llz_bands_refuse_range(who, "outputs", first, count, f->outputs, a, b) ? f : NULL;
}

int llz_kalman_bands_matrix_mc_set_adapt(unsigned long h, int out_first, int out_count, const int *on)
{
    const char *who = "llz_kalman_bands_matrix_mc_set_adapt";
    mkal_t *f = mkal_range(h, who, out_first, out_count, on, on);
    return f ? llz_bands_flags(&f->b, who, "adapt flags", f->d_on, out_first, out_count, on) : LLZ_ERR_ARG;
}

/* the handle, an output and an input range inside it, or NULL with a message naming who */
static mkal_t *mkal_paths(unsigned long h, const char *who, int out_first, int out_count, int in_first, int in_count, const void *a,
                          const void *b)
{
    mkal_t *f = mkal_range(h, who, out_first, out_count, a, b);
    return f && !llz_bands_refuse_range(who, "inputs", in_first, in_count, f->inputs, a, b) ? f : NULL;
}

/* up (up != 0) or down, the paths (out_first .., in_first ..) between one device array [outputs][inputs][taps][bins] and HOST
 * [out_count][in_count][taps][bins]: one copy when the inputs are all of them, else one per output */
static int mkal_copy(const mkal_t *f, float *d_state, int out_first, int out_count, int in_first, int in_count, float *host, int up)
{
    const int whole = in_count == f->inputs;
    const size_t run = (whole ? (size_t)out_count : 1) * (size_t)in_count * mkal_path(f);       /* floats of one copy */
    const int copies = whole ? 1 : out_count;
    int rc = LLZ_OK;
    for (int o = 0; o < copies && rc == LLZ_OK; o++) {
        float *d = d_state + (size_t)(out_first + o) * mkal_wrow(f) + (size_t)in_first * mkal_path(f), *w = host + (size_t)o * run;
        rc = llz_bands_copy(&f->b, d, sizeof(float) * run, 0, 1, up ? w : NULL, w);
    }
    return rc;
}

static int mkal_taps(unsigned long h, const char *who, int out_first, int out_count, int in_first, int in_count, float *wre,
                     float *wim, int up)
{
    mkal_t *f = mkal_paths(h, who, out_first, out_count, in_first, in_count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    const int rc = mkal_copy(f, f->d_w[0], out_first, out_count, in_first, in_count, wre, up);
    return rc == LLZ_OK ? mkal_copy(f, f->d_w[1], out_first, out_count, in_first, in_count, wim, up) : rc;
}

int llz_kalman_bands_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                        const float *wre, const float *wim)
{
    return mkal_taps(h, "llz_kalman_bands_matrix_mc_set_taps", out_first, out_count, in_first, in_count, (float *)wre, (float *)wim, 1);
}

int llz_kalman_bands_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *wre,
                                        float *wim)
{
    return mkal_taps(h, "llz_kalman_bands_matrix_mc_get_taps", out_first, out_count, in_first, in_count, wre, wim, 0);
}

int llz_kalman_bands_matrix_mc_set_variance(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                            const float *p)
{
    const char *who = "llz_kalman_bands_matrix_mc_set_variance";
    mkal_t *f = mkal_paths(h, who, out_first, out_count, in_first, in_count, p, p);
    if (!f) return LLZ_ERR_ARG;
    const size_t n = (size_t)out_count * (size_t)in_count * mkal_path(f);
    for (size_t i = 0; i < n; i++)
        if (!(p[i] >= 0.f) || !isfinite(p[i])) {                                                /* a NaN fails the first */
            llzs_set_error("%s: variance %g at element %zu is not finite and at least 0", who, (double)p[i], i);
            return LLZ_ERR_ARG;
        }
    return mkal_copy(f, f->d_p, out_first, out_count, in_first, in_count, (float *)p, 1);
}

int llz_kalman_bands_matrix_mc_get_variance(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *p)
{
    mkal_t *f = mkal_paths(h, "llz_kalman_bands_matrix_mc_get_variance", out_first, out_count, in_first, in_count, p, p);
    return f ? mkal_copy(f, f->d_p, out_first, out_count, in_first, in_count, p, 0) : LLZ_ERR_ARG;
}

int llz_kalman_bands_matrix_mc_get_noise(unsigned long h, int out_first, int out_count, float *psi)
{
    mkal_t *f = mkal_range(h, "llz_kalman_bands_matrix_mc_get_noise", out_first, out_count, psi, psi);
    return f ? llz_bands_copy(&f->b, f->d_psi, sizeof(float) * (size_t)f->bins, out_first, out_count, NULL, psi) : LLZ_ERR_ARG;
}

int llz_kalman_bands_matrix_mc_reset(unsigned long h, int clear)
{
    mkal_t *f = (mkal_t *)llz_handle(h, LLZ_TAG_KALX, "llz_kalman_bands_matrix_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    int rc = mkal_clear(f);
    if (rc == LLZ_OK && clear) rc = mkal_clear_state(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_kalman_bands_matrix_mc_frames(unsigned long h, long long *out)
{
    return llz_bands_frames(h, LLZ_TAG_KALX, "llz_kalman_bands_matrix_mc_frames", out);
}

int llz_kalman_bands_matrix_mc_plan(unsigned long h, int out[5])
{
    const mkal_t *f = (const mkal_t *)llz_bands_out(h, LLZ_TAG_KALX, "llz_kalman_bands_matrix_mc_plan", out);
    return f ? llzs_mkalman_bands_plan(f->inputs, f->outputs, f->bins, f->taps, out) : LLZ_ERR_ARG;
}

int llz_kalman_bands_matrix_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_KALX, "llz_kalman_bands_matrix_mc_set_stream", stream);
}
