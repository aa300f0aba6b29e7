/* llz_adapt_bands_matrix_host.c -- include/llz_adapt_bands_matrix.h: llz_adapt_bands_matrix_mc, the multi-reference normalised LMS
 * filter per band (kernel K4k, adapt_bands_matrix.hip).  The head is llz_util.c's, the staged call, the counter and the range
 * checks llz_bands_core.c's, the step sizes with their host copy llz_adapt_core.c's.  What is this file's own: the weights
 * [outputs][inputs][taps][bins], re and im apart, in the layout of set_taps and get_taps, so both are plain copies on the stream
 * (one per output for a sub-matrix of the inputs); and the history [inputs][taps - 1][bins], which every output's lanes read and
 * which a launch therefore never updates in place.  There are TWO history buffers: a launch reads d_h[cur] and writes
 * d_h[cur ^ 1] in full, and cur flips behind a launch that was issued -- never behind an empty or a refused call.  A reset clears
 * d_h[cur] where it is. */
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_bands_matrix.h"

#define BMX_MAX_INPUTS 8
#define BMX_MAX_OUTPUTS 4096
#define BMX_MAX_TAPS 64
#define BMX_MAX_ENTRIES 64

typedef struct {
    llz_bands_t b;
    int inputs, outputs, bins, taps, hist;  /* hist = max(taps - 1, 1) rows of history per input */
    float delta;
    llz_adapt_steps_t mu;               /* [outputs]: the step sizes */
    float *d_w[2];                      /* re, im: [outputs][inputs][taps][bins] weights */
    float *d_h[2][2];                   /* [buffer][re, im]: [inputs][hist][bins] history */
    int cur;                            /* the history buffer the next launch reads */
} bmx_t;

static void bmx_destroy(void *p)
{
    bmx_t *f = (bmx_t *)p;
    for (int k = 0; k < 2; k++) {
        llzs_free(f->d_w[k]);
        llzs_free(f->d_h[0][k]);
        llzs_free(f->d_h[1][k]);
    }
    llz_adapt_steps_destroy(&f->mu);
    llz_bands_release(&f->b);
    f->b.head.tag = 0;
    free(f);
}

static size_t bmx_path(const bmx_t *f) { return (size_t)f->taps * (size_t)f->bins; }            /* floats of one path's weights */
static size_t bmx_wrow(const bmx_t *f) { return (size_t)f->inputs * bmx_path(f); }              /* ... of an output's */
static size_t bmx_hsize(const bmx_t *f) { return (size_t)f->inputs * (size_t)f->hist * (size_t)f->bins; }

static int bmx_refuse(const char *who, int inputs, int outputs, int bins, int taps, float mu, float delta)
{
    if (llz_bands_refuse_count(who, "inputs", inputs, 1, BMX_MAX_INPUTS) ||
        llz_bands_refuse_count(who, "outputs", outputs, 1, BMX_MAX_OUTPUTS) ||
        llz_bands_refuse_count(who, "bins", bins, 1, LLZ_BANDS_MAX_BINS) || llz_bands_refuse_count(who, "taps", taps, 1, BMX_MAX_TAPS))
        return 1;
    if (inputs * taps > BMX_MAX_ENTRIES) {
        llzs_set_error("%s: inputs x taps = %d x %d = %d regressor entries, above %d", who, inputs, taps, inputs * taps,
                       BMX_MAX_ENTRIES);
        return 1;
    }
    return llz_adapt_refuse_mu(who, mu) || llz_adapt_refuse_delta(who, delta);
}

/* zeros in history buffer b, ordered on the handle's stream */
static int bmx_zero_history(bmx_t *f, int b) { return llz_bands_zero_pair(f->d_h[b], bmx_hsize(f), f->b.head.stream); }

/* zeros in the history the next launch reads -- the other buffer is written in full before it is read -- and the counter at 0 */
static int bmx_clear(bmx_t *f)
{
    const int rc = bmx_zero_history(f, f->cur);
    if (rc == LLZ_OK) f->b.frames = 0;
    return rc;
}

static int bmx_clear_taps(bmx_t *f) { return llz_bands_zero_pair(f->d_w, (size_t)f->outputs * bmx_wrow(f), f->b.head.stream); }

unsigned long llz_adapt_bands_matrix_mc_init(int inputs, int outputs, int bins, int taps, float mu, float delta)
{
    const char *who = "llz_adapt_bands_matrix_mc_init";
    if (bmx_refuse(who, inputs, outputs, bins, taps, mu, delta)) return LLZ_BAD_HANDLE;
    bmx_t *f = (bmx_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ADBX, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->inputs = inputs; f->outputs = outputs; f->bins = bins; f->taps = taps; f->hist = taps > 1 ? taps - 1 : 1; f->delta = delta;
    const size_t wbytes = sizeof(float) * (size_t)outputs * bmx_wrow(f);
    const size_t hbytes = sizeof(float) * bmx_hsize(f);
    int rc = f->b.head.device < 0 ? LLZ_ERR_DEVICE : llz_adapt_steps_create(&f->mu, who, outputs, mu);
    if (rc == LLZ_OK) {
        int ok = f->mu.d_mu != NULL;
        for (int k = 0; k < 2; k++) {
            f->d_w[k] = (float *)llzs_malloc(wbytes);
            f->d_h[0][k] = (float *)llzs_malloc(hbytes);
            f->d_h[1][k] = (float *)llzs_malloc(hbytes);
            ok = ok && f->d_w[k] && f->d_h[0][k] && f->d_h[1][k];
        }
        if (!ok) {
            llzs_set_error("%s: no device memory for the weights, the two histories and the step sizes: 2 x %zu B, 4 x %zu B and "
                           "%zu B asked for (%d outputs x %d inputs x %d taps x %d bins)", who, wbytes, hbytes,
                           sizeof(float) * (size_t)outputs, outputs, inputs, taps, bins);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = bmx_clear_taps(f);
    if (rc == LLZ_OK) rc = bmx_zero_history(f, 1);                                              /* never read before a launch wrote it */
    if (rc == LLZ_OK) rc = bmx_clear(f);                                                        /* cur = 0: the first launch reads buffer 0 */
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        bmx_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_adapt_bands_matrix_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_ADBX, bmx_destroy); }

int llz_adapt_bands_matrix_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                              float *eim, float *yre, float *yim, int frames)
{
    const char *who = "llz_adapt_bands_matrix_mc";
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, who);
    if (!f || llz_bands_refuse_call(who, frames, f->bins, yre, yim)) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const size_t plane = sizeof(float) * (size_t)frames * (size_t)f->bins;
    const llz_bands_buf_t buf[] = LLZ_BANDS_XDEY(plane * (size_t)f->inputs, plane * (size_t)f->outputs);
    void *const *dev = f->b.io.dev;
    int rc = llz_bands_begin(&f->b, who, buf, 8, 4, 2);
    if (rc == LLZ_OK)
        rc = llzs_matrix_bands_nlms_f32(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], f->d_w[0], f->d_w[1],
                                        f->d_h[f->cur][0], f->d_h[f->cur][1], f->d_h[f->cur ^ 1][0], f->d_h[f->cur ^ 1][1],
                                        f->mu.d_mu, f->delta, f->inputs, f->outputs, f->bins, f->taps, frames, f->b.head.stream);
    if (rc == LLZ_OK) f->cur ^= 1;                                              /* the launch is issued: its hout is the history now */
    return llz_bands_end(&f->b, rc, frames);
}

/* the handle and an output range inside it, or NULL with a message naming who */
static bmx_t *bmx_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, who);
    return f && !llz_bands_refuse_range(who, "outputs", first, count, f->outputs, a, b) ? f : NULL;
}

int llz_adapt_bands_matrix_mc_set_step(unsigned long h, int out_first, int out_count, const float *mu)
{
    const char *who = "llz_adapt_bands_matrix_mc_set_step";
    bmx_t *f = bmx_range(h, who, out_first, out_count, mu, mu);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "output", out_first, out_count, mu, f->b.head.stream);
    llzs_device_leave(prev);
    return rc;
}

/* set_taps (up != 0) or get_taps of the paths (out_first .., in_first ..) between the device weights and HOST [out_count]
 * [in_count][taps][bins]: one copy per component when the inputs are all of them, else one per output */
static int bmx_taps(unsigned long h, const char *who, int out_first, int out_count, int in_first, int in_count, float *wre,
                    float *wim, int up)
{
    bmx_t *f = bmx_range(h, who, out_first, out_count, wre, wim);
    if (!f || llz_bands_refuse_range(who, "inputs", in_first, in_count, f->inputs, wre, wim)) return LLZ_ERR_ARG;
    const int whole = in_count == f->inputs;
    const size_t run = (whole ? (size_t)out_count : 1) * (size_t)in_count * bmx_path(f);        /* floats of one copy */
    const int copies = whole ? 1 : out_count;
    float *host[2] = { wre, wim };
    int rc = LLZ_OK;
    for (int k = 0; k < 2 && rc == LLZ_OK; k++)
        for (int o = 0; o < copies && rc == LLZ_OK; o++) {
            float *d = f->d_w[k] + (size_t)(out_first + o) * bmx_wrow(f) + (size_t)in_first * bmx_path(f), *w = host[k] + (size_t)o * run;
            rc = llz_bands_copy(&f->b, d, sizeof(float) * run, 0, 1, up ? w : NULL, w);
        }
    return rc;
}

int llz_adapt_bands_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                       const float *wre, const float *wim)
{
    return bmx_taps(h, "llz_adapt_bands_matrix_mc_set_taps", out_first, out_count, in_first, in_count, (float *)wre, (float *)wim, 1);
}

int llz_adapt_bands_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *wre,
                                       float *wim)
{
    return bmx_taps(h, "llz_adapt_bands_matrix_mc_get_taps", out_first, out_count, in_first, in_count, wre, wim, 0);
}

int llz_adapt_bands_matrix_mc_reset(unsigned long h, int clear_taps)
{
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, "llz_adapt_bands_matrix_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    int rc = bmx_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = bmx_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_matrix_mc_frames(unsigned long h, long long *out)
{
    return llz_bands_frames(h, LLZ_TAG_ADBX, "llz_adapt_bands_matrix_mc_frames", out);
}

int llz_adapt_bands_matrix_mc_plan(unsigned long h, int out[5])
{
    const bmx_t *f = (const bmx_t *)llz_bands_out(h, LLZ_TAG_ADBX, "llz_adapt_bands_matrix_mc_plan", out);
    return f ? llzs_matrix_bands_nlms_plan(f->inputs, f->outputs, f->bins, f->taps, out) : LLZ_ERR_ARG;
}

int llz_adapt_bands_matrix_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_ADBX, "llz_adapt_bands_matrix_mc_set_stream", stream);
}
