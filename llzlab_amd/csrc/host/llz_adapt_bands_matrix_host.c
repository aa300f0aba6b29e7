/* llz_adapt_bands_matrix_host.c -- include/llz_adapt_bands_matrix.h: llz_adapt_bands_matrix_mc, the multi-reference normalised LMS
 * filter per band (kernel K4k, adapt_bands_matrix.hip).  The head, the staged call and the overlap refusal are llz_util.c's, the
 * step sizes with their host copy llz_adapt_core.c's.  What is this file's own: the weights [outputs][inputs][taps][bins], re and
 * im apart, in the layout of set_taps and get_taps, so both are plain copies on the stream (one per output for a sub-matrix of
 * the inputs); the frame counter; the eight caller buffers of a call; and the history [inputs][taps - 1][bins], which every
 * output's lanes read and which a launch therefore never updates in place.  There are TWO history buffers: a launch reads
 * d_h[cur] and writes d_h[cur ^ 1] in full, and cur flips behind a launch that was issued -- never behind an empty or a refused
 * call.  A reset clears d_h[cur] where it is. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_bands_matrix.h"

#define BMX_MAX_INPUTS 8
#define BMX_MAX_OUTPUTS 4096
#define BMX_MAX_BINS 4097
#define BMX_MAX_TAPS 64
#define BMX_MAX_ENTRIES 64

enum { B_XRE, B_XIM, B_DRE, B_DIM, B_ERE, B_EIM, B_YRE, B_YIM, B_COUNT, B_INPUTS = B_ERE, B_X = B_DRE };
static const char *const bmx_name[B_COUNT] = { "xre", "xim", "dre", "dim", "ere", "eim", "yre", "yim" };

typedef struct {
    llz_head_t head;
    int inputs, outputs, bins, taps, hist;  /* hist = max(taps - 1, 1) rows of history per input */
    float delta;
    long long frames;                   /* frames since init or reset */
    llz_adapt_steps_t mu;               /* [outputs]: the step sizes */
    float *d_w[2];                      /* re, im: [outputs][inputs][taps][bins] weights */
    float *d_h[2][2];                   /* [buffer][re, im]: [inputs][hist][bins] history */
    int cur;                            /* the history buffer the next launch reads */
    llz_stage_t st[B_COUNT];
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
    for (int b = 0; b < B_COUNT; b++) llz_stage_release(&f->st[b]);
    f->head.tag = 0;
    free(f);
}

static size_t bmx_path(const bmx_t *f) { return (size_t)f->taps * (size_t)f->bins; }            /* floats of one path's weights */
static size_t bmx_wrow(const bmx_t *f) { return (size_t)f->inputs * bmx_path(f); }              /* ... of an output's */
static size_t bmx_hsize(const bmx_t *f) { return (size_t)f->inputs * (size_t)f->hist * (size_t)f->bins; }

static int bmx_refuse(const char *who, int inputs, int outputs, int bins, int taps, float mu, float delta)
{
    if (inputs < 1 || inputs > BMX_MAX_INPUTS) {
        llzs_set_error("%s: inputs %d outside 1..%d", who, inputs, BMX_MAX_INPUTS);
        return 1;
    }
    if (outputs < 1 || outputs > BMX_MAX_OUTPUTS) {
        llzs_set_error("%s: outputs %d outside 1..%d", who, outputs, BMX_MAX_OUTPUTS);
        return 1;
    }
    if (bins < 1 || bins > BMX_MAX_BINS) {
        llzs_set_error("%s: bins %d outside 1..%d", who, bins, BMX_MAX_BINS);
        return 1;
    }
    if (taps < 1 || taps > BMX_MAX_TAPS) {
        llzs_set_error("%s: taps %d outside 1..%d", who, taps, BMX_MAX_TAPS);
        return 1;
    }
    if (inputs * taps > BMX_MAX_ENTRIES) {
        llzs_set_error("%s: inputs x taps = %d x %d = %d regressor entries, above %d", who, inputs, taps, inputs * taps,
                       BMX_MAX_ENTRIES);
        return 1;
    }
    if (!(mu >= 0.f && mu <= 2.f)) {                                                            /* a NaN fails both */
        llzs_set_error("%s: mu %g outside 0..2", who, (double)mu);
        return 1;
    }
    if (!(delta > 0.f) || !isfinite(delta)) {
        llzs_set_error("%s: delta %g is not a finite value above 0", who, (double)delta);
        return 1;
    }
    return 0;
}

/* zeros in history buffer b, ordered on the handle's stream */
static int bmx_zero_history(bmx_t *f, int b)
{
    const size_t bytes = sizeof(float) * bmx_hsize(f);
    const int rc = llzs_memset(f->d_h[b][0], 0, bytes, f->head.stream);
    return rc == LLZ_OK ? llzs_memset(f->d_h[b][1], 0, bytes, f->head.stream) : rc;
}

/* zeros in the history the next launch reads -- the other buffer is written in full before it is read -- and the counter at 0 */
static int bmx_clear(bmx_t *f)
{
    const int rc = bmx_zero_history(f, f->cur);
    if (rc == LLZ_OK) f->frames = 0;
    return rc;
}

static int bmx_clear_taps(bmx_t *f)
{
    const size_t bytes = sizeof(float) * (size_t)f->outputs * bmx_wrow(f);
    const int rc = llzs_memset(f->d_w[0], 0, bytes, f->head.stream);
    return rc == LLZ_OK ? llzs_memset(f->d_w[1], 0, bytes, f->head.stream) : rc;
}

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
    int rc = f->head.device < 0 ? LLZ_ERR_DEVICE : llz_adapt_steps_create(&f->mu, who, outputs, mu);
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
    if (!f) return LLZ_ERR_ARG;
    if (frames < 0 || (long long)frames * f->bins > 2147483647LL) {
        llzs_set_error("%s: frames %d outside 0..%d (frames x bins below 2^31, bins %d)", who, frames, 2147483647 / f->bins,
                       f->bins);
        return LLZ_ERR_ARG;
    }
    if (!yre != !yim) {
        llzs_set_error("%s: yre and yim must both be NULL or both be set", who);
        return LLZ_ERR_ARG;
    }
    if (frames == 0) return 0;
    if (!xre || !xim || !dre || !dim || !ere || !eim) {
        llzs_set_error("%s: NULL buffer", who);
        return LLZ_ERR_ARG;
    }
    const void *user[B_COUNT] = { xre, xim, dre, dim, ere, eim, yre, yim };
    const int nbuf = yre ? B_COUNT : B_YRE;
    const size_t plane = sizeof(float) * (size_t)frames * (size_t)f->bins;
    size_t bytes[B_COUNT];
    for (int b = 0; b < B_COUNT; b++) bytes[b] = plane * (size_t)(b < B_X ? f->inputs : f->outputs);
    const int prev = llzs_device_enter(f->head.device);
    int on_dev[B_COUNT] = { 0 }, rc = LLZ_OK;
    for (int b = 0; b < nbuf && rc == LLZ_OK; b++)
        if ((on_dev[b] = llzs_is_device_ptr(user[b])) < 0) rc = LLZ_ERR_ARG;   /* a buffer of another GPU: message set */
    /* every output against every input and every output in front of it, before anything is staged or launched */
    for (int o = B_INPUTS; o < nbuf && rc == LLZ_OK; o++)
        for (int i = 0; i < o && rc == LLZ_OK; i++)
            rc = llz_refuse_device_overlap(who, bmx_name[i], user[i], bytes[i], on_dev[i], bmx_name[o], user[o], bytes[o],
                                           on_dev[o]);
    void *dev[B_COUNT] = { NULL };
    for (int b = 0; b < nbuf; b++)
        dev[b] = b < B_INPUTS ? (void *)llz_stage_in(&f->st[b], user[b], bytes[b], on_dev[b], f->head.stream, &rc)
                              : llz_stage_out(&f->st[b], (void *)user[b], bytes[b], on_dev[b], &rc);
    if (rc == LLZ_ERR_NOMEM)
        llzs_set_error("%s: no device memory to stage %d buffers of %zu B (x) and %zu B", who, nbuf, bytes[B_XRE], bytes[B_DRE]);
    if (rc == LLZ_OK)
        rc = llzs_matrix_bands_nlms_f32((const float *)dev[B_XRE], (const float *)dev[B_XIM], (const float *)dev[B_DRE],
                                        (const float *)dev[B_DIM], (float *)dev[B_ERE], (float *)dev[B_EIM], (float *)dev[B_YRE],
                                        (float *)dev[B_YIM], f->d_w[0], f->d_w[1], f->d_h[f->cur][0], f->d_h[f->cur][1],
                                        f->d_h[f->cur ^ 1][0], f->d_h[f->cur ^ 1][1], f->mu.d_mu, f->delta, f->inputs, f->outputs,
                                        f->bins, f->taps, frames, f->head.stream);
    if (rc == LLZ_OK) {                                                        /* the launch is issued: its hout is the history now */
        f->frames += frames;
        f->cur ^= 1;
    }
    for (int o = B_INPUTS; o < nbuf && rc == LLZ_OK; o++)
        if (!on_dev[o]) rc = llzs_d2h((void *)user[o], dev[o], bytes[o], f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

/* the handle and an output range inside it, or NULL with a message naming who */
static bmx_t *bmx_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, who);
    if (!f) return NULL;
    if (!a || !b) {
        llzs_set_error("%s: NULL buffer", who);
        return NULL;
    }
    if (first < 0 || count < 1 || first >= f->outputs || count > f->outputs - first) {
        llzs_set_error("%s: outputs [%d, %d + %d) outside the handle's [0, %d)", who, first, first, count, f->outputs);
        return NULL;
    }
    return f;
}

int llz_adapt_bands_matrix_mc_set_step(unsigned long h, int out_first, int out_count, const float *mu)
{
    const char *who = "llz_adapt_bands_matrix_mc_set_step";
    bmx_t *f = bmx_range(h, who, out_first, out_count, mu, mu);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "output", out_first, out_count, mu, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

/* set_taps (up != 0) or get_taps of the paths (out_first .., in_first ..) between the device weights and HOST [out_count]
 * [in_count][taps][bins]: one copy per component when the inputs are all of them, else one per output */
static int bmx_taps(unsigned long h, const char *who, int out_first, int out_count, int in_first, int in_count, float *wre,
                    float *wim, int up)
{
    bmx_t *f = bmx_range(h, who, out_first, out_count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    if (in_first < 0 || in_count < 1 || in_first >= f->inputs || in_count > f->inputs - in_first) {
        llzs_set_error("%s: inputs [%d, %d + %d) outside the handle's [0, %d)", who, in_first, in_first, in_count, f->inputs);
        return LLZ_ERR_ARG;
    }
    const size_t path = bmx_path(f), wrow = bmx_wrow(f);
    const int whole = in_count == f->inputs;
    const size_t run = (whole ? (size_t)out_count : 1) * (size_t)in_count * path;               /* floats of one copy */
    const int copies = whole ? 1 : out_count;
    float *host[2] = { wre, wim };
    const int prev = llzs_device_enter(f->head.device);
    int rc = LLZ_OK;
    for (int k = 0; k < 2 && rc == LLZ_OK; k++)
        for (int o = 0; o < copies && rc == LLZ_OK; o++) {
            float *d = f->d_w[k] + (size_t)(out_first + o) * wrow + (size_t)in_first * path;
            rc = up ? llzs_h2d(d, host[k] + (size_t)o * run, sizeof(float) * run, f->head.stream)     /* behind the calls issued */
                    : llzs_d2h(host[k] + (size_t)o * run, d, sizeof(float) * run, f->head.stream);
        }
    llzs_device_leave(prev);
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
    const int prev = llzs_device_enter(f->head.device);
    int rc = bmx_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = bmx_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_matrix_mc_frames(unsigned long h, long long *out)
{
    const char *who = "llz_adapt_bands_matrix_mc_frames";
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    *out = f->frames;
    return LLZ_OK;
}

int llz_adapt_bands_matrix_mc_plan(unsigned long h, int out[5])
{
    const char *who = "llz_adapt_bands_matrix_mc_plan";
    bmx_t *f = (bmx_t *)llz_handle(h, LLZ_TAG_ADBX, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    return llzs_matrix_bands_nlms_plan(f->inputs, f->outputs, f->bins, f->taps, out);
}

int llz_adapt_bands_matrix_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_ADBX, "llz_adapt_bands_matrix_mc_set_stream", stream);
}
