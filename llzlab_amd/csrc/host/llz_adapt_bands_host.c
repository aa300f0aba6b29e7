/* llz_adapt_bands_host.c -- include/llz_adapt_bands.h: llz_adapt_bands_mc, the normalised LMS filter per band (kernel K4j,
 * adapt_bands.hip).  The head, the staged call and the overlap refusal are llz_util.c's, the step sizes with their host copy
 * llz_adapt_core.c's.  What is this file's own: the state -- weights [channels][taps][bins] and history [channels][taps - 1]
 * [bins], re and im apart, which the one launch of a call reads and writes back -- in the layout of set_taps and get_taps, so
 * both are plain copies on the stream; the frame counter; and the eight caller buffers of a call. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_bands.h"

#define BANDS_MAX_BINS 4097
#define BANDS_MAX_TAPS 64

enum { B_XRE, B_XIM, B_DRE, B_DIM, B_ERE, B_EIM, B_YRE, B_YIM, B_COUNT, B_INPUTS = B_ERE };
static const char *const bands_name[B_COUNT] = { "xre", "xim", "dre", "dim", "ere", "eim", "yre", "yim" };

typedef struct {
    llz_head_t head;
    int channels, bins, taps, hist;     /* hist = max(taps - 1, 1) rows of history */
    float delta;
    long long frames;                   /* frames since init or reset */
    llz_adapt_steps_t mu;               /* [channels]: the step sizes */
    float *d_w[2], *d_h[2];             /* re, im: [channels][taps][bins] weights, [channels][hist][bins] history */
    llz_stage_t st[B_COUNT];
} bands_t;

static void bands_destroy(void *p)
{
    bands_t *f = (bands_t *)p;
    for (int k = 0; k < 2; k++) {
        llzs_free(f->d_w[k]);
        llzs_free(f->d_h[k]);
    }
    llz_adapt_steps_destroy(&f->mu);
    for (int b = 0; b < B_COUNT; b++) llz_stage_release(&f->st[b]);
    f->head.tag = 0;
    free(f);
}

static size_t bands_wrow(const bands_t *f) { return (size_t)f->taps * (size_t)f->bins; }        /* floats of a channel's weights */
static size_t bands_hrow(const bands_t *f) { return (size_t)f->hist * (size_t)f->bins; }

static int bands_refuse(const char *who, int channels, int bins, int taps, float mu, float delta)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (bins < 1 || bins > BANDS_MAX_BINS) {
        llzs_set_error("%s: bins %d outside 1..%d", who, bins, BANDS_MAX_BINS);
        return 1;
    }
    if (taps < 1 || taps > BANDS_MAX_TAPS) {
        llzs_set_error("%s: taps %d outside 1..%d", who, taps, BANDS_MAX_TAPS);
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

/* zeros in the history and the counter at 0, ordered on the handle's stream */
static int bands_clear(bands_t *f)
{
    const size_t bytes = sizeof(float) * (size_t)f->channels * bands_hrow(f);
    int rc = llzs_memset(f->d_h[0], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_h[1], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) f->frames = 0;
    return rc;
}

static int bands_clear_taps(bands_t *f)
{
    const size_t bytes = sizeof(float) * (size_t)f->channels * bands_wrow(f);
    const int rc = llzs_memset(f->d_w[0], 0, bytes, f->head.stream);
    return rc == LLZ_OK ? llzs_memset(f->d_w[1], 0, bytes, f->head.stream) : rc;
}

unsigned long llz_adapt_bands_mc_init(int channels, int bins, int taps, float mu, float delta)
{
    const char *who = "llz_adapt_bands_mc_init";
    if (bands_refuse(who, channels, bins, taps, mu, delta)) return LLZ_BAD_HANDLE;
    bands_t *f = (bands_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ADPB, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->bins = bins; f->taps = taps; f->hist = taps > 1 ? taps - 1 : 1; f->delta = delta;
    const size_t wbytes = sizeof(float) * (size_t)channels * bands_wrow(f);
    const size_t hbytes = sizeof(float) * (size_t)channels * bands_hrow(f);
    int rc = f->head.device < 0 ? LLZ_ERR_DEVICE : llz_adapt_steps_create(&f->mu, who, channels, mu);
    if (rc == LLZ_OK) {
        for (int k = 0; k < 2; k++) {
            f->d_w[k] = (float *)llzs_malloc(wbytes);
            f->d_h[k] = (float *)llzs_malloc(hbytes);
        }
        if (!f->d_w[0] || !f->d_w[1] || !f->d_h[0] || !f->d_h[1] || !f->mu.d_mu) {
            llzs_set_error("%s: no device memory for the weights, the history and the step sizes: 2 x %zu B, 2 x %zu B and %zu B "
                           "asked for (%d channels x %d taps x %d bins)", who, wbytes, hbytes, sizeof(float) * (size_t)channels,
                           channels, taps, bins);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = bands_clear_taps(f);
    if (rc == LLZ_OK) rc = bands_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        bands_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_adapt_bands_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_ADPB, bands_destroy); }

int llz_adapt_bands_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                       float *eim, float *yre, float *yim, int frames)
{
    const char *who = "llz_adapt_bands_mc";
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, who);
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
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    const int prev = llzs_device_enter(f->head.device);
    int on_dev[B_COUNT] = { 0 }, rc = LLZ_OK;
    for (int b = 0; b < nbuf && rc == LLZ_OK; b++)
        if ((on_dev[b] = llzs_is_device_ptr(user[b])) < 0) rc = LLZ_ERR_ARG;   /* a buffer of another GPU: message set */
    /* every output against every input and every output in front of it, before anything is staged or launched */
    for (int o = B_INPUTS; o < nbuf && rc == LLZ_OK; o++)
        for (int i = 0; i < o && rc == LLZ_OK; i++)
            rc = llz_refuse_device_overlap(who, bands_name[i], user[i], bytes, on_dev[i], bands_name[o], user[o], bytes, on_dev[o]);
    void *dev[B_COUNT] = { NULL };
    for (int b = 0; b < nbuf; b++)
        dev[b] = b < B_INPUTS ? (void *)llz_stage_in(&f->st[b], user[b], bytes, on_dev[b], f->head.stream, &rc)
                              : llz_stage_out(&f->st[b], (void *)user[b], bytes, on_dev[b], &rc);
    if (rc == LLZ_ERR_NOMEM) llzs_set_error("%s: no device memory to stage %d buffers of %zu B", who, nbuf, bytes);
    if (rc == LLZ_OK)
        rc = llzs_bands_nlms_f32((const float *)dev[B_XRE], (const float *)dev[B_XIM], (const float *)dev[B_DRE],
                                 (const float *)dev[B_DIM], (float *)dev[B_ERE], (float *)dev[B_EIM], (float *)dev[B_YRE],
                                 (float *)dev[B_YIM], f->d_w[0], f->d_w[1], f->d_h[0], f->d_h[1], f->mu.d_mu, f->delta,
                                 f->channels, f->bins, f->taps, frames, f->head.stream);
    if (rc == LLZ_OK) f->frames += frames;
    for (int o = B_INPUTS; o < nbuf && rc == LLZ_OK; o++)
        if (!on_dev[o]) rc = llzs_d2h((void *)user[o], dev[o], bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static bands_t *bands_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, who);
    if (!f) return NULL;
    if (!a || !b) {
        llzs_set_error("%s: NULL buffer", who);
        return NULL;
    }
    if (first < 0 || count < 1 || first >= f->channels || count > f->channels - first) {
        llzs_set_error("%s: channels [%d, %d + %d) outside the handle's [0, %d)", who, first, first, count, f->channels);
        return NULL;
    }
    return f;
}

int llz_adapt_bands_mc_set_step(unsigned long h, int first, int count, const float *mu)
{
    const char *who = "llz_adapt_bands_mc_set_step";
    bands_t *f = bands_range(h, who, first, count, mu, mu);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "channel", first, count, mu, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim)
{
    bands_t *f = bands_range(h, "llz_adapt_bands_mc_set_taps", first, count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    const size_t row = bands_wrow(f), bytes = sizeof(float) * (size_t)count * row;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_w[0] + (size_t)first * row, wre, bytes, f->head.stream);             /* behind the calls already issued */
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_w[1] + (size_t)first * row, wim, bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim)
{
    bands_t *f = bands_range(h, "llz_adapt_bands_mc_get_taps", first, count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    const size_t row = bands_wrow(f), bytes = sizeof(float) * (size_t)count * row;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_d2h(wre, f->d_w[0] + (size_t)first * row, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_d2h(wim, f->d_w[1] + (size_t)first * row, bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_reset(unsigned long h, int clear_taps)
{
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    int rc = bands_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = bands_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_frames(unsigned long h, long long *out)
{
    const char *who = "llz_adapt_bands_mc_frames";
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    *out = f->frames;
    return LLZ_OK;
}

int llz_adapt_bands_mc_plan(unsigned long h, int out[4])
{
    const char *who = "llz_adapt_bands_mc_plan";
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    return llzs_bands_nlms_plan(f->channels, f->bins, f->taps, out);
}

int llz_adapt_bands_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_set_stream", stream);
}
