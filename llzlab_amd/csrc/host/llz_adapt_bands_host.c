/* llz_adapt_bands_host.c -- include/llz_adapt_bands.h: llz_adapt_bands_mc, the normalised LMS filter per band (kernel K4j,
 * adapt_bands.hip).  The head is llz_util.c's, the staged call, the counter and the copies llz_bands_core.c's, the step sizes
 * with their host copy llz_adapt_core.c's.  What is this file's own: the state -- weights [channels][taps][bins] and history
 * [channels][taps - 1][bins], re and im apart, which the one launch of a call reads and writes back -- in the layout of set_taps
 * and get_taps, so both are plain copies on the stream. */
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_bands.h"

#define BANDS_MAX_TAPS 64

typedef struct {
    llz_bands_t b;
    int channels, bins, taps, hist;     /* hist = max(taps - 1, 1) rows of history */
    float delta;
    llz_adapt_steps_t mu;               /* [channels]: the step sizes */
    float *d_w[2], *d_h[2];             /* re, im: [channels][taps][bins] weights, [channels][hist][bins] history */
} bands_t;

static void bands_destroy(void *p)
{
    bands_t *f = (bands_t *)p;
    for (int k = 0; k < 2; k++) {
        llzs_free(f->d_w[k]);
        llzs_free(f->d_h[k]);
    }
    llz_adapt_steps_destroy(&f->mu);
    llz_bands_release(&f->b);
    f->b.head.tag = 0;
    free(f);
}

static size_t bands_wrow(const bands_t *f) { return (size_t)f->taps * (size_t)f->bins; }        /* floats of a channel's weights */
static size_t bands_hrow(const bands_t *f) { return (size_t)f->hist * (size_t)f->bins; }

/* zeros in the history and the counter at 0, ordered on the handle's stream */
static int bands_clear(bands_t *f)
{
    const int rc = llz_bands_zero_pair(f->d_h, (size_t)f->channels * bands_hrow(f), f->b.head.stream);
    if (rc == LLZ_OK) f->b.frames = 0;
    return rc;
}

static int bands_clear_taps(bands_t *f) { return llz_bands_zero_pair(f->d_w, (size_t)f->channels * bands_wrow(f), f->b.head.stream); }

unsigned long llz_adapt_bands_mc_init(int channels, int bins, int taps, float mu, float delta)
{
    const char *who = "llz_adapt_bands_mc_init";
    if (llz_bands_refuse_count(who, "channels", channels, 1, LLZ_BANDS_MAX_CHANNELS) ||
        llz_bands_refuse_count(who, "bins", bins, 1, LLZ_BANDS_MAX_BINS) ||
        llz_bands_refuse_count(who, "taps", taps, 1, BANDS_MAX_TAPS) || llz_adapt_refuse_mu(who, mu) ||
        llz_adapt_refuse_delta(who, delta))
        return LLZ_BAD_HANDLE;
    bands_t *f = (bands_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ADPB, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->bins = bins; f->taps = taps; f->hist = taps > 1 ? taps - 1 : 1; f->delta = delta;
    const size_t wbytes = sizeof(float) * (size_t)channels * bands_wrow(f);
    const size_t hbytes = sizeof(float) * (size_t)channels * bands_hrow(f);
    int rc = f->b.head.device < 0 ? LLZ_ERR_DEVICE : llz_adapt_steps_create(&f->mu, who, channels, mu);
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
    if (!f || llz_bands_refuse_call(who, frames, f->bins, yre, yim)) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    const llz_bands_buf_t buf[] = LLZ_BANDS_XDEY(bytes, bytes);
    void *const *dev = f->b.io.dev;
    int rc = llz_bands_begin(&f->b, who, buf, 8, 4, 0);
    if (rc == LLZ_OK)
        rc = llzs_bands_nlms_f32(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], f->d_w[0], f->d_w[1], f->d_h[0],
                                 f->d_h[1], f->mu.d_mu, f->delta, f->channels, f->bins, f->taps, frames, f->b.head.stream);
    return llz_bands_end(&f->b, rc, frames);
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static bands_t *bands_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, who);
    return f && !llz_bands_refuse_range(who, "channels", first, count, f->channels, a, b) ? f : NULL;
}

int llz_adapt_bands_mc_set_step(unsigned long h, int first, int count, const float *mu)
{
    const char *who = "llz_adapt_bands_mc_set_step";
    bands_t *f = bands_range(h, who, first, count, mu, mu);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "channel", first, count, mu, f->b.head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim)
{
    bands_t *f = bands_range(h, "llz_adapt_bands_mc_set_taps", first, count, wre, wim);
    return f ? llz_bands_copy_pair(&f->b, f->d_w, bands_wrow(f), first, count, wre, wim, NULL, NULL) : LLZ_ERR_ARG;
}

int llz_adapt_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim)
{
    bands_t *f = bands_range(h, "llz_adapt_bands_mc_get_taps", first, count, wre, wim);
    return f ? llz_bands_copy_pair(&f->b, f->d_w, bands_wrow(f), first, count, NULL, NULL, wre, wim) : LLZ_ERR_ARG;
}

int llz_adapt_bands_mc_reset(unsigned long h, int clear_taps)
{
    bands_t *f = (bands_t *)llz_handle(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    int rc = bands_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = bands_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_bands_mc_frames(unsigned long h, long long *out)
{
    return llz_bands_frames(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_frames", out);
}

int llz_adapt_bands_mc_plan(unsigned long h, int out[4])
{
    const bands_t *f = (const bands_t *)llz_bands_out(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_plan", out);
    return f ? llzs_bands_nlms_plan(f->channels, f->bins, f->taps, out) : LLZ_ERR_ARG;
}

int llz_adapt_bands_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_ADPB, "llz_adapt_bands_mc_set_stream", stream);
}
