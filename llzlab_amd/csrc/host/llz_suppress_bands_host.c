/* llz_suppress_bands_host.c -- include/llz_suppress_bands.h: llz_suppress_bands_mc, the noise and residual-echo postfilter per
 * band (kernel K4m, suppress_bands.hip).  The head is llz_util.c's, the staged call, the counter, the copies and the flag upload
 * llz_bands_core.c's.  What is this file's own: the state -- seven rows [channels][bins], which the one launch of a call reads and
 * writes back -- in the layout of get_state, so that it is a plain copy on the stream; the floors, leakages and flags per
 * channel; the float32 constants of the recursion; the folding of the frame counter into two windows for the kernel; and the
 * seven caller buffers of a call, three of them optional. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_suppress_bands.h"

typedef struct {
    llz_bands_t b;
    int channels, bins, window;
    int with_y;                         /* the last call's form, for plan */
    float consts[10];                   /* omas, omaq, omad, omb, kt, aq, beta, rho, delta, t1: each formed once, in float32 */
    float *d_state;                     /* device [7][channels][bins]: S, Smin, Stmp, q, N, R, Z */
    float *d_floor, *d_leak;            /* device [channels] */
    int *d_on;                          /* device [channels]: 1 = the channel is processed */
} suppress_t;

static void suppress_destroy(void *p)
{
    suppress_t *f = (suppress_t *)p;
    llzs_free(f->d_state);
    llzs_free(f->d_floor);
    llzs_free(f->d_leak);
    llzs_free(f->d_on);
    llz_bands_release(&f->b);
    f->b.head.tag = 0;
    free(f);
}

static size_t suppress_row(const suppress_t *f) { return (size_t)f->channels * (size_t)f->bins; }   /* floats of one state value */

void llz_suppress_bands_mc_default_cfg(llz_suppress_cfg *cfg)
{
    if (!cfg) return;
    cfg->window = 128;
    cfg->as = 0.8f; cfg->aq = 0.2f; cfg->ad = 0.95f;
    cfg->t0 = 2.f; cfg->t1 = 5.f;
    cfg->beta = 0.98f; cfg->rho = 0.6f; cfg->delta = 1e-6f;
}

static int suppress_unit(const char *who, const char *name, float v)
{
    if (v >= 0.f && v < 1.f) return 0;                                                          /* a NaN fails both */
    llzs_set_error("%s: %s %g is not at least 0 and below 1", who, name, (double)v);
    return 1;
}

static int suppress_refuse(const char *who, int channels, int bins, const llz_suppress_cfg *cfg)
{
    if (llz_bands_refuse_count(who, "channels", channels, 1, LLZ_BANDS_MAX_CHANNELS) ||
        llz_bands_refuse_count(who, "bins", bins, 1, LLZ_BANDS_MAX_BINS) || llz_bands_refuse_count(who, "window", cfg->window, 2, 65535))
        return 1;
    if (suppress_unit(who, "as", cfg->as) || suppress_unit(who, "aq", cfg->aq) || suppress_unit(who, "ad", cfg->ad) ||
        suppress_unit(who, "beta", cfg->beta) || suppress_unit(who, "rho", cfg->rho)) return 1;
    if (!(cfg->t0 > 0.f) || !(cfg->t1 > cfg->t0) || !isfinite(cfg->t1)) {
        llzs_set_error("%s: thresholds t0 %g, t1 %g are not finite with 0 < t0 < t1", who, (double)cfg->t0, (double)cfg->t1);
        return 1;
    }
    return llz_adapt_refuse_delta(who, cfg->delta);
}

/* S = Smin = Stmp = N = R = Z = 0, q = 1 and the counter at 0, ordered on the handle's stream */
static int suppress_clear(suppress_t *f)
{
    const size_t row = suppress_row(f);
    int rc = llzs_memset(f->d_state, 0, sizeof(float) * (size_t)LLZ_SUPPRESS_STATES * row, f->b.head.stream);
    if (rc == LLZ_OK) rc = llzs_fill_f32(f->d_state + (size_t)LLZ_SUPPRESS_Q * row, 1.f, row, f->b.head.stream);
    if (rc == LLZ_OK) f->b.frames = 0;
    return rc;
}

unsigned long llz_suppress_bands_mc_init(int channels, int bins, const llz_suppress_cfg *cfg)
{
    const char *who = "llz_suppress_bands_mc_init";
    llz_suppress_cfg own;
    if (!cfg) {
        llz_suppress_bands_mc_default_cfg(&own);
        cfg = &own;
    }
    if (suppress_refuse(who, channels, bins, cfg)) return LLZ_BAD_HANDLE;
    suppress_t *f = (suppress_t *)llz_handle_new(sizeof(*f), LLZ_TAG_SUPB, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->bins = bins; f->window = cfg->window;
    f->consts[0] = 1.f - cfg->as; f->consts[1] = 1.f - cfg->aq; f->consts[2] = 1.f - cfg->ad;       /* float32 differences */
    f->consts[3] = 1.f - cfg->beta; f->consts[4] = 1.f / (cfg->t1 - cfg->t0);
    f->consts[5] = cfg->aq; f->consts[6] = cfg->beta; f->consts[7] = cfg->rho; f->consts[8] = cfg->delta; f->consts[9] = cfg->t1;
    const size_t sbytes = sizeof(float) * (size_t)LLZ_SUPPRESS_STATES * suppress_row(f);
    const size_t cbytes = sizeof(float) * (size_t)channels;
    float *floors = NULL;
    int *flags = NULL;
    int rc = f->b.head.device < 0 ? LLZ_ERR_DEVICE : LLZ_OK;
    if (rc == LLZ_OK) {
        f->d_state = (float *)llzs_malloc(sbytes);
        f->d_floor = (float *)llzs_malloc(cbytes);
        f->d_leak = (float *)llzs_malloc(cbytes);
        f->d_on = (int *)llzs_malloc(sizeof(int) * (size_t)channels);
        if (!f->d_state || !f->d_floor || !f->d_leak || !f->d_on) {
            llzs_set_error("%s: no device memory for the state, the floors, the leakages and the flags: %zu B and 3 x %zu B asked "
                           "for (%d channels x %d bins)", who, sbytes, cbytes, channels, bins);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) {
        floors = (float *)malloc(cbytes);
        flags = (int *)malloc(sizeof(int) * (size_t)channels);
        if (!floors || !flags) {
            llzs_set_error("%s: no host memory for %zu B of floors and flags", who, 2 * cbytes);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) {
        for (int c = 0; c < channels; c++) {
            floors[c] = 0.1f;
            flags[c] = 1;
        }
        rc = llzs_h2d(f->d_floor, floors, cbytes, f->b.head.stream);
        if (rc == LLZ_OK) rc = llzs_h2d(f->d_on, flags, sizeof(int) * (size_t)channels, f->b.head.stream);
        if (rc == LLZ_OK) rc = llzs_memset(f->d_leak, 0, cbytes, f->b.head.stream);
    }
    free(floors);
    free(flags);
    if (rc == LLZ_OK) rc = suppress_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        suppress_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_suppress_bands_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_SUPB, suppress_destroy); }

int llz_suppress_bands_mc(unsigned long h, const float *ere, const float *eim, const float *yre, const float *yim, float *ore,
                          float *oim, float *g, int frames)
{
    const char *who = "llz_suppress_bands_mc";
    suppress_t *f = (suppress_t *)llz_handle(h, LLZ_TAG_SUPB, who);
    if (!f || llz_bands_refuse_call(who, frames, f->bins, yre, yim)) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    const llz_bands_buf_t buf[] = { { "ere", ere, bytes, 0 }, { "eim", eim, bytes, 0 }, { "yre", yre, bytes, 1 }, { "yim", yim, bytes, 1 },
                                    { "ore", ore, bytes, 0 }, { "oim", oim, bytes, 0 }, { "g", g, bytes, 1 } };
    void *const *dev = f->b.io.dev;
    int rc = llz_bands_begin(&f->b, who, buf, 7, 4, 0);
    if (rc == LLZ_OK) {
        const int W = f->window;
        const int n0 = f->b.frames < W ? (int)f->b.frames : W + (int)(f->b.frames % W);
        rc = llzs_suppress_bands_f32(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], f->d_state, f->d_floor, f->d_leak,
                                     f->d_on, f->consts, W, f->channels, f->bins, frames, n0, f->b.head.stream);
    }
    if (rc == LLZ_OK) f->with_y = yre != NULL;
    return llz_bands_end(&f->b, rc, frames);
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static suppress_t *suppress_range(unsigned long h, const char *who, int first, int count, const void *a)
{
    suppress_t *f = (suppress_t *)llz_handle(h, LLZ_TAG_SUPB, who);
    return f && !llz_bands_refuse_range(who, "channels", first, count, f->channels, a, a) ? f : NULL;
}

int llz_suppress_bands_mc_set_floor(unsigned long h, int first, int count, const float *gmin)
{
    const char *who = "llz_suppress_bands_mc_set_floor";
    suppress_t *f = suppress_range(h, who, first, count, gmin);
    if (!f) return LLZ_ERR_ARG;
    for (int c = 0; c < count; c++)
        if (!(gmin[c] >= 0.f && gmin[c] <= 1.f)) {                                              /* a NaN fails both */
            llzs_set_error("%s: floor %g of channel %d is not in [0, 1]", who, (double)gmin[c], first + c);
            return LLZ_ERR_ARG;
        }
    return llz_bands_copy(&f->b, f->d_floor, sizeof(float), first, count, gmin, NULL);
}

int llz_suppress_bands_mc_set_leak(unsigned long h, int first, int count, const float *eta)
{
    const char *who = "llz_suppress_bands_mc_set_leak";
    suppress_t *f = suppress_range(h, who, first, count, eta);
    if (!f) return LLZ_ERR_ARG;
    for (int c = 0; c < count; c++)
        if (!(eta[c] >= 0.f) || !isfinite(eta[c])) {                                            /* a NaN fails the first */
            llzs_set_error("%s: leakage %g of channel %d is not finite and at least 0", who, (double)eta[c], first + c);
            return LLZ_ERR_ARG;
        }
    return llz_bands_copy(&f->b, f->d_leak, sizeof(float), first, count, eta, NULL);
}

int llz_suppress_bands_mc_set_enable(unsigned long h, int first, int count, const int *on)
{
    const char *who = "llz_suppress_bands_mc_set_enable";
    suppress_t *f = suppress_range(h, who, first, count, on);
    return f ? llz_bands_flags(&f->b, who, "flags", f->d_on, first, count, on) : LLZ_ERR_ARG;
}

int llz_suppress_bands_mc_get_state(unsigned long h, int which, int first, int count, float *out)
{
    const char *who = "llz_suppress_bands_mc_get_state";
    suppress_t *f = suppress_range(h, who, first, count, out);
    if (!f) return LLZ_ERR_ARG;
    if (which < 0 || which >= LLZ_SUPPRESS_STATES) {
        llzs_set_error("%s: state value %d outside 0..%d (S, Smin, Stmp, q, N, R, Z)", who, which, LLZ_SUPPRESS_STATES - 1);
        return LLZ_ERR_ARG;
    }
    return llz_bands_copy(&f->b, f->d_state + (size_t)which * suppress_row(f), sizeof(float) * (size_t)f->bins, first, count, NULL, out);
}

int llz_suppress_bands_mc_reset(unsigned long h)
{
    suppress_t *f = (suppress_t *)llz_handle(h, LLZ_TAG_SUPB, "llz_suppress_bands_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    const int rc = suppress_clear(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_suppress_bands_mc_frames(unsigned long h, long long *out)
{
    return llz_bands_frames(h, LLZ_TAG_SUPB, "llz_suppress_bands_mc_frames", out);
}

int llz_suppress_bands_mc_plan(unsigned long h, int out[4])
{
    const suppress_t *f = (const suppress_t *)llz_bands_out(h, LLZ_TAG_SUPB, "llz_suppress_bands_mc_plan", out);
    return f ? llzs_suppress_bands_plan(f->channels, f->bins, f->with_y, out) : LLZ_ERR_ARG;
}

int llz_suppress_bands_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_SUPB, "llz_suppress_bands_mc_set_stream", stream);
}
