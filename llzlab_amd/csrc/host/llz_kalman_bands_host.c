/* llz_kalman_bands_host.c -- include/llz_kalman_bands.h: llz_kalman_bands_mc, the Kalman filter per band (kernel K4l,
 * kalman_bands.hip).  The head is llz_util.c's, the staged call, the counter, the copies and the flag upload llz_bands_core.c's.
 * What is this file's own: the state -- weights and variances [channels][taps][bins], history [channels][taps - 1][bins], noise
 * powers [channels][bins], which the one launch of a call reads and writes back -- in the layout of the set_* and get_* calls, so
 * all of them are plain copies on the stream; the adapt flags; and the float32 constants of the recursion. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_kalman_bands.h"

#define KALMAN_MAX_TAPS 32
#define KALMAN_NLMS_TAPS 64             /* llz_adapt_bands_mc's ceiling: taps between the two get a message of their own */

typedef struct {
    llz_bands_t b;
    int channels, bins, taps, hist;     /* hist = max(taps - 1, 1) rows of history */
    float p0;
    float consts[5];                    /* A2 = a a, 1 - A2, lam, 1 - lam, delta: each formed once, in float32 */
    int *d_on;                          /* device [channels]: 1 = the channel adapts */
    float *d_w[2], *d_h[2];             /* re, im: [channels][taps][bins] weights, [channels][hist][bins] history */
    float *d_p, *d_psi;                 /* [channels][taps][bins] variances, [channels][bins] noise powers */
} kalman_t;

static void kalman_destroy(void *p)
{
    kalman_t *f = (kalman_t *)p;
    for (int k = 0; k < 2; k++) {
        llzs_free(f->d_w[k]);
        llzs_free(f->d_h[k]);
    }
    llzs_free(f->d_p);
    llzs_free(f->d_psi);
    llzs_free(f->d_on);
    llz_bands_release(&f->b);
    f->b.head.tag = 0;
    free(f);
}

static size_t kalman_wrow(const kalman_t *f) { return (size_t)f->taps * (size_t)f->bins; }      /* floats of a channel's weights */
static size_t kalman_hrow(const kalman_t *f) { return (size_t)f->hist * (size_t)f->bins; }

static int kalman_refuse(const char *who, int channels, int bins, int taps, float a, float lam, float p0, float delta)
{
    if (llz_bands_refuse_count(who, "channels", channels, 1, LLZ_BANDS_MAX_CHANNELS) ||
        llz_bands_refuse_count(who, "bins", bins, 1, LLZ_BANDS_MAX_BINS))
        return 1;
    if (taps > KALMAN_MAX_TAPS && taps <= KALMAN_NLMS_TAPS) {
        llzs_set_error("%s: taps %d: above %d taps the weights, the history and the variances of a band no longer fit a lane's "
                       "registers (llz_adapt_bands_mc takes up to %d)", who, taps, KALMAN_MAX_TAPS, KALMAN_NLMS_TAPS);
        return 1;
    }
    if (llz_bands_refuse_count(who, "taps", taps, 1, KALMAN_MAX_TAPS)) return 1;
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

/* zeros in the history and the counter at 0, ordered on the handle's stream */
static int kalman_clear(kalman_t *f)
{
    const int rc = llz_bands_zero_pair(f->d_h, (size_t)f->channels * kalman_hrow(f), f->b.head.stream);
    if (rc == LLZ_OK) f->b.frames = 0;
    return rc;
}

/* w = 0, P = p0, psi = 0 */
static int kalman_clear_state(kalman_t *f)
{
    const size_t count = (size_t)f->channels * kalman_wrow(f);
    int rc = llz_bands_zero_pair(f->d_w, count, f->b.head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_psi, 0, sizeof(float) * (size_t)f->channels * (size_t)f->bins, f->b.head.stream);
    if (rc == LLZ_OK) rc = llzs_fill_f32(f->d_p, f->p0, count, f->b.head.stream);
    return rc;
}

unsigned long llz_kalman_bands_mc_init(int channels, int bins, int taps, float a, float lam, float p0, float delta)
{
    const char *who = "llz_kalman_bands_mc_init";
    if (kalman_refuse(who, channels, bins, taps, a, lam, p0, delta)) return LLZ_BAD_HANDLE;
    kalman_t *f = (kalman_t *)llz_handle_new(sizeof(*f), LLZ_TAG_KALB, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->bins = bins; f->taps = taps; f->hist = taps > 1 ? taps - 1 : 1; f->p0 = p0;
    const float A2 = a * a;                                                                     /* float32 products and differences */
    f->consts[0] = A2; f->consts[1] = 1.f - A2; f->consts[2] = lam; f->consts[3] = 1.f - lam; f->consts[4] = delta;
    const size_t wbytes = sizeof(float) * (size_t)channels * kalman_wrow(f);
    const size_t hbytes = sizeof(float) * (size_t)channels * kalman_hrow(f);
    const size_t nbytes = sizeof(float) * (size_t)channels * (size_t)bins, obytes = sizeof(int) * (size_t)channels;
    int rc = f->b.head.device < 0 ? LLZ_ERR_DEVICE : LLZ_OK;
    if (rc == LLZ_OK) {
        for (int k = 0; k < 2; k++) {
            f->d_w[k] = (float *)llzs_malloc(wbytes);
            f->d_h[k] = (float *)llzs_malloc(hbytes);
        }
        f->d_p = (float *)llzs_malloc(wbytes);
        f->d_psi = (float *)llzs_malloc(nbytes);
        f->d_on = (int *)llzs_malloc(obytes);
        if (!f->d_w[0] || !f->d_w[1] || !f->d_h[0] || !f->d_h[1] || !f->d_p || !f->d_psi || !f->d_on) {
            llzs_set_error("%s: no device memory for the weights and variances, the history, the noise powers and the flags: "
                           "3 x %zu B, 2 x %zu B, %zu B and %zu B asked for (%d channels x %d taps x %d bins)", who, wbytes, hbytes,
                           nbytes, obytes, channels, taps, bins);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_bands_flags(&f->b, who, "adapt flags", f->d_on, 0, channels, NULL);
    if (rc == LLZ_OK) rc = kalman_clear_state(f);
    if (rc == LLZ_OK) rc = kalman_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        kalman_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_kalman_bands_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_KALB, kalman_destroy); }

int llz_kalman_bands_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                        float *eim, float *yre, float *yim, int frames)
{
    const char *who = "llz_kalman_bands_mc";
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, who);
    if (!f || llz_bands_refuse_call(who, frames, f->bins, yre, yim)) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    const llz_bands_buf_t buf[] = LLZ_BANDS_XDEY(bytes, bytes);
    void *const *dev = f->b.io.dev;
    int rc = llz_bands_begin(&f->b, who, buf, 8, 4, 0);
    if (rc == LLZ_OK)
        rc = llzs_kalman_bands_f32(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], f->d_w[0], f->d_w[1], f->d_h[0],
                                   f->d_h[1], f->d_p, f->d_psi, f->d_on, f->consts, f->channels, f->bins, f->taps, frames,
                                   f->b.head.stream);
    return llz_bands_end(&f->b, rc, frames);
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static kalman_t *kalman_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, who);
    return f && !llz_bands_refuse_range(who, "channels", first, count, f->channels, a, b) ? f : NULL;
}

int llz_kalman_bands_mc_set_adapt(unsigned long h, int first, int count, const int *on)
{
    const char *who = "llz_kalman_bands_mc_set_adapt";
    kalman_t *f = kalman_range(h, who, first, count, on, on);
    return f ? llz_bands_flags(&f->b, who, "adapt flags", f->d_on, first, count, on) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_set_taps", first, count, wre, wim);
    return f ? llz_bands_copy_pair(&f->b, f->d_w, kalman_wrow(f), first, count, wre, wim, NULL, NULL) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_taps", first, count, wre, wim);
    return f ? llz_bands_copy_pair(&f->b, f->d_w, kalman_wrow(f), first, count, NULL, NULL, wre, wim) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_set_variance(unsigned long h, int first, int count, const float *p)
{
    const char *who = "llz_kalman_bands_mc_set_variance";
    kalman_t *f = kalman_range(h, who, first, count, p, p);
    if (!f) return LLZ_ERR_ARG;
    const size_t n = (size_t)count * kalman_wrow(f);
    for (size_t i = 0; i < n; i++)
        if (!(p[i] >= 0.f) || !isfinite(p[i])) {                                                /* a NaN fails the first */
            llzs_set_error("%s: variance %g at element %zu is not finite and at least 0", who, (double)p[i], i);
            return LLZ_ERR_ARG;
        }
    return llz_bands_copy(&f->b, f->d_p, sizeof(float) * kalman_wrow(f), first, count, p, NULL);
}

int llz_kalman_bands_mc_get_variance(unsigned long h, int first, int count, float *p)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_variance", first, count, p, p);
    return f ? llz_bands_copy(&f->b, f->d_p, sizeof(float) * kalman_wrow(f), first, count, NULL, p) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_get_noise(unsigned long h, int first, int count, float *psi)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_noise", first, count, psi, psi);
    return f ? llz_bands_copy(&f->b, f->d_psi, sizeof(float) * (size_t)f->bins, first, count, NULL, psi) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_reset(unsigned long h, int clear)
{
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->b.head.device);
    int rc = kalman_clear(f);
    if (rc == LLZ_OK && clear) rc = kalman_clear_state(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_kalman_bands_mc_frames(unsigned long h, long long *out)
{
    return llz_bands_frames(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_frames", out);
}

int llz_kalman_bands_mc_plan(unsigned long h, int out[4])
{
    const kalman_t *f = (const kalman_t *)llz_bands_out(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_plan", out);
    return f ? llzs_kalman_bands_plan(f->channels, f->bins, f->taps, out) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_set_stream", stream);
}
