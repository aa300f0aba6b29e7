/* llz_kalman_bands_host.c -- include/llz_kalman_bands.h: llz_kalman_bands_mc, the Kalman filter per band (kernel K4l,
 * kalman_bands.hip), after llz_adapt_bands_host.c.  The head, the staged call and the overlap refusal are llz_util.c's.  What is
 * this file's own: the state -- weights and variances [channels][taps][bins], history [channels][taps - 1][bins], noise powers
 * [channels][bins], which the one launch of a call reads and writes back -- in the layout of the set_* and get_* calls, so all of
 * them are plain copies on the stream; the adapt flags; the float32 constants of the recursion; the frame counter; and the eight
 * caller buffers of a call. */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_kalman_bands.h"

#define KALMAN_MAX_BINS 4097
#define KALMAN_MAX_TAPS 32
#define KALMAN_NLMS_TAPS 64             /* llz_adapt_bands_mc's ceiling: taps between the two get a message of their own */

enum { B_XRE, B_XIM, B_DRE, B_DIM, B_ERE, B_EIM, B_YRE, B_YIM, B_COUNT, B_INPUTS = B_ERE };
static const char *const kalman_name[B_COUNT] = { "xre", "xim", "dre", "dim", "ere", "eim", "yre", "yim" };

typedef struct {
    llz_head_t head;
    int channels, bins, taps, hist;     /* hist = max(taps - 1, 1) rows of history */
    float p0;
    float consts[5];                    /* A2 = a a, 1 - A2, lam, 1 - lam, delta: each formed once, in float32 */
    long long frames;                   /* frames since init or reset */
    int *d_on;                          /* device [channels]: 1 = the channel adapts */
    float *d_w[2], *d_h[2];             /* re, im: [channels][taps][bins] weights, [channels][hist][bins] history */
    float *d_p, *d_psi;                 /* [channels][taps][bins] variances, [channels][bins] noise powers */
    llz_stage_t st[B_COUNT];
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
    for (int b = 0; b < B_COUNT; b++) llz_stage_release(&f->st[b]);
    f->head.tag = 0;
    free(f);
}

static size_t kalman_wrow(const kalman_t *f) { return (size_t)f->taps * (size_t)f->bins; }      /* floats of a channel's weights */
static size_t kalman_hrow(const kalman_t *f) { return (size_t)f->hist * (size_t)f->bins; }

static int kalman_refuse(const char *who, int channels, int bins, int taps, float a, float lam, float p0, float delta)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (bins < 1 || bins > KALMAN_MAX_BINS) {
        llzs_set_error("%s: bins %d outside 1..%d", who, bins, KALMAN_MAX_BINS);
        return 1;
    }
    if (taps > KALMAN_MAX_TAPS && taps <= KALMAN_NLMS_TAPS) {
        llzs_set_error("%s: taps %d: above %d taps the weights, the history and the variances of a band no longer fit a lane's "
                       "registers (llz_adapt_bands_mc takes up to %d)", who, taps, KALMAN_MAX_TAPS, KALMAN_NLMS_TAPS);
        return 1;
    }
    if (taps < 1 || taps > KALMAN_MAX_TAPS) {
        llzs_set_error("%s: taps %d outside 1..%d", who, taps, KALMAN_MAX_TAPS);
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
    if (!(delta > 0.f) || !isfinite(delta)) {
        llzs_set_error("%s: delta %g is not a finite value above 0", who, (double)delta);
        return 1;
    }
    return 0;
}

/* zeros in the history and the counter at 0, ordered on the handle's stream */
static int kalman_clear(kalman_t *f)
{
    const size_t bytes = sizeof(float) * (size_t)f->channels * kalman_hrow(f);
    int rc = llzs_memset(f->d_h[0], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_h[1], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) f->frames = 0;
    return rc;
}

/* w = 0, P = p0, psi = 0 */
static int kalman_clear_state(kalman_t *f)
{
    const size_t count = (size_t)f->channels * kalman_wrow(f), bytes = sizeof(float) * count;
    int rc = llzs_memset(f->d_w[0], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_w[1], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_psi, 0, sizeof(float) * (size_t)f->channels * (size_t)f->bins, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_kalman_bands_fill_f32(f->d_p, f->p0, count, f->head.stream);
    return rc;
}

/* the flags of channels [first, first + count) to on[] != 0 (on = NULL: all on), uploaded on the stream behind the calls already
 * issued */
static int kalman_flags(kalman_t *f, const char *who, int first, int count, const int *on)
{
    const size_t bytes = sizeof(int) * (size_t)count;
    int *flags = (int *)malloc(bytes);
    if (!flags) {
        llzs_set_error("%s: no host memory for %zu B of adapt flags", who, bytes);
        return LLZ_ERR_NOMEM;
    }
    for (int c = 0; c < count; c++) flags[c] = on ? on[c] != 0 : 1;
    const int rc = llzs_h2d(f->d_on + first, flags, bytes, f->head.stream);
    free(flags);
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
    int rc = f->head.device < 0 ? LLZ_ERR_DEVICE : LLZ_OK;
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
    if (rc == LLZ_OK) rc = kalman_flags(f, who, 0, channels, NULL);
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
            rc = llz_refuse_device_overlap(who, kalman_name[i], user[i], bytes, on_dev[i], kalman_name[o], user[o], bytes, on_dev[o]);
    void *dev[B_COUNT] = { NULL };
    for (int b = 0; b < nbuf; b++)
        dev[b] = b < B_INPUTS ? (void *)llz_stage_in(&f->st[b], user[b], bytes, on_dev[b], f->head.stream, &rc)
                              : llz_stage_out(&f->st[b], (void *)user[b], bytes, on_dev[b], &rc);
    if (rc == LLZ_ERR_NOMEM) llzs_set_error("%s: no device memory to stage %d buffers of %zu B", who, nbuf, bytes);
    if (rc == LLZ_OK)
        rc = llzs_kalman_bands_f32((const float *)dev[B_XRE], (const float *)dev[B_XIM], (const float *)dev[B_DRE],
                                   (const float *)dev[B_DIM], (float *)dev[B_ERE], (float *)dev[B_EIM], (float *)dev[B_YRE],
                                   (float *)dev[B_YIM], f->d_w[0], f->d_w[1], f->d_h[0], f->d_h[1], f->d_p, f->d_psi, f->d_on,
                                   f->consts, f->channels, f->bins, f->taps, frames, f->head.stream);
    if (rc == LLZ_OK) f->frames += frames;
    for (int o = B_INPUTS; o < nbuf && rc == LLZ_OK; o++)
        if (!on_dev[o]) rc = llzs_d2h((void *)user[o], dev[o], bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static kalman_t *kalman_range(unsigned long h, const char *who, int first, int count, const void *a, const void *b)
{
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, who);
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

/* `count` channels of a state array of `row` floats per channel, up (src) or down (dst), ordered on the stream */
static int kalman_copy(kalman_t *f, float *d_state, size_t row, int first, int count, const float *src, float *dst)
{
    const size_t bytes = sizeof(float) * (size_t)count * row;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = src ? llzs_h2d(d_state + (size_t)first * row, src, bytes, f->head.stream)
                       : llzs_d2h(dst, d_state + (size_t)first * row, bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_kalman_bands_mc_set_adapt(unsigned long h, int first, int count, const int *on)
{
    const char *who = "llz_kalman_bands_mc_set_adapt";
    kalman_t *f = kalman_range(h, who, first, count, on, on);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = kalman_flags(f, who, first, count, on);
    llzs_device_leave(prev);
    return rc;
}

int llz_kalman_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_set_taps", first, count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    const int rc = kalman_copy(f, f->d_w[0], kalman_wrow(f), first, count, wre, NULL);
    return rc == LLZ_OK ? kalman_copy(f, f->d_w[1], kalman_wrow(f), first, count, wim, NULL) : rc;
}

int llz_kalman_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_taps", first, count, wre, wim);
    if (!f) return LLZ_ERR_ARG;
    const int rc = kalman_copy(f, f->d_w[0], kalman_wrow(f), first, count, NULL, wre);
    return rc == LLZ_OK ? kalman_copy(f, f->d_w[1], kalman_wrow(f), first, count, NULL, wim) : rc;
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
    return kalman_copy(f, f->d_p, kalman_wrow(f), first, count, p, NULL);
}

int llz_kalman_bands_mc_get_variance(unsigned long h, int first, int count, float *p)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_variance", first, count, p, p);
    return f ? kalman_copy(f, f->d_p, kalman_wrow(f), first, count, NULL, p) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_get_noise(unsigned long h, int first, int count, float *psi)
{
    kalman_t *f = kalman_range(h, "llz_kalman_bands_mc_get_noise", first, count, psi, psi);
    return f ? kalman_copy(f, f->d_psi, (size_t)f->bins, first, count, NULL, psi) : LLZ_ERR_ARG;
}

int llz_kalman_bands_mc_reset(unsigned long h, int clear)
{
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    int rc = kalman_clear(f);
    if (rc == LLZ_OK && clear) rc = kalman_clear_state(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_kalman_bands_mc_frames(unsigned long h, long long *out)
{
    const char *who = "llz_kalman_bands_mc_frames";
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    *out = f->frames;
    return LLZ_OK;
}

int llz_kalman_bands_mc_plan(unsigned long h, int out[4])
{
    const char *who = "llz_kalman_bands_mc_plan";
    kalman_t *f = (kalman_t *)llz_handle(h, LLZ_TAG_KALB, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("%s: no out", who);
        return LLZ_ERR_ARG;
    }
    return llzs_kalman_bands_plan(f->channels, f->bins, f->taps, out);
}

int llz_kalman_bands_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_KALB, "llz_kalman_bands_mc_set_stream", stream);
}
