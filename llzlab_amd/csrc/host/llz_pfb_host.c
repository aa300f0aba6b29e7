/* llz_pfb_host.c -- include/llz_pfb.h: llz_pfb_mc, the uniform DFT polyphase filter bank (kernels/pfb.hip).  One handle serves
 * both directions, in the shape of llz_stft_mc's (llz_asmodel_host.c): the head, the staged call and the overlap refusal are
 * llz_util.c's, the history behind an analysis call is the FIR family's tail launch.  What is this file's own: the two caller
 * windows, a frame counter and the TIME phase's rotation (m + 1) D mod M per direction, and the synthesis scratch -- a call's
 * inverse transforms go there in chunks of frames of at most LLZ_PFB_SCRATCH_BYTES, and each chunk is overlap-added as a call of
 * its own would be (no bit depends on the grouping of frames, so none depends on the chunks). */
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"
#include "../../../include/llz_pfb.h"

#define LLZ_PFB_SCRATCH_BYTES ((size_t)128 << 20)

typedef struct {
    llz_head_t head;
    int channels, M, D, P, L, bins, keep;   /* keep = L - D */
    int rstep;                              /* D in TIME phase, 0 in FRAME phase */
    float *d_w, *d_g, *d_cs;
    float *d_hist[2], *d_tail[2];           /* [channels][keep], ping-pong */
    int cur_hist, cur_tail;
    long long frames[2];                    /* frames since init or reset: analysis, synthesis */
    int rot[2];                             /* (m + 1) D mod M of the next frame, per direction */
    llz_stage_t st_x, st_re, st_im, st_u;
} pfb_t;

static void pfb_destroy(void *p)
{
    pfb_t *f = (pfb_t *)p;
    if (f->d_g != f->d_w) llzs_free(f->d_g);
    llzs_free(f->d_w); llzs_free(f->d_cs);
    llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]); llzs_free(f->d_tail[0]); llzs_free(f->d_tail[1]);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_re); llz_stage_release(&f->st_im); llz_stage_release(&f->st_u);
    f->head.tag = 0;
    free(f);
}

static int pfb_refuse(const char *who, int channels, int M, int D, int P, const float *w, int phase)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (M < 8 || M > 4096 || (M & (M - 1))) {
        llzs_set_error("%s: bands %d is not a power of two in 8..4096", who, M);
        return 1;
    }
    if (D < 1 || M % D || (M / D != 1 && M / D != 2 && M / D != 4 && M / D != 8)) {
        llzs_set_error("%s: hop %d: bands / hop must be 1, 2, 4 or 8 (bands %d)", who, D, M);
        return 1;
    }
    if (P < 1 || P > LLZ_PFB_MAX_TAPS) {
        llzs_set_error("%s: taps_per_band %d outside 1..%d", who, P, LLZ_PFB_MAX_TAPS);
        return 1;
    }
    if ((long)P * M > LLZ_PFB_MAX_LENGTH) {
        llzs_set_error("%s: prototype length %d x %d = %ld exceeds %d", who, P, M, (long)P * M, LLZ_PFB_MAX_LENGTH);
        return 1;
    }
    if (!w) {
        llzs_set_error("%s: no analysis window (w is NULL)", who);
        return 1;
    }
    if (phase != LLZ_PFB_PHASE_FRAME && phase != LLZ_PFB_PHASE_TIME) {
        llzs_set_error("%s: unknown phase %d (LLZ_PFB_PHASE_FRAME %d, LLZ_PFB_PHASE_TIME %d)", who, phase, LLZ_PFB_PHASE_FRAME,
                       LLZ_PFB_PHASE_TIME);
        return 1;
    }
    return 0;
}

/* both streams at t = 0: histories zero, counters zero, ordered on the handle's stream */
static int pfb_restart(pfb_t *f)
{
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)(f->keep > 0 ? f->keep : 1);
    int rc = llzs_memset(f->d_hist[f->cur_hist], 0, bytes, f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_tail[f->cur_tail], 0, bytes, f->head.stream);
    if (rc != LLZ_OK) return rc;
    f->frames[0] = f->frames[1] = 0;
    f->rot[0] = f->rot[1] = f->D % f->M;
    return LLZ_OK;
}

unsigned long llz_pfb_mc_init(int channels, int bands, int hop, int taps_per_band, const float *w, const float *g, int phase)
{
    const char *who = "llz_pfb_mc_init";
    if (pfb_refuse(who, channels, bands, hop, taps_per_band, w, phase)) return LLZ_BAD_HANDLE;
    pfb_t *f = (pfb_t *)llz_handle_new(sizeof(*f), LLZ_TAG_PFB, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->M = bands; f->D = hop; f->P = taps_per_band; f->L = taps_per_band * bands;
    f->bins = bands / 2 + 1; f->keep = f->L - hop;
    f->rstep = phase == LLZ_PFB_PHASE_TIME ? hop : 0;
    const size_t wbytes = sizeof(float) * (size_t)f->L;
    const size_t kbytes = sizeof(float) * (size_t)channels * (size_t)(f->keep > 0 ? f->keep : 1);
    int rc = f->head.device < 0 ? LLZ_ERR_DEVICE : LLZ_OK;
    if (rc == LLZ_OK) {
        f->d_w = (float *)llz_host_upload(w, wbytes);
        f->d_g = g ? (float *)llz_host_upload(g, wbytes) : f->d_w;
        f->d_cs = llz_host_cs_f32(bands);
        for (int k = 0; k < 2; k++) {
            f->d_hist[k] = (float *)llzs_malloc(kbytes);
            f->d_tail[k] = (float *)llzs_malloc(kbytes);
        }
        if (!f->d_w || !f->d_g || !f->d_cs || !f->d_hist[0] || !f->d_hist[1] || !f->d_tail[0] || !f->d_tail[1]) {
            llzs_set_error("%s: no device memory for the windows and the state: 2 x %zu B and 4 x %zu B asked for", who, wbytes,
                           kbytes);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = pfb_restart(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        pfb_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_pfb_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_PFB, pfb_destroy); }

int llz_pfb_mc_bins(unsigned long h)
{
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, "llz_pfb_mc_bins");
    return f ? f->bins : LLZ_ERR_ARG;
}

int llz_pfb_mc_delay(unsigned long h)
{
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, "llz_pfb_mc_delay");
    return f ? f->keep : LLZ_ERR_ARG;
}

int llz_pfb_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_PFB, "llz_pfb_mc_set_stream", stream);
}

int llz_pfb_mc_frames(unsigned long h, long long *analysis, long long *synthesis)
{
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, "llz_pfb_mc_frames");
    if (!f) return LLZ_ERR_ARG;
    if (analysis) *analysis = f->frames[0];
    if (synthesis) *synthesis = f->frames[1];
    return LLZ_OK;
}

int llz_pfb_mc_reset(unsigned long h)
{
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, "llz_pfb_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = pfb_restart(f);
    llzs_device_leave(prev);
    return rc;
}

/* frames of a synthesis chunk: what the scratch cap holds of [channels][M] floats, one at least */
static int pfb_chunk(const pfb_t *f, int frames)
{
    const size_t per = sizeof(float) * (size_t)f->channels * (size_t)f->M;
    const size_t fit = LLZ_PFB_SCRATCH_BYTES / per;
    return fit < 1 ? 1 : fit < (size_t)frames ? (int)fit : frames;
}

/* the handle and a call's frame count: 0 with a message for a bad handle, a NULL buffer or a count out of range */
static pfb_t *pfb_call(unsigned long h, const char *who, const void *a, const void *b, const void *c, int frames)
{
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, who);
    if (!f) return NULL;
    if (frames < 0 || (long)frames * f->D > 2147483647L) {
        llzs_set_error("%s: frames %d outside 0..%ld (frames x hop below 2^31)", who, frames, 2147483647L / f->D);
        return NULL;
    }
    if (frames > 0 && (!a || !b || !c)) {
        llzs_set_error("%s: NULL buffer", who);
        return NULL;
    }
    return f;
}

/* device views of the three caller buffers: x [C][frames*D], re/im [C][frames][bins]; x_is_input marks which side is input */
static int pfb_stage(pfb_t *f, const char *who, const float *x, const float *re, const float *im, int frames, int x_is_input,
                     float **dx, float **dre, float **dim)
{
    const size_t xb = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->D;
    const size_t sb = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    const int x_dev = llzs_is_device_ptr(x), re_dev = llzs_is_device_ptr(re), im_dev = llzs_is_device_ptr(im);
    if (x_dev < 0 || re_dev < 0 || im_dev < 0) return LLZ_ERR_ARG;
    if (x_is_input ? (llz_refuse_device_overlap(who, "x", x, xb, x_dev, "re", re, sb, re_dev) ||
                      llz_refuse_device_overlap(who, "x", x, xb, x_dev, "im", im, sb, im_dev))
                   : (llz_refuse_device_overlap(who, "re", re, sb, re_dev, "x", x, xb, x_dev) ||
                      llz_refuse_device_overlap(who, "im", im, sb, im_dev, "x", x, xb, x_dev)))
        return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    if (x_is_input) {
        *dx = (float *)llz_stage_in(&f->st_x, x, xb, x_dev, f->head.stream, &rc);
        *dre = (float *)llz_stage_out(&f->st_re, (float *)re, sb, re_dev, &rc);
        *dim = (float *)llz_stage_out(&f->st_im, (float *)im, sb, im_dev, &rc);
    } else {
        *dx = (float *)llz_stage_out(&f->st_x, (float *)x, xb, x_dev, &rc);
        *dre = (float *)llz_stage_in(&f->st_re, re, sb, re_dev, f->head.stream, &rc);
        *dim = (float *)llz_stage_in(&f->st_im, im, sb, im_dev, f->head.stream, &rc);
    }
    if (rc == LLZ_ERR_NOMEM) llzs_set_error("%s: no device memory to stage %zu B of samples and 2 x %zu B of bins", who, xb, sb);
    return rc;
}

/* the counter and the rotation of direction dir behind `frames` more frames */
static void pfb_advance(pfb_t *f, int dir, int frames)
{
    f->frames[dir] += frames;
    f->rot[dir] = (int)(((f->frames[dir] + 1) * f->D) % f->M);
}

int llz_pfb_mc_analysis(unsigned long h, const float *x, float *re, float *im, int frames)
{
    const char *who = "llz_pfb_mc_analysis";
    pfb_t *f = pfb_call(h, who, x, re, im, frames);
    if (!f) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const long n = (long)frames * f->D;
    float *dx, *dre, *dim;
    const int prev = llzs_device_enter(f->head.device);
    int rc = pfb_stage(f, who, x, re, im, frames, 1, &dx, &dre, &dim);
    if (rc == LLZ_OK)
        rc = llzs_pfb_analysis_f32(dx, f->d_hist[f->cur_hist], dre, dim, f->d_w, f->d_cs, f->channels, frames, f->M, f->D, f->L,
                                   f->rstep ? f->rot[0] : 0, f->rstep, n, f->head.stream);
    /* history for the next call: the last L - D samples of concat(history, x) */
    if (rc == LLZ_OK)
        rc = llzs_fir_tail_f32(dx, f->d_hist[f->cur_hist], f->d_hist[f->cur_hist ^ 1], f->channels, n, n, f->keep + 1,
                               f->head.stream);
    if (rc == LLZ_OK) {
        if (f->keep > 0) f->cur_hist ^= 1;
        pfb_advance(f, 0, frames);
    }
    const size_t sb = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->bins;
    if (rc == LLZ_OK && dre != re) rc = llzs_d2h(re, dre, sb, f->head.stream);
    if (rc == LLZ_OK && dim != im) rc = llzs_d2h(im, dim, sb, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

int llz_pfb_mc_synthesis(unsigned long h, const float *re, const float *im, float *x, int frames)
{
    const char *who = "llz_pfb_mc_synthesis";
    pfb_t *f = pfb_call(h, who, re, im, x, frames);
    if (!f) return LLZ_ERR_ARG;
    if (frames == 0) return 0;
    const long n = (long)frames * f->D;
    float *dx, *dre, *dim;
    const int prev = llzs_device_enter(f->head.device);
    int rc = pfb_stage(f, who, x, re, im, frames, 0, &dx, &dre, &dim);
    const int chunk = pfb_chunk(f, frames);
    float *u = NULL;
    if (rc == LLZ_OK) {
        const size_t ub = sizeof(float) * (size_t)f->channels * (size_t)chunk * (size_t)f->M;
        u = (float *)llz_stage_reserve(&f->st_u, ub);
        if (!u) {
            llzs_set_error("%s: no device memory for the %zu-byte scratch of inverse transforms", who, ub);
            rc = LLZ_ERR_NOMEM;
        }
    }
    /* a chunk that fails after an earlier one ran leaves the handle behind the chunks that ran: the streams stay consistent */
    for (int f0 = 0; f0 < frames && rc == LLZ_OK; f0 += chunk) {
        const int count = frames - f0 < chunk ? frames - f0 : chunk;
        rc = llzs_pfb_inverse_f32(dre, dim, u, f->d_cs, f->channels, frames, f0, count, f->M, f->D, f->rstep ? f->rot[1] : 0,
                                  f->rstep, f->head.stream);
        if (rc == LLZ_OK)
            rc = llzs_pfb_ola_f32(u, dx + (size_t)f0 * (size_t)f->D, f->d_tail[f->cur_tail], f->d_tail[f->cur_tail ^ 1], f->d_g,
                                  f->channels, count, f->M, f->D, f->L, n, f->head.stream);
        if (rc == LLZ_OK) {
            f->cur_tail ^= 1;
            pfb_advance(f, 1, count);
        }
    }
    if (rc == LLZ_OK && dx != x) rc = llzs_d2h(x, dx, sizeof(float) * (size_t)f->channels * (size_t)n, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

int llz_pfb_mc_plan(unsigned long h, int frames, int out[8])
{
    const char *who = "llz_pfb_mc_plan";
    pfb_t *f = (pfb_t *)llz_handle(h, LLZ_TAG_PFB, who);
    if (!f) return LLZ_ERR_ARG;
    if (!out || frames < 1 || (long)frames * f->D > 2147483647L) {
        llzs_set_error("%s: no out, or frames %d outside 1..%ld", who, frames, 2147483647L / f->D);
        return LLZ_ERR_ARG;
    }
    return llzs_pfb_plan(f->channels, frames, pfb_chunk(f, frames), f->M, f->D, f->L, out);
}
