/* llz_lpc_filter_host.c -- include/llz_lpc.h part 3: llz_lpc_filter_mc, the prediction-error filter A_f(z) and the all-pole
 * filter 1 / A_f(z) with a coefficient set per (channel, frame) -- llz_lpc_mc's output applied on the device (kernels:
 * lpc_filter.hip).  One handle keeps both delay lines per channel: the last p inputs of the residual direction (float32, two
 * buffers swapped per call: a row's first tile reads the old one while it writes the new one) and the last p unrounded outputs
 * of the synthesis direction (double, updated in place by the channel's own lane).
 *
 * Caller buffers: device memory is used where it lies at any float alignment (both kernels take their rows at the
 * element's alignment: the residual kernel aligns its 16-byte accesses to each row's own address, the synthesis kernel's are
 * unaligned accesses) ; host memory is staged through the handle's device buffers. */
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_levinson.h"
#include "../../../include/llz_lpc.h"
#include "llz_host.h"

#define LLZ_TAG_LPCF 0x4c5a5046

typedef struct {
    llz_head_t head;
    int channels, frame_len, p;
    int cur;                    /* which half of d_hist holds the residual's history in front of the next call */
    float *d_hist;              /* [2][channels][LLZ_LEVINSON_ORDER_MAX]: [c][i] = x(-1 - i), i < p */
    double *d_ys;               /* [channels][LLZ_LEVINSON_ORDER_MAX]: [c][i] = the unrounded y(-1 - i), i < p */
    llz_stage_t st_in, st_cof, st_out;   /* only for callers passing host memory */
} lpcf_t;

static size_t lpcf_hist_count(const lpcf_t *f) { return (size_t)f->channels * LLZ_LEVINSON_ORDER_MAX; }

static void lpcf_destroy(void *p)
{
    lpcf_t *f = (lpcf_t *)p;
    llzs_free(f->d_hist); llzs_free(f->d_ys);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_cof); llz_stage_release(&f->st_out);
    f->head.tag = 0;
    free(f);
}

/* zeros in both delay lines, ordered on the handle's stream */
static int lpcf_clear(lpcf_t *f)
{
    int rc = llzs_memset(f->d_hist, 0, sizeof(float) * 2 * lpcf_hist_count(f), f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_ys, 0, sizeof(double) * lpcf_hist_count(f), f->head.stream);
    f->cur = 0;
    return rc;
}

unsigned long llz_lpc_filter_mc_init(int channels, int frame_len, int p)
{
    const char *who = "llz_lpc_filter_mc_init";
    if (channels < 1) {
        llzs_set_error("%s: channels %d (channels >= 1)", who, channels);
        return LLZ_BAD_HANDLE;
    }
    if (p < 0 || p > LLZ_LEVINSON_ORDER_MAX) {
        llzs_set_error("%s: p %d outside 0..%d", who, p, LLZ_LEVINSON_ORDER_MAX);
        return LLZ_BAD_HANDLE;
    }
    if (frame_len <= p) {
        llzs_set_error("%s: frame_len %d does not exceed p %d (p < frame_len: a frame's history lies in the frame before it)",
                       who, frame_len, p);
        return LLZ_BAD_HANDLE;
    }
    lpcf_t *f = (lpcf_t *)llz_handle_new(sizeof(*f), LLZ_TAG_LPCF, 1);
    if (!f) {
        llzs_set_error("%s: no host memory for the handle", who);
        return LLZ_BAD_HANDLE;
    }
    f->channels = channels; f->frame_len = frame_len; f->p = p;
    const size_t hb = sizeof(float) * 2 * lpcf_hist_count(f), yb = sizeof(double) * lpcf_hist_count(f);
    f->d_hist = (float *)llzs_malloc(hb);
    if (f->d_hist) f->d_ys = (double *)llzs_malloc(yb);
    int rc = LLZ_OK;
    if (!f->d_hist || !f->d_ys) {
        llzs_set_error("%s: no device memory for the delay lines: %zu B and %zu B asked for (%d channels)", who, hb, yb, channels);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = lpcf_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        lpcf_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_lpc_filter_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_LPCF, lpcf_destroy); }

int llz_lpc_filter_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_LPCF, "llz_lpc_filter_mc_set_stream", stream);
}

int llz_lpc_filter_mc_reset(unsigned long handle)
{
    lpcf_t *f = (lpcf_t *)llz_handle(handle, LLZ_TAG_LPCF, "llz_lpc_filter_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = lpcf_clear(f);
    llzs_device_leave(prev);
    return rc;
}

/* both directions: in -> out with acof, `in_name` / `out_name` as the header calls them */
static int lpcf_run(lpcf_t *f, const char *who, int synth, const char *in_name, const float *in, const float *acof,
                    const char *out_name, float *out, int frames)
{
    const size_t fb = sizeof(float);
    const size_t bytes = fb * (size_t)f->channels * (size_t)frames * (size_t)f->frame_len;
    const size_t cbytes = fb * (size_t)f->channels * (size_t)frames * ((size_t)f->p + 1);
    const int in_dev = llzs_is_device_ptr(in), cof_dev = llzs_is_device_ptr(acof), out_dev = llzs_is_device_ptr(out);
    if (in_dev < 0 || cof_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;     /* a buffer of another GPU: refused, message set */
    if (llz_refuse_device_overlap(who, in_name, in, bytes, in_dev, out_name, out, bytes, out_dev) ||
        llz_refuse_device_overlap(who, "acof", acof, cbytes, cof_dev, out_name, out, bytes, out_dev))
        return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = llz_stage_in(&f->st_in, in, bytes, in_dev, f->head.stream, &rc);
    const float *d_cof = llz_stage_in(&f->st_cof, acof, cbytes, cof_dev, f->head.stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc == LLZ_OK && synth)
        rc = llzs_lpc_synth_f32(d_in, d_cof, d_out, f->d_ys, f->channels, frames, f->frame_len, f->p, f->head.stream);
    if (rc == LLZ_OK && !synth) {
        const float *h_in = f->d_hist + (size_t)f->cur * lpcf_hist_count(f);
        float *h_out = f->d_hist + (size_t)(1 - f->cur) * lpcf_hist_count(f);
        rc = llzs_lpc_residual_f32(d_in, d_cof, d_out, h_in, h_out, f->channels, frames, f->frame_len, f->p, f->head.stream);
        if (rc == LLZ_OK) f->cur = 1 - f->cur;
    }
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->head.stream);
    return rc == LLZ_OK ? frames : rc;
}

static int lpcf_call(const char *who, int synth, unsigned long handle, const char *in_name, const float *in, const float *acof,
                     const char *out_name, float *out, int frames)
{
    lpcf_t *f = (lpcf_t *)llz_handle(handle, LLZ_TAG_LPCF, who);
    if (!f) return LLZ_ERR_ARG;
    if (!in || !acof || !out) {
        llzs_set_error("%s: NULL buffer (%s, acof and %s are all needed)", who, in_name, out_name);
        return LLZ_ERR_ARG;
    }
    if (frames < 1) {
        llzs_set_error("%s: frames %d (frames >= 1)", who, frames);
        return LLZ_ERR_ARG;
    }
    if ((long long)frames * f->frame_len > INT_MAX || (long long)frames * f->channels > INT_MAX) {
        llzs_set_error("%s: frames %d x frame_len %d or x channels %d does not fit an int", who, frames, f->frame_len,
                       f->channels);
        return LLZ_ERR_RANGE;
    }
    const int prev = llzs_device_enter(f->head.device);       /* the handle's device, whatever the caller has current */
    const int rc = lpcf_run(f, who, synth, in_name, in, acof, out_name, out, frames);
    llzs_device_leave(prev);
    return rc;
}

int llz_lpc_residual_mc(unsigned long handle, const float *x, const float *acof, float *e, int frames)
{
    return lpcf_call("llz_lpc_residual_mc", 0, handle, "x", x, acof, "e", e, frames);
}

int llz_lpc_synth_mc(unsigned long handle, const float *e, const float *acof, float *y, int frames)
{
    return lpcf_call("llz_lpc_synth_mc", 1, handle, "e", e, acof, "y", y, frames);
}
