/* llz_adapt_host.c -- include/llz_adapt.h: llz_adapt_mc, the partitioned frequency-domain NLMS adaptive filter (kernel K4h,
 * fir_adapt.hip).  Its own handle and tag.  What it shares with the stream convolver (llz_fir_stream_host.c) it takes from the
 * same places: the split-twiddle table (llz_host_stream_twiddles), the builder of the packed spectra for set_taps
 * (llz_host_load_spectra) and its inverse for get_taps (llz_host_stream_taps), the staged call and the overlap refusal
 * (llz_util.c).  The ring's head and the step sizes' host copy live here: the head goes by value with each launch, and a call
 * launches no update while every channel is frozen. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"
#include "../../../include/llz_adapt.h"

#define ADPT_MIN_BLOCK 64
#define ADPT_MAX_BLOCK 2048
#define ADPT_STAGE_BYTES ((size_t)8 << 20)      /* host staging of get_taps: whole rows up to this, one row at least */

typedef struct {
    int tag;                    /* LLZ_TAG_ADPT */
    int device;
    int channels, block, frame_len, flt_len;
    int k, P, R;                /* blocks per call of the init's frame_len, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes */
    float delta;
    float *h_mu;                /* HOST [channels]: the step sizes; d_mu is its device copy */
    int adapting;               /* channels whose mu is not zero */
    float *d_w;                 /* [channels][P][block] complex: the weights' packed spectra */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [channels][R][block] complex */
    float *d_prev;              /* [channels][block]: the last input block */
    float *d_g;                 /* [channels][block] complex: the normalised gradient of the block in flight */
    float *d_mu;                /* [channels] */
    void *stream;
    llz_stage_t st_x, st_d, st_e, st_y;
} adpt_t;

static void adpt_destroy(adpt_t *f)
{
    if (!f) return;
    llzs_free(f->d_w); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev); llzs_free(f->d_g); llzs_free(f->d_mu);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_d); llz_stage_release(&f->st_e); llz_stage_release(&f->st_y);
    free(f->h_mu);
    f->tag = 0;
    free(f);
}

static size_t adpt_row(const adpt_t *f) { return 2 * (size_t)f->P * (size_t)f->block; }       /* floats of a channel's spectra */

static int adpt_mu_ok(float mu) { return mu >= 0.f && mu <= 2.f; }                             /* a NaN fails both */

static int adpt_refuse(const char *who, int channels, int block, int frame_len, int flt_len, float mu, float delta)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (block == 4096) {
        llzs_set_error("%s: block 4096 is not built (a thread would own 16 bins: no registers left); blocks are %d..%d", who,
                       ADPT_MIN_BLOCK, ADPT_MAX_BLOCK);
        return 1;
    }
    if (block < ADPT_MIN_BLOCK || block > ADPT_MAX_BLOCK || (block & (block - 1))) {
        llzs_set_error("%s: block %d is not a power of two in %d..%d", who, block, ADPT_MIN_BLOCK, ADPT_MAX_BLOCK);
        return 1;
    }
    if (frame_len < block || frame_len % block) {
        llzs_set_error("%s: frame_len %d is not k x block with k >= 1 (block %d)", who, frame_len, block);
        return 1;
    }
    if (flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("%s: flt_len %d outside 1..%d", who, flt_len, LLZS_FIR_PART_MAX_TAPS);
        return 1;
    }
    if (!adpt_mu_ok(mu)) {
        llzs_set_error("%s: mu %g outside 0..2", who, (double)mu);
        return 1;
    }
    if (!(delta > 0.f) || !isfinite(delta)) {
        llzs_set_error("%s: delta %g is not a finite value above 0", who, (double)delta);
        return 1;
    }
    return 0;
}

/* zeros in the delay line, ordered on the handle's stream */
static int adpt_clear(adpt_t *f)
{
    int rc = llzs_memset(f->d_ring, 0, sizeof(float) * 2 * (size_t)f->channels * (size_t)f->R * (size_t)f->block, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev, 0, sizeof(float) * (size_t)f->channels * (size_t)f->block, f->stream);
    f->head = 0;
    return rc;
}

static int adpt_clear_taps(adpt_t *f)
{
    return llzs_memset(f->d_w, 0, sizeof(float) * (size_t)f->channels * adpt_row(f), f->stream);
}

unsigned long llz_adapt_mc_init(int channels, int block, int frame_len, int flt_len, float mu, float delta)
{
    const char *who = "llz_adapt_mc_init";
    if (adpt_refuse(who, channels, block, frame_len, flt_len, mu, delta)) return LLZ_BAD_HANDLE;
    adpt_t *f = (adpt_t *)calloc(1, sizeof(*f));
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->tag = LLZ_TAG_ADPT;
    f->device = llzs_device_get();
    f->channels = channels; f->block = block; f->frame_len = frame_len; f->flt_len = flt_len; f->delta = delta;
    f->k = frame_len / block;
    f->P = (flt_len + block - 1) / block;
    f->R = f->P + f->k - 1;
    const size_t wbytes = sizeof(float) * (size_t)channels * adpt_row(f);
    const size_t rbytes = sizeof(float) * 2 * (size_t)channels * (size_t)f->R * (size_t)block;
    const size_t tbytes = sizeof(float) * 2 * ((size_t)block / 2 + (size_t)block);
    const size_t pbytes = sizeof(float) * (size_t)channels * (size_t)block, mbytes = sizeof(float) * (size_t)channels;
    int rc = LLZ_OK;
    f->h_mu = (float *)malloc(mbytes);
    if (!f->h_mu) {
        llzs_set_error("%s: no host memory for %zu B of step sizes", who, mbytes);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_w = (float *)llzs_malloc(wbytes))) {
        llzs_set_error("%s: no device memory for the weights' spectra: %zu B asked for (%d channels x %d partitions x %d bins)", who,
                       wbytes, channels, f->P, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_ring = (float *)llzs_malloc(rbytes))) {
        llzs_set_error("%s: no device memory for the delay line: %zu B asked for (%d channels x %d slots x %d bins)", who, rbytes,
                       channels, f->R, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) {
        f->d_tw = (float *)llzs_malloc(tbytes);
        f->d_prev = (float *)llzs_malloc(pbytes);
        f->d_g = (float *)llzs_malloc(2 * pbytes);
        f->d_mu = (float *)llzs_malloc(mbytes);
        if (!f->d_tw || !f->d_prev || !f->d_g || !f->d_mu) {
            llzs_set_error("%s: no device memory for the twiddles, the last input blocks, the gradient and the step sizes: %zu B, "
                           "%zu B, %zu B and %zu B asked for", who, tbytes, pbytes, 2 * pbytes, mbytes);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, f->block);
    if (rc == LLZ_OK) {
        for (int c = 0; c < channels; c++) f->h_mu[c] = mu;
        f->adapting = mu != 0.f ? channels : 0;
        rc = llzs_h2d(f->d_mu, f->h_mu, mbytes, NULL);
    }
    if (rc == LLZ_OK) rc = adpt_clear_taps(f);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_g, 0, 2 * pbytes, f->stream);
    if (rc == LLZ_OK) rc = adpt_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        adpt_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_adapt_mc_uninit(unsigned long h)
{
    if (LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT)) {
        adpt_t *f = (adpt_t *)h;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        adpt_destroy(f);
        llzs_device_leave(prev);
    }
}

static int adpt_process(adpt_t *f, const float *x, const float *d, float *e, float *y, int frame_len)
{
    const char *who = "llz_adapt_mc";
    if (frame_len < f->block || frame_len > f->frame_len || frame_len % f->block) {
        llzs_set_error("%s: frame_len %d is not a multiple of block %d in %d..%d (the init's frame_len)", who, frame_len, f->block,
                       f->block, f->frame_len);
        return LLZ_ERR_ARG;
    }
    if ((const float *)e == x || (const float *)e == d || (y && ((const float *)y == x || (const float *)y == d || y == e))) {
        llzs_set_error("%s: in-place filtering is not supported: e and y may not be x, d or each other", who);
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len, ybytes = y ? bytes : 0;
    const int x_dev = llzs_is_device_ptr(x), d_dev = llzs_is_device_ptr(d), e_dev = llzs_is_device_ptr(e);
    const int y_dev = y ? llzs_is_device_ptr(y) : 0;
    if (x_dev < 0 || d_dev < 0 || e_dev < 0 || y_dev < 0) return LLZ_ERR_ARG;        /* a buffer of another GPU: message set */
    if (llz_refuse_device_overlap(who, "x", x, bytes, x_dev, "e", e, bytes, e_dev) ||
        llz_refuse_device_overlap(who, "d", d, bytes, d_dev, "e", e, bytes, e_dev) ||
        llz_refuse_device_overlap(who, "x", x, bytes, x_dev, "y", y, ybytes, y_dev) ||
        llz_refuse_device_overlap(who, "d", d, bytes, d_dev, "y", y, ybytes, y_dev) ||
        llz_refuse_device_overlap(who, "e", e, bytes, e_dev, "y", y, ybytes, y_dev))
        return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_x = (const float *)llz_stage_in(&f->st_x, x, bytes, x_dev, f->stream, &rc);
    const float *d_d = (const float *)llz_stage_in(&f->st_d, d, bytes, d_dev, f->stream, &rc);
    float *d_e = (float *)llz_stage_out(&f->st_e, e, bytes, e_dev, &rc);
    float *d_y = y ? (float *)llz_stage_out(&f->st_y, y, bytes, y_dev, &rc) : NULL;
    const int nblk = frame_len / f->block;
    for (int j = 0; j < nblk && rc == LLZ_OK; j++) {
        const int slot = (f->head + j) % f->R;
        rc = llzs_fir_adapt_filter_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_prev, f->d_g, f->d_mu, f->delta, d_x,
                                       d_d, d_e, d_y, f->channels, nblk, j, frame_len, f->P, f->R, slot, f->stream);
        if (rc == LLZ_OK && f->adapting)
            rc = llzs_fir_adapt_update_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_g, f->d_mu, f->channels, f->P,
                                           f->R, slot, f->stream);
    }
    if (rc == LLZ_OK) f->head = (f->head + nblk) % f->R;
    if (rc == LLZ_OK && !e_dev) rc = llzs_d2h(e, d_e, bytes, f->stream);
    if (rc == LLZ_OK && y && !y_dev) rc = llzs_d2h(y, d_y, bytes, f->stream);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_adapt_mc(unsigned long h, const float *x, const float *d, float *e, float *y, int frame_len)
{
    if (!LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT) || !x || !d || !e) {
        llzs_set_error("llz_adapt_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    adpt_t *f = (adpt_t *)h;
    const int prev = llzs_device_enter(f->device);
    const int rc = adpt_process(f, x, d, e, y, frame_len);
    llzs_device_leave(prev);
    return rc;
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static adpt_t *adpt_range(unsigned long h, const char *who, int first, int count, const void *buf)
{
    if (!LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT) || !buf) {
        llzs_set_error("%s: bad handle or NULL buffer", who);
        return NULL;
    }
    adpt_t *f = (adpt_t *)h;
    if (first < 0 || count < 1 || first >= f->channels || count > f->channels - first) {
        llzs_set_error("%s: channels [%d, %d + %d) outside the handle's [0, %d)", who, first, first, count, f->channels);
        return NULL;
    }
    return f;
}

int llz_adapt_mc_set_step(unsigned long h, int first, int count, const float *mu)
{
    const char *who = "llz_adapt_mc_set_step";
    adpt_t *f = adpt_range(h, who, first, count, mu);
    if (!f) return LLZ_ERR_ARG;
    for (int c = 0; c < count; c++)
        if (!adpt_mu_ok(mu[c])) {
            llzs_set_error("%s: mu %g of channel %d outside 0..2", who, (double)mu[c], first + c);
            return LLZ_ERR_ARG;
        }
    const int prev = llzs_device_enter(f->device);
    const int rc = llzs_h2d(f->d_mu + first, mu, sizeof(float) * (size_t)count, f->stream);      /* behind the calls already issued */
    if (rc == LLZ_OK) {
        memcpy(f->h_mu + first, mu, sizeof(float) * (size_t)count);
        f->adapting = 0;
        for (int c = 0; c < f->channels; c++) f->adapting += f->h_mu[c] != 0.f;
    }
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_mc_set_taps(unsigned long h, int first, int count, const float *taps)
{
    const char *who = "llz_adapt_mc_set_taps";
    adpt_t *f = adpt_range(h, who, first, count, taps);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const size_t row = adpt_row(f);
    const int rc = llz_host_load_spectra(who, f->d_w + (size_t)first * row, row, count, taps, f->flt_len, 2 * f->block, 1, 0,
                                         f->stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_mc_get_taps(unsigned long h, int first, int count, float *taps)
{
    const char *who = "llz_adapt_mc_get_taps";
    adpt_t *f = adpt_range(h, who, first, count, taps);
    if (!f) return LLZ_ERR_ARG;
    const int B = f->block, N = 2 * B;
    const size_t row = adpt_row(f);
    size_t chunk = ADPT_STAGE_BYTES / (sizeof(float) * row);
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)count) chunk = (size_t)count;
    float *hw = (float *)malloc(sizeof(float) * row * chunk);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N), *z = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (hw && cs && z) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc != LLZ_OK) llzs_set_error("%s: no host memory for %zu B of weight spectra", who, sizeof(float) * row * chunk);
    if (rc == LLZ_OK) llz_host_cs_table(cs, N);
    const int prev = llzs_device_enter(f->device);
    for (size_t r0 = 0; r0 < (size_t)count && rc == LLZ_OK; r0 += chunk) {
        const size_t rows = (size_t)count - r0 < chunk ? (size_t)count - r0 : chunk;
        rc = llzs_d2h(hw, f->d_w + ((size_t)first + r0) * row, sizeof(float) * row * rows, f->stream);
        for (size_t r = 0; r < rows && rc == LLZ_OK; r++)
            for (int p = 0; p < f->P; p++) {
                const long left = (long)f->flt_len - (long)p * B;
                llz_host_stream_taps(taps + (r0 + r) * (size_t)f->flt_len + (size_t)p * B, left < B ? (int)left : B,
                                     hw + r * row + 2 * (size_t)p * B, B, cs, z);
            }
    }
    llzs_device_leave(prev);
    free(hw); free(cs); free(z);
    return rc;
}

int llz_adapt_mc_reset(unsigned long h, int clear_taps)
{
    if (!LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT)) {
        llzs_set_error("llz_adapt_mc_reset: bad handle");
        return LLZ_ERR_ARG;
    }
    adpt_t *f = (adpt_t *)h;
    const int prev = llzs_device_enter(f->device);
    int rc = adpt_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = adpt_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_mc_plan(unsigned long h, int out[4])
{
    if (!LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT) || !out) {
        llzs_set_error("llz_adapt_mc_plan: bad handle or no out");
        return LLZ_ERR_ARG;
    }
    const adpt_t *f = (const adpt_t *)h;
    out[0] = 2 * f->block; out[1] = f->P; out[2] = f->R; out[3] = f->k;
    return LLZ_OK;
}

int llz_adapt_mc_set_stream(unsigned long h, void *stream)
{
    if (!LLZ_HANDLE_OK(h, adpt_t, LLZ_TAG_ADPT)) {
        llzs_set_error("llz_adapt_mc_set_stream: bad handle");
        return LLZ_ERR_ARG;
    }
    ((adpt_t *)h)->stream = stream;
    return LLZ_OK;
}
