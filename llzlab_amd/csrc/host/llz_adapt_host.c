/* llz_adapt_host.c -- include/llz_adapt.h: llz_adapt_mc, the partitioned frequency-domain NLMS adaptive filter (kernel K4h,
 * fir_adapt.hip).  Its own handle and tag.  What it shares with the stream convolver (llz_fir_stream_host.c) it takes from the
 * same places: the split-twiddle table (llz_host_stream_twiddles) and the builder of the packed spectra for set_taps
 * (llz_host_load_spectra).  What it shares with llz_adapt_matrix_mc is llz_adapt_core.c's: the init's refusals, the step sizes
 * with their host copy, get_taps and the staged call.  The delay line lives here: the ring's head goes by value with each
 * launch, and a call launches no update while every channel is frozen. */
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt.h"

typedef struct {
    int tag;                    /* LLZ_TAG_ADPT */
    int device;
    int channels, block, frame_len, flt_len;
    int k, P, R;                /* blocks per call of the init's frame_len, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes */
    float delta;
    llz_adapt_steps_t mu;       /* [channels]: the step sizes */
    float *d_w;                 /* [channels][P][block] complex: the weights' packed spectra */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [channels][R][block] complex */
    float *d_prev;              /* [channels][block]: the last input block */
    float *d_g;                 /* [channels][block] complex: the normalised gradient of the block in flight */
    void *stream;
    llz_adapt_io_t io;
} adpt_t;

static void adpt_destroy(adpt_t *f)
{
    if (!f) return;
    llzs_free(f->d_w); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev); llzs_free(f->d_g);
    llz_adapt_steps_destroy(&f->mu);
    llz_adapt_io_release(&f->io);
    f->tag = 0;
    free(f);
}

static size_t adpt_row(const adpt_t *f) { return 2 * (size_t)f->P * (size_t)f->block; }       /* floats of a channel's spectra */

static int adpt_refuse(const char *who, int channels, int block, int frame_len, int flt_len, float mu, float delta)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    return llz_adapt_refuse(who, block, frame_len, 0, flt_len, mu, delta);
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
    int rc = llz_adapt_steps_create(&f->mu, who, channels, mu);
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
        if (!f->d_tw || !f->d_prev || !f->d_g || !f->mu.d_mu) {
            llzs_set_error("%s: no device memory for the twiddles, the last input blocks, the gradient and the step sizes: %zu B, "
                           "%zu B, %zu B and %zu B asked for", who, tbytes, pbytes, 2 * pbytes, mbytes);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, f->block);
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
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len;
    llz_adapt_io_t *io = &f->io;
    int rc = llz_adapt_io_begin(io, who, x, bytes, d, e, y, bytes, f->stream);
    const int nblk = frame_len / f->block;
    for (int j = 0; j < nblk && rc == LLZ_OK; j++) {
        const int slot = (f->head + j) % f->R;
        rc = llzs_fir_adapt_filter_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_prev, f->d_g, f->mu.d_mu, f->delta,
                                       io->x, io->d, io->e, io->y, f->channels, nblk, j, frame_len, f->P, f->R, slot, f->stream);
        if (rc == LLZ_OK && f->mu.adapting)
            rc = llzs_fir_adapt_update_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_g, f->mu.d_mu, f->channels,
                                           f->P, f->R, slot, f->stream);
    }
    if (rc == LLZ_OK) f->head = (f->head + nblk) % f->R;
    rc = llz_adapt_io_end(io, rc, f->stream);
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
    const int prev = llzs_device_enter(f->device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "channel", first, count, mu, f->stream);
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
    const int prev = llzs_device_enter(f->device);
    const int rc = llz_adapt_get_taps(who, taps, f->d_w + (size_t)first * adpt_row(f), count, f->block, f->flt_len, f->stream);
    llzs_device_leave(prev);
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
