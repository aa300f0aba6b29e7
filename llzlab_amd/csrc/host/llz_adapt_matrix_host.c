/* llz_adapt_matrix_host.c -- include/llz_adapt_matrix.h: llz_adapt_matrix_mc, the multi-reference frequency-domain NLMS adaptive
 * filter (kernels K4i, fir_adapt_matrix.hip, on K4g's forward and product launches, fir_matrix.hip).  Its own handle and tag.
 * The delay lines are the matrix convolver's (llz_fir_matrix_host.c: a ring per input, the last input block double-buffered)
 * and the input groups of the product come from the same function (llz_host_matrix_groups), so a frozen handle has that
 * convolver's bits; the twiddles and the builder of the packed spectra are the shared ones (llz_spectra.c).  What it shares
 * with llz_adapt_mc is llz_adapt_core.c's: the init's refusals, the step sizes with their host copy, get_taps and the staged
 * call.  The delay lines live here: the slot goes by value with each launch, and a call launches no power and no update while
 * every output is frozen. */
#include <stdlib.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_matrix.h"

#define ADPX_MAX_PORTS 4096                     /* inputs, outputs */
#define ADPX_MAX_BLOCKS 65535                   /* blocks of a call: a grid dimension of the forward launch */

typedef struct {
    int tag;                    /* LLZ_TAG_ADPX */
    int device;
    int inputs, outputs, block, frame_len, flt_len;
    int k, P, R;                /* blocks per call of the init's frame_len, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes */
    int cur;                    /* d_prev[cur] holds the last input block; a call writes the other and swaps */
    int G, gsize;               /* input groups of the product, inputs per group: llz_fir_matrix_mc's */
    float delta;
    llz_adapt_steps_t mu;       /* [outputs]: the step sizes */
    float *d_w;                 /* [outputs][inputs][P][block] complex: the weights' packed spectra */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [inputs][R][block] complex */
    float *d_prev[2];           /* [inputs][block]: the last input block, double-buffered */
    float *d_y;                 /* [G][outputs][block] complex: the groups' partial spectra of the block in flight */
    float *d_den;               /* [k][block] pairs: the denominators D + delta of a call's blocks */
    float *d_g;                 /* [outputs][block] complex: the normalised gradient of the block in flight */
    unsigned char *d_conn;      /* [outputs][inputs] ones: every path is connected */
    void *stream;
    llz_adapt_io_t io;
} adpx_t;

static void adpx_destroy(adpx_t *f)
{
    if (!f) return;
    llzs_free(f->d_w); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev[0]); llzs_free(f->d_prev[1]);
    llzs_free(f->d_y); llzs_free(f->d_den); llzs_free(f->d_g); llzs_free(f->d_conn);
    llz_adapt_steps_destroy(&f->mu);
    llz_adapt_io_release(&f->io);
    f->tag = 0;
    free(f);
}

static size_t adpx_row(const adpx_t *f) { return 2 * (size_t)f->P * (size_t)f->block; }       /* floats of a path's spectra */

static int adpx_refuse(const char *who, int inputs, int outputs, int block, int frame_len, int flt_len, float mu, float delta)
{
    if (inputs < 1 || inputs > ADPX_MAX_PORTS) {
        llzs_set_error("%s: inputs %d outside 1..%d", who, inputs, ADPX_MAX_PORTS);
        return 1;
    }
    if (outputs < 1 || outputs > ADPX_MAX_PORTS) {
        llzs_set_error("%s: outputs %d outside 1..%d", who, outputs, ADPX_MAX_PORTS);
        return 1;
    }
    return llz_adapt_refuse(who, block, frame_len, ADPX_MAX_BLOCKS, flt_len, mu, delta);
}

/* zeros in the delay lines (rings and last blocks), ordered on the handle's stream */
static int adpx_clear(adpx_t *f)
{
    const size_t pbytes = sizeof(float) * (size_t)f->inputs * (size_t)f->block;
    int rc = llzs_memset(f->d_ring, 0, sizeof(float) * 2 * (size_t)f->inputs * (size_t)f->R * (size_t)f->block, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev[0], 0, pbytes, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev[1], 0, pbytes, f->stream);
    f->head = 0;
    f->cur = 0;
    return rc;
}

static int adpx_clear_taps(adpx_t *f)
{
    return llzs_memset(f->d_w, 0, sizeof(float) * (size_t)f->outputs * (size_t)f->inputs * adpx_row(f), f->stream);
}

unsigned long llz_adapt_matrix_mc_init(int inputs, int outputs, int block, int frame_len, int flt_len, float mu, float delta)
{
    const char *who = "llz_adapt_matrix_mc_init";
    if (adpx_refuse(who, inputs, outputs, block, frame_len, flt_len, mu, delta)) return LLZ_BAD_HANDLE;
    adpx_t *f = (adpx_t *)calloc(1, sizeof(*f));
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->tag = LLZ_TAG_ADPX;
    f->device = llzs_device_get();
    f->inputs = inputs; f->outputs = outputs; f->block = block; f->frame_len = frame_len; f->flt_len = flt_len; f->delta = delta;
    f->k = frame_len / block;
    f->P = (flt_len + block - 1) / block;
    f->R = f->P + f->k - 1;
    llz_host_matrix_groups(inputs, outputs, block, &f->G, &f->gsize);
    const size_t paths = (size_t)outputs * (size_t)inputs;
    const size_t wbytes = sizeof(float) * paths * adpx_row(f);
    const size_t rbytes = sizeof(float) * 2 * (size_t)inputs * (size_t)f->R * (size_t)block;
    const size_t tbytes = sizeof(float) * 2 * ((size_t)block / 2 + (size_t)block);
    const size_t pbytes = sizeof(float) * (size_t)inputs * (size_t)block;
    const size_t gbytes = sizeof(float) * 2 * (size_t)outputs * (size_t)block, ybytes = gbytes * (size_t)f->G;
    const size_t dbytes = sizeof(float) * 2 * (size_t)f->k * (size_t)block, mbytes = sizeof(float) * (size_t)outputs;
    int rc = llz_adapt_steps_create(&f->mu, who, outputs, mu);
    if (rc == LLZ_OK && !(f->d_w = (float *)llzs_malloc(wbytes))) {
        llzs_set_error("%s: no device memory for the weights' spectra: %zu B asked for (%d outputs x %d inputs x %d partitions x %d "
                       "bins)", who, wbytes, outputs, inputs, f->P, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_ring = (float *)llzs_malloc(rbytes))) {
        llzs_set_error("%s: no device memory for the delay lines: %zu B asked for (%d inputs x %d slots x %d bins)", who, rbytes,
                       inputs, f->R, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_y = (float *)llzs_malloc(ybytes))) {
        llzs_set_error("%s: no device memory for the partial spectra: %zu B asked for (%d groups x %d outputs x %d bins)", who,
                       ybytes, f->G, outputs, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_den = (float *)llzs_malloc(dbytes))) {
        llzs_set_error("%s: no device memory for the power of a call's blocks: %zu B asked for (%d blocks x %d bins)", who, dbytes,
                       f->k, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) {
        f->d_tw = (float *)llzs_malloc(tbytes);
        f->d_prev[0] = (float *)llzs_malloc(pbytes);
        f->d_prev[1] = (float *)llzs_malloc(pbytes);
        f->d_g = (float *)llzs_malloc(gbytes);
        f->d_conn = (unsigned char *)llzs_malloc(paths);
        if (!f->d_tw || !f->d_prev[0] || !f->d_prev[1] || !f->d_g || !f->mu.d_mu || !f->d_conn) {
            llzs_set_error("%s: no device memory for the twiddles, the last input blocks, the gradient, the step sizes and the "
                           "connection table: %zu B, 2 x %zu B, %zu B, %zu B and %zu B asked for", who, tbytes, pbytes, gbytes,
                           mbytes, paths);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, f->block);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_conn, 1, paths, f->stream);
    if (rc == LLZ_OK) rc = adpx_clear_taps(f);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_g, 0, gbytes, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_den, 0, dbytes, f->stream);
    if (rc == LLZ_OK) rc = adpx_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        adpx_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_adapt_matrix_mc_uninit(unsigned long h)
{
    if (LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX)) {
        adpx_t *f = (adpx_t *)h;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        adpx_destroy(f);
        llzs_device_leave(prev);
    }
}

static int adpx_process(adpx_t *f, const float *x, const float *d, float *e, float *y, int n)
{
    const char *who = "llz_adapt_matrix_mc";
    if (n < f->block || n > f->frame_len || n % f->block) {
        llzs_set_error("%s: n %d is not a multiple of block %d in %d..%d (the init's frame_len)", who, n, f->block, f->block,
                       f->frame_len);
        return LLZ_ERR_ARG;
    }
    const size_t xbytes = sizeof(float) * (size_t)f->inputs * (size_t)n, bytes = sizeof(float) * (size_t)f->outputs * (size_t)n;
    llz_adapt_io_t *io = &f->io;
    int rc = llz_adapt_io_begin(io, who, x, xbytes, d, e, y, bytes, f->stream);
    const int nblk = n / f->block, head = f->head;
    if (rc == LLZ_OK)
        rc = llzs_fir_matrix_fwd_f32(f->block, f->d_tw, f->d_ring, f->d_prev[f->cur], f->d_prev[f->cur ^ 1], io->x, f->inputs, nblk, 0,
                                     n, f->R, head, f->stream);
    if (rc == LLZ_OK) {
        /* the delay lines have moved on, whatever becomes of the rest of the call */
        f->head = (head + nblk) % f->R;
        f->cur ^= 1;
        if (f->mu.adapting)
            rc = llzs_fir_adapt_matrix_power_f32(f->block, f->flt_len, f->d_ring, f->d_den, f->delta, f->inputs, nblk, f->P, f->R,
                                                 head, f->stream);
    }
    for (int j = 0; j < nblk && rc == LLZ_OK; j++) {
        const int slot = (head + j) % f->R;
        rc = llzs_fir_matrix_mac_f32(f->block, f->d_w, f->d_ring, f->d_conn, f->d_y, f->inputs, f->outputs, 1, 0, 0, f->P, f->R,
                                     slot, f->G, f->gsize, f->stream);
        if (rc == LLZ_OK)
            rc = llzs_fir_adapt_matrix_error_f32(f->block, f->d_y, f->d_tw, f->d_den + 2 * (size_t)j * (size_t)f->block, f->d_g,
                                                 f->mu.d_mu, io->d, io->e, io->y, f->outputs, f->G, j, n, f->stream);
        if (rc == LLZ_OK && f->mu.adapting)
            rc = llzs_fir_adapt_matrix_update_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_g, f->mu.d_mu, f->inputs,
                                                  f->outputs, f->P, f->R, slot, f->stream);
    }
    rc = llz_adapt_io_end(io, rc, f->stream);
    return rc == LLZ_OK ? n : rc;
}

int llz_adapt_matrix_mc(unsigned long h, const float *x, const float *d, float *e, float *y, int n)
{
    if (!LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX) || !x || !d || !e) {
        llzs_set_error("llz_adapt_matrix_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    adpx_t *f = (adpx_t *)h;
    const int prev = llzs_device_enter(f->device);
    const int rc = adpx_process(f, x, d, e, y, n);
    llzs_device_leave(prev);
    return rc;
}

/* the handle and a range of outputs and of inputs inside it, or NULL with a message naming who */
static adpx_t *adpx_range(unsigned long h, const char *who, int out_first, int out_count, int in_first, int in_count,
                          const void *buf)
{
    if (!LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX) || !buf) {
        llzs_set_error("%s: bad handle or NULL buffer", who);
        return NULL;
    }
    adpx_t *f = (adpx_t *)h;
    if (out_first < 0 || out_count < 1 || out_first >= f->outputs || out_count > f->outputs - out_first) {
        llzs_set_error("%s: outputs [%d, %d + %d) outside the handle's [0, %d)", who, out_first, out_first, out_count, f->outputs);
        return NULL;
    }
    if (in_first < 0 || in_count < 1 || in_first >= f->inputs || in_count > f->inputs - in_first) {
        llzs_set_error("%s: inputs [%d, %d + %d) outside the handle's [0, %d)", who, in_first, in_first, in_count, f->inputs);
        return NULL;
    }
    return f;
}

int llz_adapt_matrix_mc_set_step(unsigned long h, int out_first, int out_count, const float *mu)
{
    const char *who = "llz_adapt_matrix_mc_set_step";
    adpx_t *f = adpx_range(h, who, out_first, out_count, 0, 1, mu);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const int rc = llz_adapt_steps_set(&f->mu, who, "output", out_first, out_count, mu, f->stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, const float *taps)
{
    const char *who = "llz_adapt_matrix_mc_set_taps";
    adpx_t *f = adpx_range(h, who, out_first, out_count, in_first, in_count, taps);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const size_t row = adpx_row(f);
    int rc = LLZ_OK;
    for (int o = 0; o < out_count && rc == LLZ_OK; o++) {
        const size_t first = (size_t)(out_first + o) * (size_t)f->inputs + (size_t)in_first;
        rc = llz_host_load_spectra(who, f->d_w + first * row, row, in_count, taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len,
                                   f->flt_len, 2 * f->block, 1, 0, f->stream);
    }
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *taps)
{
    const char *who = "llz_adapt_matrix_mc_get_taps";
    adpx_t *f = adpx_range(h, who, out_first, out_count, in_first, in_count, taps);
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    int rc = LLZ_OK;
    for (int o = 0; o < out_count && rc == LLZ_OK; o++) {
        const size_t first = (size_t)(out_first + o) * (size_t)f->inputs + (size_t)in_first;
        rc = llz_adapt_get_taps(who, taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len, f->d_w + first * adpx_row(f), in_count,
                                f->block, f->flt_len, f->stream);
    }
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_matrix_mc_reset(unsigned long h, int clear_taps)
{
    if (!LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX)) {
        llzs_set_error("llz_adapt_matrix_mc_reset: bad handle");
        return LLZ_ERR_ARG;
    }
    adpx_t *f = (adpx_t *)h;
    const int prev = llzs_device_enter(f->device);
    int rc = adpx_clear(f);
    if (rc == LLZ_OK && clear_taps) rc = adpx_clear_taps(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_adapt_matrix_mc_plan(unsigned long h, int out[6])
{
    if (!LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX) || !out) {
        llzs_set_error("llz_adapt_matrix_mc_plan: bad handle or no out");
        return LLZ_ERR_ARG;
    }
    const adpx_t *f = (const adpx_t *)h;
    out[0] = 2 * f->block; out[1] = f->P; out[2] = f->R; out[3] = f->k; out[4] = f->G; out[5] = f->gsize;
    return LLZ_OK;
}

int llz_adapt_matrix_mc_set_stream(unsigned long h, void *stream)
{
    if (!LLZ_HANDLE_OK(h, adpx_t, LLZ_TAG_ADPX)) {
        llzs_set_error("llz_adapt_matrix_mc_set_stream: bad handle");
        return LLZ_ERR_ARG;
    }
    ((adpx_t *)h)->stream = stream;
    return LLZ_OK;
}
