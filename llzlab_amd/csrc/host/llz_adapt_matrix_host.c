/* llz_adapt_matrix_host.c -- include/llz_adapt_matrix.h: llz_adapt_matrix_mc, the multi-reference frequency-domain NLMS adaptive
 * filter (kernels K4i, fir_adapt_matrix.hip, on K4g's forward and product launches, fir_matrix.hip).  Its own handle and tag.
 * The delay lines are the matrix convolver's (llz_fir_matrix_host.c: a ring per input, the last input block double-buffered)
 * and the input groups of the product come from the same function (llz_host_matrix_groups), so a frozen handle has that
 * convolver's bits; the twiddles, the builder of the packed spectra and its inverse, the staged call and the overlap refusal
 * are the shared ones (llz_spectra.c, llz_util.c).  The rings' head and the step sizes' host copy live here: the slot goes by
 * value with each launch, and a call launches no power and no update while every output is frozen. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"
#include "../../../include/llz_adapt_matrix.h"

#define ADPX_MIN_BLOCK 64
#define ADPX_MAX_BLOCK 2048
#define ADPX_MAX_PORTS 4096                     /* inputs, outputs */
#define ADPX_MAX_BLOCKS 65535                   /* blocks of a call: a grid dimension of the forward launch */
#define ADPX_STAGE_BYTES ((size_t)8 << 20)      /* host staging of get_taps: whole paths up to this, one path at least */

typedef struct {
    int tag;                    /* LLZ_TAG_ADPX */
    int device;
    int inputs, outputs, block, frame_len, flt_len;
    int k, P, R;                /* blocks per call of the init's frame_len, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes */
    int cur;                    /* d_prev[cur] holds the last input block; a call writes the other and swaps */
    int G, gsize;               /* input groups of the product, inputs per group: llz_fir_matrix_mc's */
    float delta;
    float *h_mu;                /* HOST [outputs]: the step sizes; d_mu is its device copy */
    int adapting;               /* outputs whose mu is not zero */
    float *d_w;                 /* [outputs][inputs][P][block] complex: the weights' packed spectra */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [inputs][R][block] complex */
    float *d_prev[2];           /* [inputs][block]: the last input block, double-buffered */
    float *d_y;                 /* [G][outputs][block] complex: the groups' partial spectra of the block in flight */
    float *d_den;               /* [k][block] pairs: the denominators D + delta of a call's blocks */
    float *d_g;                 /* [outputs][block] complex: the normalised gradient of the block in flight */
    float *d_mu;                /* [outputs] */
    unsigned char *d_conn;      /* [outputs][inputs] ones: every path is connected */
    void *stream;
    llz_stage_t st_x, st_d, st_e, st_y;
} adpx_t;

static void adpx_destroy(adpx_t *f)
{
    if (!f) return;
    llzs_free(f->d_w); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev[0]); llzs_free(f->d_prev[1]);
    llzs_free(f->d_y); llzs_free(f->d_den); llzs_free(f->d_g); llzs_free(f->d_mu); llzs_free(f->d_conn);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_d); llz_stage_release(&f->st_e); llz_stage_release(&f->st_y);
    free(f->h_mu);
    f->tag = 0;
    free(f);
}

static size_t adpx_row(const adpx_t *f) { return 2 * (size_t)f->P * (size_t)f->block; }       /* floats of a path's spectra */

static int adpx_mu_ok(float mu) { return mu >= 0.f && mu <= 2.f; }                             /* a NaN fails both */

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
    if (block == 4096) {
        llzs_set_error("%s: block 4096 is not built (a thread would own 16 bins: no registers left); blocks are %d..%d", who,
                       ADPX_MIN_BLOCK, ADPX_MAX_BLOCK);
        return 1;
    }
    if (block < ADPX_MIN_BLOCK || block > ADPX_MAX_BLOCK || (block & (block - 1))) {
        llzs_set_error("%s: block %d is not a power of two in %d..%d", who, block, ADPX_MIN_BLOCK, ADPX_MAX_BLOCK);
        return 1;
    }
    if (frame_len < block || frame_len % block || frame_len / block > ADPX_MAX_BLOCKS) {
        llzs_set_error("%s: frame_len %d is not k x block with k in 1..%d (block %d)", who, frame_len, ADPX_MAX_BLOCKS, block);
        return 1;
    }
    if (flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("%s: flt_len %d outside 1..%d", who, flt_len, LLZS_FIR_PART_MAX_TAPS);
        return 1;
    }
    if (!adpx_mu_ok(mu)) {
        llzs_set_error("%s: mu %g outside 0..2", who, (double)mu);
        return 1;
    }
    if (!(delta > 0.f) || !isfinite(delta)) {
        llzs_set_error("%s: delta %g is not a finite value above 0", who, (double)delta);
        return 1;
    }
    return 0;
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
    int rc = LLZ_OK;
    f->h_mu = (float *)malloc(mbytes);
    if (!f->h_mu) {
        llzs_set_error("%s: no host memory for %zu B of step sizes", who, mbytes);
        rc = LLZ_ERR_NOMEM;
    }
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
        f->d_mu = (float *)llzs_malloc(mbytes);
        f->d_conn = (unsigned char *)llzs_malloc(paths);
        if (!f->d_tw || !f->d_prev[0] || !f->d_prev[1] || !f->d_g || !f->d_mu || !f->d_conn) {
            llzs_set_error("%s: no device memory for the twiddles, the last input blocks, the gradient, the step sizes and the "
                           "connection table: %zu B, 2 x %zu B, %zu B, %zu B and %zu B asked for", who, tbytes, pbytes, gbytes,
                           mbytes, paths);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, f->block);
    if (rc == LLZ_OK) {
        for (int o = 0; o < outputs; o++) f->h_mu[o] = mu;
        f->adapting = mu != 0.f ? outputs : 0;
        rc = llzs_h2d(f->d_mu, f->h_mu, mbytes, NULL);
    }
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
    if ((const float *)e == x || (const float *)e == d || (y && ((const float *)y == x || (const float *)y == d || y == e))) {
        llzs_set_error("%s: in-place filtering is not supported: e and y may not be x, d or each other", who);
        return LLZ_ERR_ARG;
    }
    const size_t xbytes = sizeof(float) * (size_t)f->inputs * (size_t)n, bytes = sizeof(float) * (size_t)f->outputs * (size_t)n;
    const size_t ybytes = y ? bytes : 0;
    const int x_dev = llzs_is_device_ptr(x), d_dev = llzs_is_device_ptr(d), e_dev = llzs_is_device_ptr(e);
    const int y_dev = y ? llzs_is_device_ptr(y) : 0;
    if (x_dev < 0 || d_dev < 0 || e_dev < 0 || y_dev < 0) return LLZ_ERR_ARG;        /* a buffer of another GPU: message set */
    if (llz_refuse_device_overlap(who, "x", x, xbytes, x_dev, "e", e, bytes, e_dev) ||
        llz_refuse_device_overlap(who, "d", d, bytes, d_dev, "e", e, bytes, e_dev) ||
        llz_refuse_device_overlap(who, "x", x, xbytes, x_dev, "y", y, ybytes, y_dev) ||
        llz_refuse_device_overlap(who, "d", d, bytes, d_dev, "y", y, ybytes, y_dev) ||
        llz_refuse_device_overlap(who, "e", e, bytes, e_dev, "y", y, ybytes, y_dev))
        return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_x = (const float *)llz_stage_in(&f->st_x, x, xbytes, x_dev, f->stream, &rc);
    const float *d_d = (const float *)llz_stage_in(&f->st_d, d, bytes, d_dev, f->stream, &rc);
    float *d_e = (float *)llz_stage_out(&f->st_e, e, bytes, e_dev, &rc);
    float *d_y = y ? (float *)llz_stage_out(&f->st_y, y, bytes, y_dev, &rc) : NULL;
    const int nblk = n / f->block, head = f->head;
    if (rc == LLZ_OK)
        rc = llzs_fir_matrix_fwd_f32(f->block, f->d_tw, f->d_ring, f->d_prev[f->cur], f->d_prev[f->cur ^ 1], d_x, f->inputs, nblk, 0,
                                     n, f->R, head, f->stream);
    if (rc == LLZ_OK) {
        /* the delay lines have moved on, whatever becomes of the rest of the call */
        f->head = (head + nblk) % f->R;
        f->cur ^= 1;
        if (f->adapting)
            rc = llzs_fir_adapt_matrix_power_f32(f->block, f->flt_len, f->d_ring, f->d_den, f->delta, f->inputs, nblk, f->P, f->R,
                                                 head, f->stream);
    }
    for (int j = 0; j < nblk && rc == LLZ_OK; j++) {
        const int slot = (head + j) % f->R;
        rc = llzs_fir_matrix_mac_f32(f->block, f->d_w, f->d_ring, f->d_conn, f->d_y, f->inputs, f->outputs, 1, 0, 0, f->P, f->R,
                                     slot, f->G, f->gsize, f->stream);
        if (rc == LLZ_OK)
            rc = llzs_fir_adapt_matrix_error_f32(f->block, f->d_y, f->d_tw, f->d_den + 2 * (size_t)j * (size_t)f->block, f->d_g,
                                                 f->d_mu, d_d, d_e, d_y, f->outputs, f->G, j, n, f->stream);
        if (rc == LLZ_OK && f->adapting)
            rc = llzs_fir_adapt_matrix_update_f32(f->block, f->flt_len, f->d_w, f->d_tw, f->d_ring, f->d_g, f->d_mu, f->inputs,
                                                  f->outputs, f->P, f->R, slot, f->stream);
    }
    if (rc == LLZ_OK && !e_dev) rc = llzs_d2h(e, d_e, bytes, f->stream);
    if (rc == LLZ_OK && y && !y_dev) rc = llzs_d2h(y, d_y, bytes, f->stream);
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
    for (int o = 0; o < out_count; o++)
        if (!adpx_mu_ok(mu[o])) {
            llzs_set_error("%s: mu %g of output %d outside 0..2", who, (double)mu[o], out_first + o);
            return LLZ_ERR_ARG;
        }
    const int prev = llzs_device_enter(f->device);
    const int rc = llzs_h2d(f->d_mu + out_first, mu, sizeof(float) * (size_t)out_count, f->stream);   /* behind the calls issued */
    if (rc == LLZ_OK) {
        memcpy(f->h_mu + out_first, mu, sizeof(float) * (size_t)out_count);
        f->adapting = 0;
        for (int o = 0; o < f->outputs; o++) f->adapting += f->h_mu[o] != 0.f;
    }
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
    const int B = f->block, N = 2 * B;
    const size_t row = adpx_row(f);
    size_t chunk = ADPX_STAGE_BYTES / (sizeof(float) * row);
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)in_count) chunk = (size_t)in_count;
    float *hw = (float *)malloc(sizeof(float) * row * chunk);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N), *z = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (hw && cs && z) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc != LLZ_OK) llzs_set_error("%s: no host memory for %zu B of weight spectra", who, sizeof(float) * row * chunk);
    if (rc == LLZ_OK) llz_host_cs_table(cs, N);
    const int prev = llzs_device_enter(f->device);
    for (int o = 0; o < out_count && rc == LLZ_OK; o++) {
        const size_t first = (size_t)(out_first + o) * (size_t)f->inputs + (size_t)in_first;
        float *trow = taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len;
        for (size_t r0 = 0; r0 < (size_t)in_count && rc == LLZ_OK; r0 += chunk) {
            const size_t rows = (size_t)in_count - r0 < chunk ? (size_t)in_count - r0 : chunk;
            rc = llzs_d2h(hw, f->d_w + (first + r0) * row, sizeof(float) * row * rows, f->stream);
            for (size_t r = 0; r < rows && rc == LLZ_OK; r++)
                for (int p = 0; p < f->P; p++) {
                    const long left = (long)f->flt_len - (long)p * B;
                    llz_host_stream_taps(trow + (r0 + r) * (size_t)f->flt_len + (size_t)p * B, left < B ? (int)left : B,
                                         hw + r * row + 2 * (size_t)p * B, B, cs, z);
                }
        }
    }
    llzs_device_leave(prev);
    free(hw); free(cs); free(z);
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
