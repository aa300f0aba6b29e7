/* llz_adapt_core.c -- what the two adaptive handles share (llz_adapt_host.c: llz_adapt_mc; llz_adapt_matrix_host.c:
 * llz_adapt_matrix_mc), declared in llz_host.h: the refusals of an init behind the port counts, the step sizes with their host
 * copy, get_taps from a run of weight rows, and the staged call around the launches.  The delay lines (ring, last block, head)
 * are each handle's own: the two differ there. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"

#define ADAPT_MIN_BLOCK 64
#define ADAPT_MAX_BLOCK 2048
#define ADAPT_STAGE_BYTES ((size_t)8 << 20)     /* host staging of get_taps: whole rows up to this, one row at least */

static int adapt_mu_ok(float mu) { return mu >= 0.f && mu <= 2.f; }                            /* a NaN fails both */

int llz_adapt_refuse_mu(const char *who, float mu)
{
    if (adapt_mu_ok(mu)) return 0;
    llzs_set_error("%s: mu %g outside 0..2", who, (double)mu);
    return 1;
}

int llz_adapt_refuse_delta(const char *who, float delta)
{
    if (delta > 0.f && isfinite(delta)) return 0;                                               /* a NaN fails the first */
    llzs_set_error("%s: delta %g is not a finite value above 0", who, (double)delta);
    return 1;
}

int llz_adapt_refuse(const char *who, int block, int frame_len, int max_blocks, int flt_len, float mu, float delta)
{
    if (block == 4096) {
        llzs_set_error("%s: block 4096 is not built (a thread would own 16 bins: no registers left); blocks are %d..%d", who,
                       ADAPT_MIN_BLOCK, ADAPT_MAX_BLOCK);
        return 1;
    }
    if (block < ADAPT_MIN_BLOCK || block > ADAPT_MAX_BLOCK || (block & (block - 1))) {
        llzs_set_error("%s: block %d is not a power of two in %d..%d", who, block, ADAPT_MIN_BLOCK, ADAPT_MAX_BLOCK);
        return 1;
    }
    if (frame_len < block || frame_len % block || (max_blocks && frame_len / block > max_blocks)) {
        if (max_blocks)
            llzs_set_error("%s: frame_len %d is not k x block with k in 1..%d (block %d)", who, frame_len, max_blocks, block);
        else
            llzs_set_error("%s: frame_len %d is not k x block with k >= 1 (block %d)", who, frame_len, block);
        return 1;
    }
    if (flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("%s: flt_len %d outside 1..%d", who, flt_len, LLZS_FIR_PART_MAX_TAPS);
        return 1;
    }
    return llz_adapt_refuse_mu(who, mu) || llz_adapt_refuse_delta(who, delta);
}

int llz_adapt_steps_create(llz_adapt_steps_t *s, const char *who, int count, float mu)
{
    const size_t bytes = sizeof(float) * (size_t)count;
    s->h_mu = (float *)malloc(bytes);
    if (!s->h_mu) {
        llzs_set_error("%s: no host memory for %zu B of step sizes", who, bytes);
        return LLZ_ERR_NOMEM;
    }
    for (int r = 0; r < count; r++) s->h_mu[r] = mu;
    s->count = count;
    s->adapting = mu != 0.f ? count : 0;
    s->d_mu = (float *)llzs_malloc(bytes);
    return s->d_mu ? llzs_h2d(s->d_mu, s->h_mu, bytes, NULL) : LLZ_OK;
}

void llz_adapt_steps_destroy(llz_adapt_steps_t *s)
{
    llzs_free(s->d_mu);
    free(s->h_mu);
    s->d_mu = s->h_mu = NULL;
}

int llz_adapt_steps_set(llz_adapt_steps_t *s, const char *who, const char *noun, int first, int count, const float *mu,
                        void *stream)
{
    for (int r = 0; r < count; r++)
        if (!adapt_mu_ok(mu[r])) {
            llzs_set_error("%s: mu %g of %s %d outside 0..2", who, (double)mu[r], noun, first + r);
            return LLZ_ERR_ARG;
        }
    const int rc = llzs_h2d(s->d_mu + first, mu, sizeof(float) * (size_t)count, stream);         /* behind the calls already issued */
    if (rc == LLZ_OK) {
        memcpy(s->h_mu + first, mu, sizeof(float) * (size_t)count);
        s->adapting = 0;
        for (int r = 0; r < s->count; r++) s->adapting += s->h_mu[r] != 0.f;
    }
    return rc;
}

int llz_adapt_get_taps(const char *who, float *taps, const float *d_w, int count, int block, int flt_len, void *stream)
{
    const int B = block, N = 2 * B, P = (flt_len + B - 1) / B;
    const size_t row = 2 * (size_t)P * (size_t)B;
    size_t chunk = ADAPT_STAGE_BYTES / (sizeof(float) * row);
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)count) chunk = (size_t)count;
    float *hw = (float *)malloc(sizeof(float) * row * chunk);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N), *z = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (hw && cs && z) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc != LLZ_OK) llzs_set_error("%s: no host memory for %zu B of weight spectra", who, sizeof(float) * row * chunk);
    if (rc == LLZ_OK) llz_host_cs_table(cs, N);
    for (size_t r0 = 0; r0 < (size_t)count && rc == LLZ_OK; r0 += chunk) {
        const size_t rows = (size_t)count - r0 < chunk ? (size_t)count - r0 : chunk;
        rc = llzs_d2h(hw, d_w + r0 * row, sizeof(float) * row * rows, stream);
        for (size_t r = 0; r < rows && rc == LLZ_OK; r++)
            for (int p = 0; p < P; p++) {
                const long left = (long)flt_len - (long)p * B;
                llz_host_stream_taps(taps + (r0 + r) * (size_t)flt_len + (size_t)p * B, left < B ? (int)left : B,
                                     hw + r * row + 2 * (size_t)p * B, B, cs, z);
            }
    }
    free(hw); free(cs); free(z);
    return rc;
}

int llz_adapt_io_begin(llz_adapt_io_t *io, const char *who, const float *x, size_t xbytes, const float *d, float *e, float *y,
                       size_t bytes, void *stream)
{
    if ((const float *)e == x || (const float *)e == d || (y && ((const float *)y == x || (const float *)y == d || y == e))) {
        llzs_set_error("%s: in-place filtering is not supported: e and y may not be x, d or each other", who);
        return LLZ_ERR_ARG;
    }
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
    io->x = (const float *)llz_stage_in(&io->st_x, x, xbytes, x_dev, stream, &rc);
    io->d = (const float *)llz_stage_in(&io->st_d, d, bytes, d_dev, stream, &rc);
    io->e = (float *)llz_stage_out(&io->st_e, e, bytes, e_dev, &rc);
    io->y = y ? (float *)llz_stage_out(&io->st_y, y, bytes, y_dev, &rc) : NULL;
    io->user_e = e_dev ? NULL : e;
    io->user_y = y && !y_dev ? y : NULL;
    io->bytes = bytes;
    return rc;
}

int llz_adapt_io_end(llz_adapt_io_t *io, int rc, void *stream)
{
    if (rc == LLZ_OK && io->user_e) rc = llzs_d2h(io->user_e, io->e, io->bytes, stream);
    if (rc == LLZ_OK && io->user_y) rc = llzs_d2h(io->user_y, io->y, io->bytes, stream);
    return rc;
}

void llz_adapt_io_release(llz_adapt_io_t *io)
{
    llz_stage_release(&io->st_x); llz_stage_release(&io->st_d); llz_stage_release(&io->st_e); llz_stage_release(&io->st_y);
}
