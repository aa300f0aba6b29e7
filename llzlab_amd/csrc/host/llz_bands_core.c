/* llz_bands_core.c -- what the five per-band handles share (llz_adapt_bands_host.c: llz_adapt_bands_mc;
 * llz_adapt_bands_matrix_host.c: llz_adapt_bands_matrix_mc; llz_kalman_bands_host.c: llz_kalman_bands_mc;
 * llz_kalman_bands_matrix_host.c: llz_kalman_bands_matrix_mc; llz_suppress_bands_host.c: llz_suppress_bands_mc), declared in
 * llz_host.h: the refusal of a count outside its range, the
 * refusals of a call behind its handle, the staged call around the one launch, the frame counter, the range check and the copies
 * of the set_* and get_* calls, the zeroing of a re / im pair and the upload of a flag array.  Every message here exists once.
 * The state itself, the init with its allocation message and the arguments of the launch are each handle's own. */
#include <stdlib.h>
#include "llz_host.h"

int llz_bands_refuse_count(const char *who, const char *name, int value, int lowest, int highest)
{
    if (value >= lowest && value <= highest) return 0;
    llzs_set_error("%s: %s %d outside %d..%d", who, name, value, lowest, highest);
    return 1;
}

int llz_bands_refuse_call(const char *who, int frames, int bins, const float *yre, const float *yim)
{
    if (frames < 0 || (long long)frames * bins > 2147483647LL) {
        llzs_set_error("%s: frames %d outside 0..%d (frames x bins below 2^31, bins %d)", who, frames, 2147483647 / bins, bins);
        return 1;
    }
    if (!yre != !yim) {
        llzs_set_error("%s: yre and yim must both be NULL or both be set", who);
        return 1;
    }
    return 0;
}

static int bands_refuse_null(const char *who, const void *a, const void *b)
{
    if (a && b) return 0;
    llzs_set_error("%s: NULL buffer", who);
    return 1;
}

int llz_bands_begin(llz_bands_t *f, const char *who, const llz_bands_buf_t *b, int count, int inputs, int split)
{
    llz_bands_io_t *io = &f->io;
    io->count = count; io->inputs = inputs; io->entered = 0;
    for (int k = 0; k < count; k++) {
        io->dev[k] = io->back[k] = NULL;
        io->bytes[k] = b[k].bytes;
        if (!b[k].optional && bands_refuse_null(who, b[k].user, b[k].user)) return LLZ_ERR_ARG;
    }
    io->prev = llzs_device_enter(f->head.device);
    io->entered = 1;
    int on_dev[LLZ_BANDS_MAX_BUFS] = { 0 }, nbuf = 0, rc = LLZ_OK;
    for (int k = 0; k < count && rc == LLZ_OK; k++)
        if (b[k].user && (on_dev[k] = llzs_is_device_ptr(b[k].user)) < 0) rc = LLZ_ERR_ARG;    /* a buffer of another GPU: message set */
    /* every output against every input and every output in front of it, before anything is staged or launched */
    for (int o = inputs; o < count && rc == LLZ_OK; o++)
        for (int i = 0; i < o && rc == LLZ_OK; i++)
            if (b[o].user && b[i].user)
                rc = llz_refuse_device_overlap(who, b[i].name, b[i].user, b[i].bytes, on_dev[i], b[o].name, b[o].user, b[o].bytes,
                                               on_dev[o]);
    for (int k = 0; k < count; k++) {
        if (!b[k].user) continue;
        nbuf++;
        io->dev[k] = k < inputs ? (void *)llz_stage_in(&io->st[k], b[k].user, b[k].bytes, on_dev[k], f->head.stream, &rc)
                                : llz_stage_out(&io->st[k], (void *)b[k].user, b[k].bytes, on_dev[k], &rc);
        if (k >= inputs && !on_dev[k]) io->back[k] = (void *)b[k].user;
    }
    if (rc == LLZ_ERR_NOMEM) {
        if (split) llzs_set_error("%s: no device memory to stage %d buffers of %zu B (x) and %zu B", who, nbuf, b[0].bytes, b[split].bytes);
        else llzs_set_error("%s: no device memory to stage %d buffers of %zu B", who, nbuf, b[0].bytes);
    }
    return rc;
}

int llz_bands_end(llz_bands_t *f, int rc, int frames)
{
    llz_bands_io_t *io = &f->io;
    if (!io->entered) return rc;
    if (rc == LLZ_OK) f->frames += frames;
    for (int o = io->inputs; o < io->count && rc == LLZ_OK; o++)
        if (io->back[o]) rc = llzs_d2h(io->back[o], io->dev[o], io->bytes[o], f->head.stream);
    llzs_device_leave(io->prev);
    return rc == LLZ_OK ? frames : rc;
}

void llz_bands_release(llz_bands_t *f)
{
    for (int k = 0; k < LLZ_BANDS_MAX_BUFS; k++) llz_stage_release(&f->io.st[k]);
}

void *llz_bands_out(unsigned long h, int tag, const char *who, const void *out)
{
    void *f = llz_handle(h, tag, who);
    if (f && !out) {
        llzs_set_error("%s: no out", who);
        return NULL;
    }
    return f;
}

int llz_bands_frames(unsigned long h, int tag, const char *who, long long *out)
{
    const llz_bands_t *f = (const llz_bands_t *)llz_bands_out(h, tag, who, out);
    if (!f) return LLZ_ERR_ARG;
    *out = f->frames;
    return LLZ_OK;
}

int llz_bands_refuse_range(const char *who, const char *noun, int first, int count, int have, const void *a, const void *b)
{
    if (bands_refuse_null(who, a, b)) return 1;
    if (first < 0 || count < 1 || first >= have || count > have - first) {
        llzs_set_error("%s: %s [%d, %d + %d) outside the handle's [0, %d)", who, noun, first, first, count, have);
        return 1;
    }
    return 0;
}

int llz_bands_copy(const llz_bands_t *f, void *d_state, size_t row_bytes, int first, int count, const void *src, void *dst)
{
    char *d = (char *)d_state + (size_t)first * row_bytes;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = src ? llzs_h2d(d, src, (size_t)count * row_bytes, f->head.stream)          /* behind the calls already issued */
                       : llzs_d2h(dst, d, (size_t)count * row_bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_bands_copy_pair(const llz_bands_t *f, float *const d_state[2], size_t row, int first, int count, const float *src_re,
                        const float *src_im, float *dst_re, float *dst_im)
{
    const int rc = llz_bands_copy(f, d_state[0], sizeof(float) * row, first, count, src_re, dst_re);
    return rc == LLZ_OK ? llz_bands_copy(f, d_state[1], sizeof(float) * row, first, count, src_im, dst_im) : rc;
}

int llz_bands_zero_pair(float *const d[2], size_t count, void *stream)
{
    const int rc = llzs_memset(d[0], 0, sizeof(float) * count, stream);
    return rc == LLZ_OK ? llzs_memset(d[1], 0, sizeof(float) * count, stream) : rc;
}

int llz_bands_flags(const llz_bands_t *f, const char *who, const char *what, int *d_flags, int first, int count, const int *on)
{
    const size_t bytes = sizeof(int) * (size_t)count;
    int *flags = (int *)malloc(bytes);
    if (!flags) {
        llzs_set_error("%s: no host memory for %zu B of %s", who, bytes, what);
        return LLZ_ERR_NOMEM;
    }
    for (int c = 0; c < count; c++) flags[c] = on ? on[c] != 0 : 1;
    const int rc = llz_bands_copy(f, d_flags, sizeof(int), first, count, flags, NULL);
    free(flags);
    return rc;
}
