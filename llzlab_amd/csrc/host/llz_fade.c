/* llz_fade.c -- the crossfade state of the delay-line convolvers (llz_fir_xfade_stream_mc, llz_fir_xfade_matrix_mc) and its rules,
 * once: one fade at a time; rows join a pending fade only with the same fade_blocks, until its first block has run; set_taps is
 * refused with the blocks left; the new spectra live in a second buffer of the handle's own buffer's size; the rows in the fade
 * are marked in a byte table; when the fade is over the new rows are adopted on the stream behind the last faded block.  Generic
 * over "rows of spectra" -- tap rows for the stream handle, paths in [outputs][inputs] order for the matrix handle: the caller
 * passes `rows` and `row` (floats of one row's spectra) and the noun of its messages, and launches its own kernels with
 * fade.done / fade.blocks by value.  After the launch or launches of a call, or of a whole flush, the caller adds the blocks
 * launched to `done` and adopts at the end of the fade. */
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"

int llz_fade_left(const llz_fade_t *fd) { return fd->blocks ? fd->blocks - fd->done : 0; }

int llz_fade_refuse(const llz_fade_t *fd, const char *who, const char *noun, int fade_blocks)
{
    if (fade_blocks < 1 || fade_blocks > LLZ_FADE_MAX_BLOCKS) {
        llzs_set_error("%s: fade_blocks %d outside 1..%d", who, fade_blocks, LLZ_FADE_MAX_BLOCKS);
        return 1;
    }
    /* one fade at a time; until its first block has run, calls with the same length add or replace rows of it */
    if (fd->blocks && fd->done > 0) {
        llzs_set_error("%s: a fade is already in flight (%d of its %d blocks left)", who, llz_fade_left(fd), fd->blocks);
        return 1;
    }
    if (fd->blocks && fade_blocks != fd->blocks) {
        llzs_set_error("%s: a fade is already in flight (%d of its %d blocks left): %s join a pending fade only with the same "
                       "fade_blocks", who, llz_fade_left(fd), fd->blocks, noun);
        return 1;
    }
    return 0;
}

int llz_fade_refuse_set_taps(const llz_fade_t *fd, const char *who)
{
    if (!fd->blocks) return 0;
    llzs_set_error("%s: refused while a fade is in flight (%d of its %d blocks left)", who, llz_fade_left(fd), fd->blocks);
    return 1;
}

int llz_fade_reserve(llz_fade_t *fd, const char *who, const char *noun, size_t rows, size_t row)
{
    if (fd->d_new) return LLZ_OK;
    const size_t hbytes = sizeof(float) * row * rows;
    float *hn = (float *)llzs_malloc(hbytes);
    unsigned char *dr = (unsigned char *)llzs_malloc(rows);
    unsigned char *hr = (unsigned char *)calloc(rows, 1);
    if (!hn || !dr || !hr) {
        llzs_set_error("%s: no memory for the new taps' spectra: %zu B of device memory asked for (%zu %s x %zu bins) and %zu B for "
                       "the table of fading %s, on the device and on the host", who, hbytes, rows, noun, row / 2, rows, noun);
        llzs_free(hn); llzs_free(dr); free(hr);
        return LLZ_ERR_NOMEM;
    }
    fd->d_new = hn; fd->d_rows = dr; fd->h_rows = hr;
    return LLZ_OK;
}

int llz_fade_commit(llz_fade_t *fd, const unsigned char *table, size_t rows, int fade_blocks, void *stream)
{
    const int rc = llzs_h2d(fd->d_rows, table, rows, stream);
    if (rc != LLZ_OK) return rc;
    memcpy(fd->h_rows, table, rows);
    fd->blocks = fade_blocks;
    fd->done = 0;
    return LLZ_OK;
}

int llz_fade_adopt(llz_fade_t *fd, float **d_h, size_t rows, size_t row, void *stream)
{
    int rc = LLZ_OK, all = 1;
    for (size_t r = 0; r < rows; r++) all &= fd->h_rows[r];
    if (all) {
        float *t = *d_h;
        *d_h = fd->d_new;
        fd->d_new = t;
    } else {
        for (size_t r = 0; r < rows && rc == LLZ_OK;) {
            size_t e = r;
            while (e < rows && fd->h_rows[e] == fd->h_rows[r]) e++;
            if (fd->h_rows[r]) rc = llzs_d2d(*d_h + r * row, fd->d_new + r * row, sizeof(float) * row * (e - r), stream);
            r = e;
        }
    }
    memset(fd->h_rows, 0, rows);
    fd->blocks = fd->done = 0;
    return rc;
}

void llz_fade_release(llz_fade_t *fd)
{
    llzs_free(fd->d_new); llzs_free(fd->d_rows); free(fd->h_rows);
    memset(fd, 0, sizeof(*fd));
}
