/* llz_fir_stream_host.c -- include/llz_fir.h part 5: llz_fir_stream_mc, the block convolver that keeps the spectra of its input
 * between calls (kernel K4f, fir_stream.hip).  Its own handle and tag: the history of a firm_t (a ping-pong of flt_len - 1
 * samples and the tail kernel) does not apply here -- the history lives as a ring of input spectra plus the last input block.
 * Staging, pointer classification and error conventions are those of llz_fir_host.c.
 *
 * llz_fir_xfade_stream_mc fades rows to new taps over fade_blocks blocks.  The fade's state and rules are llz_fade.c's (the second
 * spectra buffer, the table of fading rows, the refusals, the adoption); what is the handle's own is here: while a fade is pending
 * or in flight every launch goes to fir_stream_fade.hip with the fade's position by value, and after the launch of a call or a
 * flush the handle moves the fade on by the blocks launched and adopts at its end, so that the next call runs the untouched
 * kernel. */
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"

#define FIRS_MIN_BLOCK 64
#define FIRS_MAX_BLOCK 4096

typedef struct {
    int tag;                    /* LLZ_TAG_FIRS */
    int device;                 /* the device the handle's buffers live on: every call binds it */
    int channels, block, frame_len, flt_len, rows;
    int k, P, R;                /* blocks per call, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes: kept here, passed by value with each launch */
    float *d_h;                 /* [rows][P][block] complex: the partition spectra (llz_host_stream_spectra) */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [channels][R][block] complex: spectra of the last R input blocks */
    float *d_prev;              /* [channels][block]: the last input block */
    llz_fade_t fade;            /* over the rows of d_h (llz_fade.c); allocated at the first fade and kept */
    void *stream;
    llz_stage_t st_in, st_out;  /* only for callers passing host memory */
} firs_t;

static void firs_destroy(firs_t *f)
{
    if (!f) return;
    llzs_free(f->d_h); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev);
    llz_fade_release(&f->fade);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->tag = 0;
    free(f);
}

/* the refusals of both inits, each with a message of its own that names `who` and the range */
static int firs_refuse(const char *who, int channels, int block, int frame_len, const void *taps, int rows, int flt_len)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (block < FIRS_MIN_BLOCK || block > FIRS_MAX_BLOCK || (block & (block - 1))) {
        llzs_set_error("%s: block %d is not a power of two in %d..%d", who, block, FIRS_MIN_BLOCK, FIRS_MAX_BLOCK);
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
    if (rows != 1 && rows != channels) {
        llzs_set_error("%s: rows %d is neither 1 (one tap set for all channels) nor channels (%d)", who, rows, channels);
        return 1;
    }
    if (!taps) {
        llzs_set_error("%s: no taps", who);
        return 1;
    }
    return 0;
}

/* zeros in the delay line (ring and last block), ordered on the handle's stream */
static int firs_clear(firs_t *f)
{
    int rc = llzs_memset(f->d_ring, 0, sizeof(float) * 2 * (size_t)f->channels * (size_t)f->R * (size_t)f->block, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev, 0, sizeof(float) * (size_t)f->channels * (size_t)f->block, f->stream);
    f->head = 0;
    return rc;
}

/* floats of one row's spectra */
static size_t firs_row(const firs_t *f) { return 2 * (size_t)f->P * (size_t)f->block; }

/* the fade is over (its last block launched, a reset, a flush): the new rows become the handle's */
static int firs_adopt(firs_t *f) { return llz_fade_adopt(&f->fade, &f->d_h, (size_t)f->rows, firs_row(f), f->stream); }

/* one launch of nblk blocks: the fade kernel exactly while a fade is pending or in flight.  The caller moves the fade on */
static int firs_launch(firs_t *f, const float *d_in, float *d_out, int nblk, int flush, long n_out, long in_pitch, long out_pitch)
{
    if (!f->fade.blocks)
        return llzs_fir_stream_f32(f->block, f->d_h, f->rows > 1, f->d_tw, f->d_ring, f->d_prev, d_in, d_out, f->channels, nblk,
                                   flush, n_out, in_pitch, out_pitch, f->P, f->R, f->head, f->stream);
    return llzs_fir_stream_fade_f32(f->block, f->d_h, f->rows > 1, f->d_tw, f->d_ring, f->d_prev, d_in, d_out, f->channels, nblk,
                                    flush, n_out, in_pitch, out_pitch, f->P, f->R, f->head, f->fade.d_new, f->fade.d_rows,
                                    f->fade.done, f->fade.blocks, f->stream);
}

unsigned long llz_fir_stream_mc_init(int channels, int block, int frame_len, const float *taps, int rows, int flt_len)
{
    const char *who = "llz_fir_stream_mc_init";
    if (firs_refuse(who, channels, block, frame_len, taps, rows, flt_len)) return LLZ_BAD_HANDLE;
    firs_t *f = (firs_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIRS;
    f->device = llzs_device_get();
    f->channels = channels; f->block = block; f->frame_len = frame_len; f->flt_len = flt_len; f->rows = rows;
    f->k = frame_len / block;
    f->P = (flt_len + block - 1) / block;
    f->R = f->P + f->k - 1;
    const size_t hbytes = sizeof(float) * 2 * (size_t)rows * (size_t)f->P * (size_t)block;
    const size_t rbytes = sizeof(float) * 2 * (size_t)channels * (size_t)f->R * (size_t)block;
    int rc = LLZ_OK;
    f->d_h = (float *)llzs_malloc(hbytes);
    if (!f->d_h) {
        llzs_set_error("%s: no device memory for the partition spectra: %zu B asked for (%d rows x %d partitions x %d bins)", who,
                       hbytes, rows, f->P, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_ring = (float *)llzs_malloc(rbytes))) {
        llzs_set_error("%s: no device memory for the delay line: %zu B asked for (%d channels x %d slots x %d bins)", who, rbytes,
                       channels, f->R, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) {
        f->d_tw = (float *)llzs_malloc(sizeof(float) * 2 * ((size_t)block / 2 + (size_t)block));
        f->d_prev = (float *)llzs_malloc(sizeof(float) * (size_t)channels * (size_t)block);
        if (!f->d_tw || !f->d_prev) {
            llzs_set_error("%s: no device memory for the twiddles and the last input blocks: %zu B and %zu B asked for", who,
                           sizeof(float) * 2 * ((size_t)block / 2 + (size_t)block), sizeof(float) * (size_t)channels * (size_t)block);
            rc = LLZ_ERR_NOMEM;
        }
    }
    /* tables through llzs_h2d_table, in a fixed order */
    if (rc == LLZ_OK)
        rc = llz_host_load_spectra(who, f->d_h, 2 * (size_t)f->P * (size_t)block, rows, taps, flt_len, 2 * block, 1, 1, NULL);
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, f->block);
    if (rc == LLZ_OK) rc = firs_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        firs_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_stream_mc_init_f64taps(int channels, int block, int frame_len, const double *taps, int rows, int flt_len)
{
    const char *who = "llz_fir_stream_mc_init_f64taps";
    if (firs_refuse(who, channels, block, frame_len, taps, rows, flt_len)) return LLZ_BAD_HANDLE;
    float *t = llz_host_taps_f32(who, taps, (size_t)rows * (size_t)flt_len);
    if (!t) return LLZ_BAD_HANDLE;
    unsigned long h = llz_fir_stream_mc_init(channels, block, frame_len, t, rows, flt_len);
    free(t);
    return h;
}

void llz_fir_stream_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS)) {
        firs_t *f = (firs_t *)handle;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        firs_destroy(f);
        llzs_device_leave(prev);
    }
}

static int firs_process(firs_t *f, const float *in, float *out, int frame_len)
{
    if (frame_len != f->frame_len) {
        llzs_set_error("llz_fir_stream_mc: frame_len %d != init frame_len %d", frame_len, f->frame_len);
        return LLZ_ERR_ARG;
    }
    if (in == out) {
        llzs_set_error("llz_fir_stream_mc: in-place filtering is not supported");
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len;
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    if (in_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;            /* a buffer of another GPU: refused, message set */
    if (llz_refuse_device_overlap("llz_fir_stream_mc", "in", in, bytes, in_dev, "out", out, bytes, out_dev)) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = llz_stage_in(&f->st_in, in, bytes, in_dev, f->stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc == LLZ_OK) rc = firs_launch(f, d_in, d_out, f->k, 0, frame_len, frame_len, frame_len);
    if (rc == LLZ_OK && f->fade.blocks) {
        f->fade.done += f->k;
        if (f->fade.done >= f->fade.blocks) rc = firs_adopt(f);
    }
    if (rc == LLZ_OK) f->head = (f->head + f->k) % f->R;
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->stream);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_fir_stream_mc(unsigned long handle, const float *in, float *out, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS) || !in || !out) {
        llzs_set_error("llz_fir_stream_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firs_t *f = (firs_t *)handle;
    const int prev = llzs_device_enter(f->device);       /* the handle's device, whatever the caller has current */
    const int rc = firs_process(f, in, out, frame_len);
    llzs_device_leave(prev);
    return rc;
}

static int firs_flush(firs_t *f, float *out)
{
    const int keep = f->flt_len - 1;
    if (keep == 0) {                                              /* nothing to emit; the handle still starts over */
        int rc0 = f->fade.blocks ? firs_adopt(f) : LLZ_OK;
        if (rc0 == LLZ_OK) rc0 = firs_clear(f);
        return rc0 == LLZ_OK ? 0 : rc0;
    }
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)keep;
    const int out_dev = llzs_is_device_ptr(out);
    if (out_dev < 0) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc != LLZ_OK) return rc;
    /* ceil(keep / block) zero blocks behind the input so far (a fade pending or in flight goes on through them: flush block j is
     * fade block done + j), then the delay line to zeros: the handle starts over, on the new taps */
    rc = firs_launch(f, NULL, d_out, (keep + f->block - 1) / f->block, 1, keep, 0, keep);
    if (rc == LLZ_OK && f->fade.blocks) rc = firs_adopt(f);
    if (rc == LLZ_OK) rc = firs_clear(f);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->stream);
    return rc == LLZ_OK ? keep : rc;
}

int llz_fir_stream_mc_flush(unsigned long handle, float *out)
{
    /* one tap: nothing to emit, so out may be NULL (an empty buffer has no address worth naming) */
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS) || (!out && ((firs_t *)handle)->flt_len > 1)) {
        llzs_set_error("llz_fir_stream_mc_flush: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firs_t *f = (firs_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = firs_flush(f, out);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_stream_mc_reset(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS)) {
        llzs_set_error("llz_fir_stream_mc_reset: bad handle");
        return LLZ_ERR_ARG;
    }
    firs_t *f = (firs_t *)handle;
    const int prev = llzs_device_enter(f->device);
    int rc = f->fade.blocks ? firs_adopt(f) : LLZ_OK;             /* a fade pending or in flight: the new taps at once */
    if (rc == LLZ_OK) rc = firs_clear(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_stream_mc_set_taps(unsigned long handle, int first, int count, const float *taps)
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS) || !taps) {
        llzs_set_error("llz_fir_stream_mc_set_taps: bad handle or NULL taps");
        return LLZ_ERR_ARG;
    }
    firs_t *f = (firs_t *)handle;
    if (first < 0 || count < 1 || first >= f->rows || count > f->rows - first) {
        llzs_set_error("llz_fir_stream_mc_set_taps: tap rows [%d, %d + %d) outside the handle's [0, %d)%s", first, first, count,
                       f->rows, f->rows == 1 && f->channels > 1 ? " (one tap set for all channels: only first 0, count 1)" : "");
        return LLZ_ERR_ARG;
    }
    if (llz_fade_refuse_set_taps(&f->fade, "llz_fir_stream_mc_set_taps")) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const size_t row = firs_row(f);
    const int rc = llz_host_load_spectra("llz_fir_stream_mc_set_taps", f->d_h + (size_t)first * row, row, count, taps, f->flt_len,
                                         2 * f->block, 1, 0, f->stream);      /* behind the calls already issued */
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_xfade_stream_mc(unsigned long handle, int first, int count, const float *taps, int fade_blocks)
{
    const char *who = "llz_fir_xfade_stream_mc";
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS)) {
        llzs_set_error("%s: bad handle", who);
        return LLZ_ERR_ARG;
    }
    firs_t *f = (firs_t *)handle;
    if (!taps) {
        llzs_set_error("%s: no taps", who);
        return LLZ_ERR_ARG;
    }
    if (first < 0 || count < 1 || first >= f->rows || count > f->rows - first) {
        llzs_set_error("%s: tap rows [%d, %d + %d) outside the handle's [0, %d)%s", who, first, first, count, f->rows,
                       f->rows == 1 && f->channels > 1 ? " (one tap set for all channels: only first 0, count 1)" : "");
        return LLZ_ERR_ARG;
    }
    if (llz_fade_refuse(&f->fade, who, "rows", fade_blocks)) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const size_t row = firs_row(f);
    int rc = llz_fade_reserve(&f->fade, who, "rows", (size_t)f->rows, row);
    if (rc == LLZ_OK)
        rc = llz_host_load_spectra(who, f->fade.d_new + (size_t)first * row, row, count, taps, f->flt_len, 2 * f->block, 1, 0,
                                   f->stream);
    if (rc == LLZ_OK) {
        unsigned char *t = (unsigned char *)malloc((size_t)f->rows);
        if (!t) {
            llzs_set_error("%s: out of host memory (%d B)", who, f->rows);
            rc = LLZ_ERR_NOMEM;
        } else {
            memcpy(t, f->fade.h_rows, (size_t)f->rows);
            memset(t + first, 1, (size_t)count);
            rc = llz_fade_commit(&f->fade, t, (size_t)f->rows, fade_blocks, f->stream);
            free(t);
        }
    }
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_xfade_stream_mc_left(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS)) return LLZ_ERR_ARG;
    return llz_fade_left(&((const firs_t *)handle)->fade);
}

int llz_fir_stream_mc_plan(unsigned long handle, int out[4])
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS) || !out) {
        llzs_set_error("llz_fir_stream_mc_plan: bad handle or no out");
        return LLZ_ERR_ARG;
    }
    const firs_t *f = (const firs_t *)handle;
    out[0] = 2 * f->block; out[1] = f->P; out[2] = f->R; out[3] = f->k;
    return LLZ_OK;
}

int llz_fir_stream_mc_flt_len(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS) ? ((firs_t *)handle)->flt_len : LLZ_ERR_ARG;
}

int llz_fir_stream_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, firs_t, LLZ_TAG_FIRS)) return LLZ_ERR_ARG;
    ((firs_t *)handle)->stream = stream;
    return LLZ_OK;
}
