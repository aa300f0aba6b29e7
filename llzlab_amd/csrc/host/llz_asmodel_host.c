/*
 * llz_asmodel_host.c -- handle layer of the windowed-FFT analysis / synthesis frames: the
 * reference's symbols (reference libllzfilter/llz_asmodel.c:109-310) and the float32 batch extension.
 */
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_asmodel.h"
#include "../../../include/llz_mdct.h"
#include "llz_host.h"

#define LLZ_TAG_ASM1 0x4c5a5331
#define LLZ_TAG_ASMM 0x4c5a534d

static int asm_shape(int overlap_hint, int frame_len, int *fft_len, double *magic)
{
    /* llz_asmodel.c:114-123 */
    if (frame_len > LLZS_FFT_MAX) return 0;                        /* (the shift below would overflow) */
    if (overlap_hint == LLZ_OVERLAP_HIGH) { *fft_len = frame_len << 2; *magic = 0.812; }
    else if (overlap_hint == LLZ_OVERLAP_LOW) { *fft_len = frame_len << 1; *magic = 1; }
    else return 0;
    return frame_len >= 1 && *fft_len >= 2 && (*fft_len & (*fft_len - 1)) == 0;
}

/* ---- Part 1: the reference's symbols, one channel, one frame per call ----
 * A handle keeps its running frame buffer, the window and the scratch spectrum in DEVICE memory.  A call copies the new
 * samples (or the two spectrum planes) in, runs framing kernel -> exact-order transform -> framing kernel on the device
 * (kernels/frames_f64.hip; the transform of llz_fft: kernels/fft.hip up to 4096 points, kernels/fft_large.hip above, up
 * to LLZS_FFT_MAX), and copies the result out; nothing is computed on the host. */

typedef struct {
    llz_head_t head;
    int hop, size, bins;                    /* hop = frame_len, size = fft_len, bins = size/2 + 1 */
    double out_scale;                       /* the reference's empirical 0.812 at 3/4 overlap, 1 at 1/2 */
    double *d_window, *d_fft_cs;
    double *d_run[2];                       /* analysis: the last `size` input samples; synthesis: the overlap-add sums */
    int cur;
    double *d_spectrum;                     /* size interleaved complex points */
    double *d_io;                           /* hop samples, or the two planes of bins values */
} asm1_t;

static void asm1_destroy(void *p)
{
    asm1_t *f = (asm1_t *)p;
    llzs_free(f->d_window); llzs_free(f->d_fft_cs); llzs_free(f->d_run[0]); llzs_free(f->d_run[1]);
    llzs_free(f->d_spectrum); llzs_free(f->d_io);
    f->head.tag = 0;
    free(f);
}

static unsigned long asm1_init(int overlap_hint, int frame_len, win_t win_type, const char *who)
{
    int fft_len;
    double magic;
    if (!asm_shape(overlap_hint, frame_len, &fft_len, &magic) || fft_len > LLZS_FFT_MAX) {
        llzs_set_error("%s: overlap_hint %d frame_len %d (fft_len must be a power of two in 2..%d)", who, overlap_hint,
                       frame_len, LLZS_FFT_MAX);
        return LLZ_BAD_HANDLE;
    }
    double *w = (double *)malloc(sizeof(double) * (size_t)fft_len);
    if (w && !llz_host_window(w, fft_len, win_type)) {
        llzs_set_error("%s: unknown window %d", who, (int)win_type);
        free(w);
        return LLZ_BAD_HANDLE;
    }
    asm1_t *f = w ? (asm1_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ASM1, 1) : NULL;
    if (f) {
        const size_t N = (size_t)fft_len, db = sizeof(double);
        f->hop = frame_len; f->size = fft_len; f->bins = (fft_len >> 1) + 1; f->out_scale = magic;
        f->d_window = (double *)llz_host_upload(w, db * N);
        f->d_fft_cs = llz_host_cs_f64(fft_len);
        f->d_run[0] = (double *)llz_host_zeros(db * N);
        f->d_run[1] = (double *)llz_host_zeros(db * N);
        f->d_spectrum = (double *)llz_host_zeros(db * 2 * N);
        f->d_io = (double *)llz_host_zeros(db * (2 * (size_t)f->bins > (size_t)frame_len ? 2 * (size_t)f->bins : (size_t)frame_len));
        if (f->head.device < 0 || !f->d_window || !f->d_fft_cs || !f->d_run[0] || !f->d_run[1] || !f->d_spectrum || !f->d_io ||
            llzs_sync(NULL) != LLZ_OK) {
            asm1_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

static void asm1_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_ASM1, asm1_destroy); }

unsigned long llz_analysis_fft_init(int overlap_hint, int frame_len, win_t win_type)
{
    return asm1_init(overlap_hint, frame_len, win_type, "llz_analysis_fft_init");
}

unsigned long llz_synthesis_fft_init(int overlap_hint, int frame_len, win_t win_type)
{
    return asm1_init(overlap_hint, frame_len, win_type, "llz_synthesis_fft_init");
}

void llz_analysis_fft_uninit(unsigned long handle) { asm1_uninit(handle); }
void llz_synthesis_fft_uninit(unsigned long handle) { asm1_uninit(handle); }

/* the exact-order transform of llz_fft / llz_ifft on the handle's spectrum, picked by size as fft1_run does */
static int asm1_fft(asm1_t *f, int inverse)
{
    return f->size <= 4096 ? llzs_fft_f64(f->d_spectrum, f->size, f->d_fft_cs, inverse, NULL)
                           : llzs_fft_large_f64(f->d_spectrum, f->size, f->d_fft_cs, inverse, NULL);
}

/* reference llz_asmodel.c:177-203: slide the input buffer by one frame, window, forward transform, bins 0..N/2 */
void llz_analysis_fft(unsigned long handle, double *x, double *re, double *im)
{
    asm1_t *f = (asm1_t *)llz_handle(handle, LLZ_TAG_ASM1, NULL);
    if (!f || !x || !re || !im) {
        llzs_set_error("llz_analysis_fft: bad handle or arguments");
        return;                                                     /* void in the reference ABI */
    }
    const size_t plane = sizeof(double) * (size_t)f->bins;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_io, x, sizeof(double) * (size_t)f->hop, NULL);
    if (rc == LLZ_OK)
        rc = llzs_frame_slide_window_f64(f->d_io, f->d_run[f->cur], f->d_run[f->cur ^ 1], f->d_window, f->d_spectrum,
                                         f->size, f->hop, 1, NULL);
    if (rc == LLZ_OK) f->cur ^= 1;
    if (rc == LLZ_OK) rc = asm1_fft(f, 0);
    if (rc == LLZ_OK) rc = llzs_spectrum_split_f64(f->d_spectrum, f->d_io, f->bins, NULL);
    if (rc == LLZ_OK) rc = llzs_d2h(re, f->d_io, plane, NULL);
    if (rc == LLZ_OK) rc = llzs_d2h(im, f->d_io + f->bins, plane, NULL);
    llzs_device_leave(prev);
}

/* reference llz_asmodel.c:274-309: conjugate-mirror the half spectrum, inverse transform, window, overlap-add, emit */
void llz_synthesis_fft(unsigned long handle, double *re, double *im, double *x)
{
    asm1_t *f = (asm1_t *)llz_handle(handle, LLZ_TAG_ASM1, NULL);
    if (!f || !x || !re || !im) {
        llzs_set_error("llz_synthesis_fft: bad handle or arguments");
        return;
    }
    const size_t plane = sizeof(double) * (size_t)f->bins;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_io, re, plane, NULL);
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_io + f->bins, im, plane, NULL);
    if (rc == LLZ_OK) rc = llzs_spectrum_mirror_f64(f->d_io, f->d_spectrum, f->size, NULL);
    if (rc == LLZ_OK) rc = asm1_fft(f, 1);
    if (rc == LLZ_OK)
        rc = llzs_frame_overlap_add_f64(f->d_spectrum, 2, f->d_window, f->d_run[f->cur], f->d_run[f->cur ^ 1], f->d_io,
                                        f->size, f->hop, f->out_scale, NULL);
    if (rc == LLZ_OK) f->cur ^= 1;
    if (rc == LLZ_OK) rc = llzs_d2h(x, f->d_io, sizeof(double) * (size_t)f->hop, NULL);
    llzs_device_leave(prev);
}

/* ---- Part 1b: MDCT frames with 50 % overlap (llz_asmodel.c:313-463), same scheme around the device MDCT ---- */

#define LLZ_TAG_ASMD 0x4c5a5344

typedef struct {
    llz_head_t head;
    int hop, size;                          /* hop = frame_len, size = mdct_len = 2 hop */
    double *d_window;
    double *d_run[2];                       /* analysis: the last two frames; synthesis: the overlap-add sums */
    int cur;
    double *d_frame, *d_coef, *d_io;        /* size windowed samples, hop coefficients, hop samples in / out */
    unsigned long mdct;                     /* llz_mdct_init(MDCT_FFT4, size): the N/4-point form, llz_asmodel.c:323 */
} asmd_t;

static void asmd_destroy(void *p)
{
    asmd_t *f = (asmd_t *)p;
    if (f->mdct && f->mdct != LLZ_BAD_HANDLE) llz_mdct_uninit(f->mdct);
    llzs_free(f->d_window); llzs_free(f->d_run[0]); llzs_free(f->d_run[1]);
    llzs_free(f->d_frame); llzs_free(f->d_coef); llzs_free(f->d_io);
    f->head.tag = 0;
    free(f);
}

/* the MDCT window of llz_asmodel.c:327-334 over N points */
static void asmd_window(double *w, int N, mdct_win_t win_type)
{
    if (win_type == MDCT_SINE) llz_mdct_sine(w, N);
    else llz_mdct_kbd(w, N, 6);
}

static unsigned long asmd_init(int frame_len, mdct_win_t win_type, const char *who)
{
    if (frame_len < 4 || frame_len > 8192 || (frame_len & (frame_len - 1)) ||
        (win_type != MDCT_SINE && win_type != MDCT_KBD)) {
        llzs_set_error("%s: frame_len %d (a power of two in 4..8192) window %d", who, frame_len, (int)win_type);
        return LLZ_BAD_HANDLE;
    }
    const int N = frame_len << 1;
    const size_t db = sizeof(double);
    double *w = (double *)malloc(db * (size_t)N);
    asmd_t *f = w ? (asmd_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ASMD, 1) : NULL;
    if (f) {
        f->hop = frame_len; f->size = N;
        asmd_window(w, N, win_type);
        f->d_window = (double *)llz_host_upload(w, db * (size_t)N);
        f->d_run[0] = (double *)llz_host_zeros(db * (size_t)N);
        f->d_run[1] = (double *)llz_host_zeros(db * (size_t)N);
        f->d_frame = (double *)llz_host_zeros(db * (size_t)N);
        f->d_coef = (double *)llz_host_zeros(db * (size_t)frame_len);
        f->d_io = (double *)llz_host_zeros(db * (size_t)frame_len);
        f->mdct = llz_mdct_init(MDCT_FFT4, N);
        if (f->head.device < 0 || !f->d_window || !f->d_run[0] || !f->d_run[1] || !f->d_frame || !f->d_coef || !f->d_io ||
            f->mdct == LLZ_BAD_HANDLE || llzs_sync(NULL) != LLZ_OK) {
            asmd_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

static void asmd_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_ASMD, asmd_destroy); }

unsigned long llz_analysis_mdct_init(int frame_len, mdct_win_t win_type)
{
    return asmd_init(frame_len, win_type, "llz_analysis_mdct_init");
}

unsigned long llz_synthesis_mdct_init(int frame_len, mdct_win_t win_type)
{
    return asmd_init(frame_len, win_type, "llz_synthesis_mdct_init");
}

void llz_analysis_mdct_uninit(unsigned long handle) { asmd_uninit(handle); }
void llz_synthesis_mdct_uninit(unsigned long handle) { asmd_uninit(handle); }

/* reference llz_asmodel.c:365-383 */
void llz_analysis_mdct(unsigned long handle, double *x, double *X)
{
    asmd_t *f = (asmd_t *)llz_handle(handle, LLZ_TAG_ASMD, NULL);
    if (!f || !x || !X) {
        llzs_set_error("llz_analysis_mdct: bad handle or arguments");
        return;
    }
    const size_t frame = sizeof(double) * (size_t)f->hop;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_io, x, frame, NULL);
    if (rc == LLZ_OK)
        rc = llzs_frame_slide_window_f64(f->d_io, f->d_run[f->cur], f->d_run[f->cur ^ 1], f->d_window, f->d_frame,
                                         f->size, f->hop, 0, NULL);
    if (rc == LLZ_OK) f->cur ^= 1;
    if (rc == LLZ_OK) rc = llz_host_mdct_on_device(f->mdct, f->d_frame, f->d_coef, 0);
    if (rc == LLZ_OK) rc = llzs_d2h(X, f->d_coef, frame, NULL);
    llzs_device_leave(prev);
}

/* reference llz_asmodel.c:440-462 */
void llz_synthesis_mdct(unsigned long handle, double *X, double *x)
{
    asmd_t *f = (asmd_t *)llz_handle(handle, LLZ_TAG_ASMD, NULL);
    if (!f || !x || !X) {
        llzs_set_error("llz_synthesis_mdct: bad handle or arguments");
        return;
    }
    const size_t frame = sizeof(double) * (size_t)f->hop;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_coef, X, frame, NULL);
    if (rc == LLZ_OK) rc = llz_host_mdct_on_device(f->mdct, f->d_coef, f->d_frame, 1);
    if (rc == LLZ_OK)
        rc = llzs_frame_overlap_add_f64(f->d_frame, 1, f->d_window, f->d_run[f->cur], f->d_run[f->cur ^ 1], f->d_io,
                                        f->size, f->hop, 1.0, NULL);
    if (rc == LLZ_OK) f->cur ^= 1;
    if (rc == LLZ_OK) rc = llzs_d2h(x, f->d_io, frame, NULL);
    llzs_device_leave(prev);
}

/* ---- Part 2: batch extension ----
 * fft_len up to 4096: one launch per direction (kernels/stft.hip).  Above 4096, and at 4096 under the fft_generic tune: the
 * composed form -- framing kernel, the float32 batch transform of llz_fft_batch on a scratch buffer, framing kernel
 * (kernels/stft_large.hip) -- over chunks of at most LLZS_STFT_CHUNK_POINTS points, so the scratch stays bounded whatever
 * a call's frame count.  (A one-launch form of 8192 on the staged LDS kernels measured slower than the composed form:
 * DESIGN.md section 3, rank 3.) */

typedef struct {
    llz_head_t head;
    int channels, frame_len, fft_len, bins;
    float magic;
    float *d_w, *d_cs;
    float *d_twb;                       /* fft_len above 4096: the large transform's LDS-block table (llz_fft_batch_init's) */
    float *d_hist[2], *d_ola[2];        /* analysis history / synthesis overlap-add tail: [channels][fft_len-frame_len] */
    int cur_hist, cur_ola;
    llz_stage_t st_x, st_re, st_im;
    llz_stage_t st_z;                   /* the composed form's scratch: one chunk of frames, then the synthesis tails */
} asmm_t;

static void asmm_destroy(void *p)
{
    asmm_t *f = (asmm_t *)p;
    llzs_free(f->d_w); llzs_free(f->d_cs); llzs_free(f->d_twb);
    llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]); llzs_free(f->d_ola[0]); llzs_free(f->d_ola[1]);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_re); llz_stage_release(&f->st_im); llz_stage_release(&f->st_z);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_stft_mc_init(int channels, int overlap_hint, int frame_len, win_t win_type)
{
    int N;
    double magic;
    if (channels < 1 || !asm_shape(overlap_hint, frame_len, &N, &magic) || N < 8 || N > LLZS_FFT_MAX) {
        llzs_set_error("llz_stft_mc_init: channels %d overlap_hint %d frame_len %d (fft_len a power of two in 8..%d)",
                       channels, overlap_hint, frame_len, LLZS_FFT_MAX);
        return LLZ_BAD_HANDLE;
    }
    double *w = (double *)malloc(sizeof(double) * (size_t)N);
    if (w && !llz_host_window(w, N, win_type)) {
        llzs_set_error("llz_stft_mc_init: unknown window %d", (int)win_type);
        free(w);
        return LLZ_BAD_HANDLE;
    }
    asmm_t *f = w ? (asmm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_ASMM, 1) : NULL;
    if (f) {
        const size_t keep = sizeof(float) * (size_t)channels * (size_t)(N - frame_len);
        f->channels = channels; f->frame_len = frame_len; f->fft_len = N; f->bins = N / 2 + 1;
        f->magic = (float)magic;
        f->d_w = llz_host_upload_f32(w, (size_t)N);
        f->d_cs = llz_host_cs_f32(N);                                /* table of llz_fft_init, llz_fft.c:222-229 */
        int rc = f->d_w && f->d_cs ? LLZ_OK : LLZ_ERR_NOMEM;
        for (int k = 0; k < 2 && rc == LLZ_OK; k++) {
            f->d_hist[k] = (float *)llz_host_zeros(keep);
            f->d_ola[k] = (float *)llz_host_zeros(keep);
            if (!f->d_hist[k] || !f->d_ola[k]) rc = LLZ_ERR_NOMEM;
        }
        if (rc == LLZ_OK && N > 4096) {                              /* as llz_fft_batch_init builds it */
            f->d_twb = (float *)llzs_malloc((size_t)llzs_fft_large_twb_bytes(N));
            rc = f->d_twb ? llzs_fft_large_twb(f->d_twb, N, f->d_cs, NULL) : LLZ_ERR_NOMEM;
        }
        if (rc == LLZ_ERR_NOMEM)
            llzs_set_error("llz_stft_mc_init: device allocation failed (channels %d fft_len %d: 4 x %zu bytes of state)",
                           channels, N, keep);
        if (rc == LLZ_OK) rc = llzs_sync(NULL);
        if (rc != LLZ_OK) {
            asmm_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

void llz_stft_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_ASMM, asmm_destroy); }

int llz_stft_mc_bins(unsigned long handle)
{
    asmm_t *f = (asmm_t *)llz_handle(handle, LLZ_TAG_ASMM, NULL);
    return f ? f->bins : LLZ_ERR_ARG;
}

int llz_stft_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_ASMM, "llz_stft_mc_set_stream", stream);
}

/* device views of the three caller buffers: x [C][frames*F], re/im [C][frames][bins]; x_is_input marks which side is input */
static int asmm_stage(asmm_t *f, const float *x, const float *re, const float *im, int frames, int x_is_input,
                      float **dx, float **dre, float **dim)
{
    const size_t xb = sizeof(float) * (size_t)f->channels * frames * f->frame_len;
    const size_t sb = sizeof(float) * (size_t)f->channels * frames * f->bins;
    const int x_dev = llzs_is_device_ptr(x), re_dev = llzs_is_device_ptr(re), im_dev = llzs_is_device_ptr(im);
    if (x_dev < 0 || re_dev < 0 || im_dev < 0) return LLZ_ERR_ARG;
    const char *who = x_is_input ? "llz_stft_mc_analysis" : "llz_stft_mc_synthesis";
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
    return rc;
}

/* the composed form: fft_len above 4096, or 4096 under the fft_generic tune (the A/B of the one-launch kernels) */
static int asmm_composed(const asmm_t *f)
{
    return f->fft_len > 4096 || (f->fft_len == 4096 && llzs_tune(LLZS_TUNE_FFT_GENERIC) == 1);
}

/* transforms per chunk, and the scratch of a chunk: count * N complex points, then (synthesis) the tails of the chunk's
 * channels (at most count + 1 of them) */
static int asmm_chunk(const asmm_t *f)
{
    const int count = LLZS_STFT_CHUNK_POINTS / f->fft_len;
    return count > 0 ? count : 1;
}

static float *asmm_scratch(asmm_t *f, int count, int with_tails)
{
    const long tails = with_tails ? (count + 1 < f->channels ? count + 1 : f->channels) : 0;
    const size_t bytes = sizeof(float) * ((size_t)2 * count * f->fft_len + (size_t)tails * (f->fft_len - f->frame_len));
    float *z = (float *)llz_stage_reserve(&f->st_z, bytes);
    if (!z) llzs_set_error("llz_stft_mc: no device memory for the %zu-byte transform scratch", bytes);
    return z;
}

/* the float32 batch transform of llz_fft_batch (fftb_launch in llz_fft_host.c) */
static int asmm_fft(const asmm_t *f, float *z, int count, int inverse)
{
    return f->fft_len <= 4096 ? llzs_fft_f32(z, count, f->fft_len, f->d_cs, inverse, f->head.stream)
                              : llzs_fft_large_f32(z, count, f->fft_len, f->d_cs, f->d_twb, inverse, f->head.stream);
}

static int asmm_analysis_composed(asmm_t *f, const float *dx, float *dre, float *dim, int frames, long x_pitch)
{
    const long total = (long)f->channels * frames;
    const int chunk = asmm_chunk(f);
    float *z = asmm_scratch(f, (int)(total < chunk ? total : chunk), 0);
    int rc = z ? LLZ_OK : LLZ_ERR_NOMEM;
    for (long g0 = 0; g0 < total && rc == LLZ_OK; g0 += chunk) {
        const int count = (int)(total - g0 < chunk ? total - g0 : chunk);
        rc = llzs_stft_frames_large_f32(dx, f->d_hist[f->cur_hist], z, f->d_w, frames, f->frame_len, f->fft_len, x_pitch,
                                        g0, count, f->head.stream);
        if (rc == LLZ_OK) rc = asmm_fft(f, z, count, 0);
        if (rc == LLZ_OK) rc = llzs_stft_bins_large_f32(z, dre, dim, f->fft_len, g0, count, f->head.stream);
    }
    return rc;
}

static int asmm_synthesis_composed(asmm_t *f, const float *dre, const float *dim, float *dx, int frames, long x_pitch)
{
    const long total = (long)f->channels * frames;
    const int chunk = asmm_chunk(f);
    const int most = (int)(total < chunk ? total : chunk);
    float *z = asmm_scratch(f, most, 1);
    int rc = z ? LLZ_OK : LLZ_ERR_NOMEM;
    float *tails = z + (size_t)2 * most * f->fft_len;
    for (long g0 = 0; g0 < total && rc == LLZ_OK; g0 += chunk) {
        const int count = (int)(total - g0 < chunk ? total - g0 : chunk);
        rc = llzs_stft_mirror_large_f32(dre, dim, z, f->fft_len, g0, count, f->head.stream);
        if (rc == LLZ_OK) rc = asmm_fft(f, z, count, 1);
        if (rc == LLZ_OK)
            rc = llzs_stft_ola_large_f32(z, dx, f->d_ola[f->cur_ola], f->d_ola[f->cur_ola ^ 1], tails, f->d_w, frames,
                                         f->frame_len, f->fft_len, x_pitch, g0, count, f->magic, f->head.stream);
    }
    return rc;
}

int llz_stft_mc_analysis(unsigned long handle, const float *x, float *re, float *im, int frames)
{
    asmm_t *f = (asmm_t *)llz_handle(handle, LLZ_TAG_ASMM, NULL);
    if (!f || !x || !re || !im || frames < 1) {
        llzs_set_error("llz_stft_mc_analysis: bad handle or arguments");
        return LLZ_ERR_ARG;
    }
    const long n = (long)frames * f->frame_len;
    float *dx, *dre, *dim;
    const int prev = llzs_device_enter(f->head.device);
    int rc = asmm_stage(f, x, re, im, frames, 1, &dx, &dre, &dim);
    if (rc == LLZ_OK && asmm_composed(f))
        rc = asmm_analysis_composed(f, dx, dre, dim, frames, n);
    else if (rc == LLZ_OK)
        rc = llzs_stft_analysis_f32(dx, f->d_hist[f->cur_hist], dre, dim, f->d_w, f->d_cs, f->channels, frames,
                                    f->frame_len, f->fft_len, n, f->head.stream);
    /* history for the next call: the last fft_len - frame_len samples of concat(history, x) */
    if (rc == LLZ_OK)
        rc = llzs_fir_tail_f32(dx, f->d_hist[f->cur_hist], f->d_hist[f->cur_hist ^ 1], f->channels, n, n,
                               f->fft_len - f->frame_len + 1, f->head.stream);
    if (rc == LLZ_OK) f->cur_hist ^= 1;
    const size_t sb = sizeof(float) * (size_t)f->channels * frames * f->bins;
    if (rc == LLZ_OK && dre != re) rc = llzs_d2h(re, dre, sb, f->head.stream);
    if (rc == LLZ_OK && dim != im) rc = llzs_d2h(im, dim, sb, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

int llz_stft_mc_synthesis(unsigned long handle, const float *re, const float *im, float *x, int frames)
{
    asmm_t *f = (asmm_t *)llz_handle(handle, LLZ_TAG_ASMM, NULL);
    if (!f || !x || !re || !im || frames < 1) {
        llzs_set_error("llz_stft_mc_synthesis: bad handle or arguments");
        return LLZ_ERR_ARG;
    }
    const long n = (long)frames * f->frame_len;
    float *dx, *dre, *dim;
    const int prev = llzs_device_enter(f->head.device);
    int rc = asmm_stage(f, x, re, im, frames, 0, &dx, &dre, &dim);
    if (rc == LLZ_OK && asmm_composed(f))
        rc = asmm_synthesis_composed(f, dre, dim, dx, frames, n);
    else if (rc == LLZ_OK)
        rc = llzs_stft_synthesis_f32(dre, dim, dx, f->d_ola[f->cur_ola], f->d_ola[f->cur_ola ^ 1], f->d_w, f->d_cs,
                                     f->channels, frames, f->frame_len, f->fft_len, n, f->magic, f->head.stream);
    if (rc == LLZ_OK) f->cur_ola ^= 1;
    if (rc == LLZ_OK && dx != x) rc = llzs_d2h(x, dx, sizeof(float) * (size_t)f->channels * n, f->head.stream);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

/* ---- Part 2b: windowed MDCT frames (time-domain alias cancellation) in batch, float32 ---- */
/* The batch form of llz_analysis_mdct / llz_synthesis_mdct (llz_asmodel.c:313-463): per channel, analysis keeps the previous
 * frame and synthesis the overlap-add tail, so consecutive calls continue the streams.  On the register MDCT kernels
 * (k_mdct_reg_f32<..., FRAMES>): the window is applied as the transform reads / writes, frames are taken straight from the
 * planar signal at a hop of frame_len (nothing is expanded in memory). */
#define LLZ_TAG_AMDM 0x4c5a4d4d

typedef struct {
    llz_head_t head;
    int channels, frame_len, mdct_len;
    float *d_w, *d_tc, *d_ts, *d_cs;
    float *d_prev[2], *d_tail[2];       /* analysis: the previous frame; synthesis: the overlap-add tail; [channels][frame_len] */
    int cur_prev, cur_tail;
    llz_stage_t st_x, st_X;
} amdm_t;

static void amdm_destroy(void *p)
{
    amdm_t *f = (amdm_t *)p;
    llzs_free(f->d_w); llzs_free(f->d_tc); llzs_free(f->d_ts); llzs_free(f->d_cs);
    llzs_free(f->d_prev[0]); llzs_free(f->d_prev[1]); llzs_free(f->d_tail[0]); llzs_free(f->d_tail[1]);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_X);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_mdct_frames_mc_init(int channels, int frame_len, mdct_win_t win_type)
{
    if (channels < 1 || frame_len < 128 || frame_len > 4096 || (frame_len & (frame_len - 1)) ||
        (win_type != MDCT_SINE && win_type != MDCT_KBD)) {
        llzs_set_error("llz_mdct_frames_mc_init: channels %d frame_len %d (a power of two in 128..4096) window %d",
                       channels, frame_len, (int)win_type);
        return LLZ_BAD_HANDLE;
    }
    const int N = frame_len << 1;
    double *w = (double *)malloc(sizeof(double) * (size_t)N);
    amdm_t *f = w ? (amdm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_AMDM, 1) : NULL;
    if (f) {
        const size_t keep = sizeof(float) * (size_t)channels * (size_t)frame_len;
        f->channels = channels; f->frame_len = frame_len; f->mdct_len = N;
        asmd_window(w, N, win_type);
        f->d_w = llz_host_upload_f32(w, (size_t)N);
        int rc = f->d_w ? llz_host_mdct_pretwiddles_f32(N, &f->d_tc, &f->d_ts) : LLZ_ERR_NOMEM;
        if (rc == LLZ_OK && !(f->d_cs = llz_host_cs_f32(N >> 2))) rc = LLZ_ERR_NOMEM;  /* llz_fft.c:222-229 for size N/4 */
        for (int k = 0; k < 2 && rc == LLZ_OK; k++) {
            f->d_prev[k] = (float *)llz_host_zeros(keep);
            f->d_tail[k] = (float *)llz_host_zeros(keep);
            if (!f->d_prev[k] || !f->d_tail[k]) rc = LLZ_ERR_NOMEM;
        }
        if (rc == LLZ_OK) rc = llzs_sync(NULL);
        if (rc != LLZ_OK) {
            amdm_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

void llz_mdct_frames_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_AMDM, amdm_destroy); }

int llz_mdct_frames_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_AMDM, "llz_mdct_frames_mc_set_stream", stream);
}

static int amdm_run(unsigned long handle, const float *in, float *out, int frames, int inverse, const char *who)
{
    amdm_t *f = (amdm_t *)llz_handle(handle, LLZ_TAG_AMDM, NULL);
    if (!f || !in || !out || frames < 1 || in == out) {
        llzs_set_error("%s: bad handle or arguments", who);
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frames * (size_t)f->frame_len;   /* both sides */
    const int prev = llzs_device_enter(f->head.device);
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    int rc = (in_dev < 0 || out_dev < 0) ? LLZ_ERR_ARG : LLZ_OK;
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap(who, "in", in, bytes, in_dev, "out", out, bytes, out_dev);
    const float *d_in = (const float *)llz_vec_stage_in(inverse ? &f->st_X : &f->st_x, in, bytes, in_dev, f->head.stream, &rc);
    float *d_out = (float *)llz_vec_stage_out(inverse ? &f->st_x : &f->st_X, out, bytes, out_dev, &rc);
    float **st = inverse ? f->d_tail : f->d_prev;
    int *cur = inverse ? &f->cur_tail : &f->cur_prev;
    if (rc == LLZ_OK)
        rc = llzs_mdct4_frames_f32(d_in, d_out, f->channels, frames, f->mdct_len, f->d_tc, f->d_ts, f->d_cs, f->d_w, st[*cur],
                                   st[*cur ^ 1], inverse, f->head.stream);
    if (rc == LLZ_OK) *cur ^= 1;
    llz_vec_stage_back(out, d_out, bytes, out_dev, f->head.stream, &rc);
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

int llz_mdct_frames_mc_analysis(unsigned long handle, const float *x, float *X, int frames)
{
    return amdm_run(handle, x, X, frames, 0, "llz_mdct_frames_mc_analysis");
}

int llz_mdct_frames_mc_synthesis(unsigned long handle, const float *X, float *x, int frames)
{
    return amdm_run(handle, X, x, frames, 1, "llz_mdct_frames_mc_synthesis");
}
