/*
 * llz_spectral_host.c -- handle layer of the Welch cross-spectra (include/llz_spectral.h; kernels/csd.hip): the window and
 * twiddle tables, the pair table, the history ping-pong, the run grid with its carried float32 partial, the double
 * accumulators, and the walk of the partial scratch in slabs of runs.
 */
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_spectral.h"
#include "llz_host.h"

#define LLZ_TAG_CSDM 0x4c5a4353
#define CSD_SCRATCH_BYTES ((size_t)256 << 20)      /* run partials: at most this much, walked in slabs of runs */
#define CSD_READ_RAW 5

typedef struct {
    llz_head_t head;
    int channels, pairs, fft_len, hop, bins, keep;
    long hops;                      /* hops of every channel's stream taken since the last reset */
    double u;                       /* sum of the squared float32 window values */
    float *d_w, *d_cs;
    int *d_pairs;
    float *d_hist[2];               /* [channels][fft_len - hop], the samples in front of the next call */
    int cur;
    double *d_acc;                  /* [pairs][bins][4]: the finished runs */
    float *d_carry[2];              /* [2][pairs][bins][4] each: the open run's sums, then their compensation terms.  A call
                                     * reads [cur_carry] and writes the other one (an update may continue one run and leave a
                                     * later one open in ONE launch, whose work items are not ordered); [cur_carry] is valid
                                     * while frames % LLZ_CSD_RUN != 0 */
    int cur_carry;
    llz_stage_t st_x, st_out, st_scratch;
} csdm_t;

static long csd_frames_at(const csdm_t *f, long hops)
{
    const long lead = f->fft_len / f->hop - 1;      /* hops before the first whole frame */
    return hops > lead ? hops - lead : 0;
}

static size_t csd_cell_bytes(const csdm_t *f, size_t elem) { return elem * 4 * (size_t)f->pairs * (size_t)f->bins; }

static void csdm_destroy(void *p)
{
    csdm_t *f = (csdm_t *)p;
    llzs_free(f->d_w); llzs_free(f->d_cs); llzs_free(f->d_pairs);
    llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]); llzs_free(f->d_acc); llzs_free(f->d_carry[0]); llzs_free(f->d_carry[1]);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_out); llz_stage_release(&f->st_scratch);
    f->head.tag = 0;
    free(f);
}

static int csd_clear(csdm_t *f)
{
    int rc = llzs_memset(f->d_acc, 0, csd_cell_bytes(f, sizeof(double)), f->head.stream);
    for (int k = 0; k < 2 && rc == LLZ_OK; k++)
        rc = llzs_memset(f->d_carry[k], 0, 2 * csd_cell_bytes(f, sizeof(float)), f->head.stream);
    for (int k = 0; k < 2 && rc == LLZ_OK && f->keep; k++)
        rc = llzs_memset(f->d_hist[k], 0, sizeof(float) * (size_t)f->channels * (size_t)f->keep, f->head.stream);
    if (rc == LLZ_OK) f->hops = 0;
    return rc;
}

unsigned long llz_csd_mc_init(int channels, int pairs, const int *pair_xy, int fft_len, int hop, win_t win_type)
{
    const int N = fft_len;
    if (channels < 1 || pairs < 1 || !pair_xy) {
        llzs_set_error("llz_csd_mc_init: channels %d pairs %d pair_xy %p (channels >= 1, pairs >= 1, a host table)", channels,
                       pairs, (const void *)pair_xy);
        return LLZ_BAD_HANDLE;
    }
    if (N < 64 || N > 4096 || (N & (N - 1)) != 0) {
        llzs_set_error("llz_csd_mc_init: fft_len %d (a power of two in 64..4096)", N);
        return LLZ_BAD_HANDLE;
    }
    if (hop != N && hop != N / 2 && hop != N / 4) {
        llzs_set_error("llz_csd_mc_init: hop %d (fft_len %d: one of %d, %d, %d)", hop, N, N, N / 2, N / 4);
        return LLZ_BAD_HANDLE;
    }
    for (int p = 0; p < 2 * pairs; p++)
        if (pair_xy[p] < 0 || pair_xy[p] >= channels) {
            llzs_set_error("llz_csd_mc_init: pair %d names channel %d (channels %d: 0..%d)", p / 2, pair_xy[p], channels,
                           channels - 1);
            return LLZ_BAD_HANDLE;
        }
    double *w = (double *)malloc(sizeof(double) * (size_t)N);
    if (w && !llz_host_window(w, N, win_type)) {
        llzs_set_error("llz_csd_mc_init: unknown window %d", (int)win_type);
        free(w);
        return LLZ_BAD_HANDLE;
    }
    csdm_t *f = w ? (csdm_t *)llz_handle_new(sizeof(*f), LLZ_TAG_CSDM, 1) : NULL;
    if (f) {
        f->channels = channels; f->pairs = pairs;
        f->fft_len = N; f->hop = hop; f->bins = N / 2 + 1; f->keep = N - hop;
        for (int i = 0; i < N; i++) f->u += (double)(float)w[i] * (double)(float)w[i];
        const size_t hist = sizeof(float) * (size_t)channels * (size_t)f->keep;
        f->d_w = llz_host_upload_f32(w, (size_t)N);
        f->d_cs = llz_host_cs_f32(N);
        f->d_pairs = (int *)llz_host_upload(pair_xy, sizeof(int) * 2 * (size_t)pairs);
        f->d_acc = (double *)llzs_malloc(csd_cell_bytes(f, sizeof(double)));
        f->d_carry[0] = (float *)llzs_malloc(2 * csd_cell_bytes(f, sizeof(float)));
        f->d_carry[1] = (float *)llzs_malloc(2 * csd_cell_bytes(f, sizeof(float)));
        if (f->keep) {
            f->d_hist[0] = (float *)llzs_malloc(hist);
            f->d_hist[1] = (float *)llzs_malloc(hist);
        }
        int rc = LLZ_OK;
        if (!f->d_w || !f->d_cs || !f->d_pairs || !f->d_acc || !f->d_carry[0] || !f->d_carry[1] || (f->keep && (!f->d_hist[0] || !f->d_hist[1]))) {
            rc = LLZ_ERR_NOMEM;
            llzs_set_error("llz_csd_mc_init: device allocation failed (channels %d pairs %d fft_len %d: %zu bytes of sums, "
                           "2 x %zu bytes of history)", channels, pairs, N, csd_cell_bytes(f, sizeof(double) + 4 * sizeof(float)), hist);
        }
        if (rc == LLZ_OK) rc = csd_clear(f);
        if (rc == LLZ_OK) rc = llzs_sync(NULL);
        if (rc != LLZ_OK) {
            csdm_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

void llz_csd_mc_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_CSDM, csdm_destroy); }

static csdm_t *csd_handle(unsigned long handle, const char *who) { return (csdm_t *)llz_handle(handle, LLZ_TAG_CSDM, who); }

int llz_csd_mc_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_CSDM, "llz_csd_mc_set_stream", stream);
}

long llz_csd_mc_frames(unsigned long handle)
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_frames");
    return f ? csd_frames_at(f, f->hops) : LLZ_ERR_ARG;
}

/* runs the partial scratch may hold at once: the cap (or the csd_scratch_kb tune) over one run's partials, one at least */
static long csd_runs_per_walk(const csdm_t *f)
{
    const int kb = llzs_tune(LLZS_TUNE_CSD_SCRATCH_KB);
    const size_t cap = kb > 0 ? (size_t)kb << 10 : CSD_SCRATCH_BYTES;
    const long runs = (long)(cap / csd_cell_bytes(f, sizeof(float)));
    return runs > 0 ? runs : 1;
}

/* the frames [f_lo, f_hi) an update of n samples adds, and the runs they touch */
static int csd_span(const csdm_t *f, const char *who, long n, long *f_lo, long *f_hi)
{
    if (n < f->hop || n % f->hop != 0 || n / f->hop > 0x3fffffffL) {
        llzs_set_error("%s: n %ld (a multiple of hop %d, at least one hop)", who, n, f->hop);
        return LLZ_ERR_ARG;
    }
    *f_lo = csd_frames_at(f, f->hops);
    *f_hi = csd_frames_at(f, f->hops + n / f->hop);
    return LLZ_OK;
}

int llz_csd_mc_plan(unsigned long handle, long n, int out[4])
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_plan");
    long f_lo, f_hi;
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("llz_csd_mc_plan: out NULL");
        return LLZ_ERR_ARG;
    }
    if (csd_span(f, "llz_csd_mc_plan", n, &f_lo, &f_hi) != LLZ_OK) return LLZ_ERR_ARG;
    const long runs = f_hi > f_lo ? (f_hi - 1) / LLZ_CSD_RUN - f_lo / LLZ_CSD_RUN + 1 : 0;
    const long per = csd_runs_per_walk(f);
    out[0] = llzs_csd_form(f->fft_len);
    out[1] = LLZ_CSD_RUN;
    out[2] = (int)(runs < per ? runs : per);
    out[3] = (int)((runs + per - 1) / per);
    return LLZ_OK;
}

long llz_csd_mc_update(unsigned long handle, const float *x, long n)
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_update");
    long f_lo, f_hi;
    if (!f) return LLZ_ERR_ARG;
    if (!x) {
        llzs_set_error("llz_csd_mc_update: x NULL");
        return LLZ_ERR_ARG;
    }
    if (csd_span(f, "llz_csd_mc_update", n, &f_lo, &f_hi) != LLZ_OK) return LLZ_ERR_ARG;
    const size_t xb = sizeof(float) * (size_t)f->channels * (size_t)n;
    const int prev = llzs_device_enter(f->head.device);
    const int x_dev = llzs_is_device_ptr(x);
    int rc = x_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;                     /* a buffer of another GPU: refused, message set */
    const float *d_x = (const float *)llz_stage_in(&f->st_x, x, xb, x_dev, f->head.stream, &rc);
    if (rc == LLZ_OK && f_hi > f_lo) {
        const long r_lo = f_lo / LLZ_CSD_RUN, r_hi = (f_hi - 1) / LLZ_CSD_RUN, per = csd_runs_per_walk(f);
        const long most = r_hi - r_lo + 1 < per ? r_hi - r_lo + 1 : per;
        float *scratch = (float *)llz_stage_reserve(&f->st_scratch, (size_t)most * csd_cell_bytes(f, sizeof(float)));
        if (!scratch) {
            llzs_set_error("llz_csd_mc_update: no device memory for %ld runs of partials (%zu bytes each)", most,
                           csd_cell_bytes(f, sizeof(float)));
            rc = LLZ_ERR_NOMEM;
        }
        /* per slab of runs: the runs, then the fold of the finished ones; a slab's launches follow the previous slab's on the stream */
        for (long r0 = r_lo; rc == LLZ_OK && r0 <= r_hi; r0 += per) {
            const long nruns = r_hi - r0 + 1 < per ? r_hi - r0 + 1 : per;
            long nfin = f_hi / LLZ_CSD_RUN - r0;                   /* runs [r0, f_hi / 32) end inside the call */
            if (nfin > nruns) nfin = nruns;
            rc = llzs_csd_runs_f32(d_x, f->d_hist[f->cur], f->d_w, f->d_cs, f->d_pairs, scratch, f->d_carry[f->cur_carry],
                                   f->d_carry[f->cur_carry ^ 1], f->pairs, f->fft_len, f->hop, n, f->hops, f_lo, f_hi, r0,
                                   (int)nruns, f->head.stream);
            if (rc == LLZ_OK && nfin > 0) rc = llzs_csd_fold_f64(scratch, f->d_acc, f->pairs, f->bins, (int)nfin, f->head.stream);
        }
        /* the call left a run open: its partial is in the other buffer (a call without a frame keeps the open run where it is) */
        if (rc == LLZ_OK && f_hi % LLZ_CSD_RUN) f->cur_carry ^= 1;
    }
    /* history for the next call: the last fft_len - hop samples of concat(history, x) */
    if (rc == LLZ_OK && f->keep) {
        rc = llzs_fir_tail_f32(d_x, f->d_hist[f->cur], f->d_hist[f->cur ^ 1], f->channels, n, n, f->keep + 1, f->head.stream);
        if (rc == LLZ_OK) f->cur ^= 1;
    }
    if (rc == LLZ_OK) f->hops += n / f->hop;
    if (rc == LLZ_OK && !x_dev) rc = llzs_sync(f->head.stream);         /* the stage may be reused by the next call */
    llzs_device_leave(prev);
    return rc == LLZ_OK ? csd_frames_at(f, f->hops) : rc;
}

static int csd_read(csdm_t *f, const char *who, int what, void *out, size_t bytes)
{
    const long K = csd_frames_at(f, f->hops);
    if (!out) {
        llzs_set_error("%s: out NULL", who);
        return LLZ_ERR_ARG;
    }
    if (K < 1) {
        llzs_set_error("%s: no frame yet (%ld of the first %d samples have arrived)", who, f->hops * f->hop, f->fft_len);
        return LLZ_ERR_ARG;
    }
    const int prev = llzs_device_enter(f->head.device);
    const int o_dev = llzs_is_device_ptr(out);
    int rc = o_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;
    void *d_out = llz_stage_out(&f->st_out, out, bytes, o_dev, &rc);
    if (rc == LLZ_OK)
        rc = llzs_csd_read_f64(f->d_acc, K % LLZ_CSD_RUN ? f->d_carry[f->cur_carry] : NULL, f->pairs, f->bins, what, (double)K * f->u,
                               what == CSD_READ_RAW ? NULL : (float *)d_out, what == CSD_READ_RAW ? (double *)d_out : NULL,
                               f->head.stream);
    if (rc == LLZ_OK && !o_dev) rc = llzs_d2h(out, d_out, bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_csd_mc_read(unsigned long handle, int what, float *out)
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_read");
    if (!f) return LLZ_ERR_ARG;
    if (what < LLZ_SPEC_PXX || what > LLZ_SPEC_TF) {
        llzs_set_error("llz_csd_mc_read: what %d (LLZ_SPEC_PXX .. LLZ_SPEC_TF: 0..4)", what);
        return LLZ_ERR_ARG;
    }
    const size_t wide = (what == LLZ_SPEC_CSD || what == LLZ_SPEC_TF) ? 2 : 1;
    return csd_read(f, "llz_csd_mc_read", what, out, sizeof(float) * wide * (size_t)f->pairs * (size_t)f->bins);
}

int llz_csd_mc_read_raw(unsigned long handle, double *out)
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_read_raw");
    if (!f) return LLZ_ERR_ARG;
    return csd_read(f, "llz_csd_mc_read_raw", CSD_READ_RAW, out, csd_cell_bytes(f, sizeof(double)));
}

int llz_csd_mc_reset(unsigned long handle)
{
    csdm_t *f = csd_handle(handle, "llz_csd_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = csd_clear(f);
    llzs_device_leave(prev);
    return rc;
}
