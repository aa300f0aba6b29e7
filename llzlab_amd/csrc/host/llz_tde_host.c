/*
 * llz_tde_host.c -- handle layer of the time-delay estimator (include/llz_tde.h; kernels/tde.hip): the window and twiddle
 * tables, the pair table, the history ping-pong and the frame grid (those of llz_spectral_host.c), the recursion's state and the
 * last curve on the device, the refusals of a call, and the staging of host outputs whose rows are out_pitch apart.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_tde.h"
#include "llz_host.h"

#define LLZ_TAG_TDEM 0x4c5a5444

typedef struct {
    llz_head_t head;
    int channels, pairs, fft_len, hop, bins, keep;
    int max_lag, weight, k_lo, k_hi;
    float lam, g, delta;
    long hops;                      /* hops of every channel's stream taken since the last reset */
    float *d_w, *d_cs;
    int *d_pairs;
    float *d_hist[2];               /* [channels][fft_len - hop], the samples in front of the next call */
    int cur;
    float *d_state;                 /* [pairs][bins][4] = Re S, Im S, Gx, Gy; valid once a frame has run */
    float *d_curve;                 /* [pairs][2 max_lag + 1] of the last frame */
    llz_stage_t st_x, st_delay, st_peak;
    float *h_rows;                  /* HOST: a call's staged output rows on their way to the caller's pitch */
    size_t h_rows_bytes;
} tdem_t;

static long tde_frames_at(const tdem_t *f, long hops)
{
    const long lead = f->fft_len / f->hop - 1;      /* hops before the first whole frame */
    return hops > lead ? hops - lead : 0;
}

static size_t tde_state_bytes(const tdem_t *f) { return sizeof(float) * 4 * (size_t)f->pairs * (size_t)f->bins; }
static size_t tde_curve_bytes(const tdem_t *f) { return sizeof(float) * (size_t)f->pairs * (size_t)(2 * f->max_lag + 1); }

static void tdem_destroy(void *p)
{
    tdem_t *f = (tdem_t *)p;
    llzs_free(f->d_w); llzs_free(f->d_cs); llzs_free(f->d_pairs);
    llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]); llzs_free(f->d_state); llzs_free(f->d_curve);
    llz_stage_release(&f->st_x); llz_stage_release(&f->st_delay); llz_stage_release(&f->st_peak);
    free(f->h_rows);
    f->head.tag = 0;
    free(f);
}

static int tde_clear(tdem_t *f)
{
    int rc = llzs_memset(f->d_state, 0, tde_state_bytes(f), f->head.stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_curve, 0, tde_curve_bytes(f), f->head.stream);
    for (int k = 0; k < 2 && rc == LLZ_OK && f->keep; k++)
        rc = llzs_memset(f->d_hist[k], 0, sizeof(float) * (size_t)f->channels * (size_t)f->keep, f->head.stream);
    if (rc == LLZ_OK) f->hops = 0;
    return rc;
}

static int tde_refuse_lam(const char *who, float lam)
{
    if (lam >= 0.0f && lam < 1.0f) return 0;
    llzs_set_error("%s: lam %g outside [0, 1)", who, (double)lam);
    return 1;
}

unsigned long llz_tde_mc_init(int channels, int pairs, const int *pair_xy, int fft_len, int hop, win_t win_type,
                              int max_lag, int weight, int k_lo, int k_hi, float lam, float delta)
{
    const int N = fft_len;
    if (channels < 1 || pairs < 1 || !pair_xy) {
        llzs_set_error("llz_tde_mc_init: channels %d pairs %d pair_xy %p (channels >= 1, pairs >= 1, a host table)", channels,
                       pairs, (const void *)pair_xy);
        return LLZ_BAD_HANDLE;
    }
    if (N < 64 || N > 4096 || (N & (N - 1)) != 0) {
        llzs_set_error("llz_tde_mc_init: fft_len %d (a power of two in 64..4096)", N);
        return LLZ_BAD_HANDLE;
    }
    if (hop != N && hop != N / 2 && hop != N / 4) {
        llzs_set_error("llz_tde_mc_init: hop %d (fft_len %d: one of %d, %d, %d)", hop, N, N, N / 2, N / 4);
        return LLZ_BAD_HANDLE;
    }
    for (int p = 0; p < 2 * pairs; p++)
        if (pair_xy[p] < 0 || pair_xy[p] >= channels) {
            llzs_set_error("llz_tde_mc_init: pair %d names channel %d (channels %d: 0..%d)", p / 2, pair_xy[p], channels,
                           channels - 1);
            return LLZ_BAD_HANDLE;
        }
    if (max_lag < 1 || max_lag > N / 2 - 1) {
        llzs_set_error("llz_tde_mc_init: max_lag %d outside 1..%d (fft_len %d)", max_lag, N / 2 - 1, N);
        return LLZ_BAD_HANDLE;
    }
    if (weight < LLZ_TDE_CC || weight > LLZ_TDE_SCOT) {
        llzs_set_error("llz_tde_mc_init: weight %d (LLZ_TDE_CC, LLZ_TDE_PHAT, LLZ_TDE_SCOT: 0..2)", weight);
        return LLZ_BAD_HANDLE;
    }
    if (k_lo < 0 || k_hi < k_lo || k_hi > N / 2) {
        llzs_set_error("llz_tde_mc_init: bins k_lo %d k_hi %d (0 <= k_lo <= k_hi <= %d)", k_lo, k_hi, N / 2);
        return LLZ_BAD_HANDLE;
    }
    if (tde_refuse_lam("llz_tde_mc_init", lam)) return LLZ_BAD_HANDLE;
    if (!(delta >= 0.0f) || isinf(delta)) {
        llzs_set_error("llz_tde_mc_init: delta %g is not a finite value of at least 0", (double)delta);
        return LLZ_BAD_HANDLE;
    }
    double *w = (double *)malloc(sizeof(double) * (size_t)N);
    if (w && !llz_host_window(w, N, win_type)) {
        llzs_set_error("llz_tde_mc_init: unknown window %d", (int)win_type);
        free(w);
        return LLZ_BAD_HANDLE;
    }
    tdem_t *f = w ? (tdem_t *)llz_handle_new(sizeof(*f), LLZ_TAG_TDEM, 1) : NULL;
    if (f) {
        f->channels = channels; f->pairs = pairs;
        f->fft_len = N; f->hop = hop; f->bins = N / 2 + 1; f->keep = N - hop;
        f->max_lag = max_lag; f->weight = weight; f->k_lo = k_lo; f->k_hi = k_hi;
        f->lam = lam; f->g = (float)(1.0 - (double)lam); f->delta = delta;
        const size_t hist = sizeof(float) * (size_t)channels * (size_t)f->keep;
        f->d_w = llz_host_upload_f32(w, (size_t)N);
        f->d_cs = llz_host_cs_f32(N);
        f->d_pairs = (int *)llz_host_upload(pair_xy, sizeof(int) * 2 * (size_t)pairs);
        f->d_state = (float *)llzs_malloc(tde_state_bytes(f));
        f->d_curve = (float *)llzs_malloc(tde_curve_bytes(f));
        if (f->keep) {
            f->d_hist[0] = (float *)llzs_malloc(hist);
            f->d_hist[1] = (float *)llzs_malloc(hist);
        }
        int rc = LLZ_OK;
        if (!f->d_w || !f->d_cs || !f->d_pairs || !f->d_state || !f->d_curve || (f->keep && (!f->d_hist[0] || !f->d_hist[1]))) {
            rc = LLZ_ERR_NOMEM;
            llzs_set_error("llz_tde_mc_init: device allocation failed (channels %d pairs %d fft_len %d: %zu bytes of state, "
                           "2 x %zu bytes of history)", channels, pairs, N, tde_state_bytes(f), hist);
        }
        if (rc == LLZ_OK) rc = tde_clear(f);
        if (rc == LLZ_OK) rc = llzs_sync(NULL);
        if (rc != LLZ_OK) {
            tdem_destroy(f);
            f = NULL;
        }
    }
    free(w);
    return f ? (unsigned long)f : LLZ_BAD_HANDLE;
}

void llz_tde_mc_uninit(unsigned long h) { llz_handle_retire(h, LLZ_TAG_TDEM, tdem_destroy); }

static tdem_t *tde_handle(unsigned long h, const char *who) { return (tdem_t *)llz_handle(h, LLZ_TAG_TDEM, who); }

int llz_tde_mc_set_stream(unsigned long h, void *stream)
{
    return llz_handle_set_stream(h, LLZ_TAG_TDEM, "llz_tde_mc_set_stream", stream);
}

long llz_tde_mc_frames(unsigned long h)
{
    tdem_t *f = tde_handle(h, "llz_tde_mc_frames");
    return f ? tde_frames_at(f, f->hops) : LLZ_ERR_ARG;
}

/* the frames [f_lo, f_hi) a call of n samples completes */
static int tde_span(const tdem_t *f, const char *who, long n, long *f_lo, long *f_hi)
{
    if (n < f->hop || n % f->hop != 0 || n / f->hop > 0x3fffffffL) {
        llzs_set_error("%s: n %ld (a multiple of hop %d, at least one hop)", who, n, f->hop);
        return LLZ_ERR_ARG;
    }
    *f_lo = tde_frames_at(f, f->hops);
    *f_hi = tde_frames_at(f, f->hops + n / f->hop);
    return LLZ_OK;
}

long llz_tde_mc_frames_for(unsigned long h, long n)
{
    tdem_t *f = tde_handle(h, "llz_tde_mc_frames_for");
    long f_lo, f_hi;
    if (!f || tde_span(f, "llz_tde_mc_frames_for", n, &f_lo, &f_hi) != LLZ_OK) return LLZ_ERR_ARG;
    return f_hi - f_lo;
}

/* rows of `frames` floats from the stage (rows `frames` apart) to the caller's host rows, out_pitch apart */
static int tde_rows_back(tdem_t *f, float *user, const float *d_rows, long frames, long out_pitch)
{
    const size_t bytes = sizeof(float) * (size_t)f->pairs * (size_t)frames;
    if (f->h_rows_bytes < bytes) {
        float *grown = (float *)realloc(f->h_rows, bytes);
        if (!grown) {
            llzs_set_error("llz_tde_mc_process: no host memory for %zu bytes of staged rows", bytes);
            return LLZ_ERR_NOMEM;
        }
        f->h_rows = grown;
        f->h_rows_bytes = bytes;
    }
    const int rc = llzs_d2h(f->h_rows, d_rows, bytes, f->head.stream);
    for (int p = 0; rc == LLZ_OK && p < f->pairs; p++)
        memcpy(user + (size_t)p * (size_t)out_pitch, f->h_rows + (size_t)p * (size_t)frames, sizeof(float) * (size_t)frames);
    return rc;
}

long llz_tde_mc_process(unsigned long h, const float *x, long n, float *delay, float *peak, long out_pitch)
{
    static const char who[] = "llz_tde_mc_process";
    tdem_t *f = tde_handle(h, who);
    long f_lo, f_hi;
    if (!f) return LLZ_ERR_ARG;
    if (!x || !delay) {
        llzs_set_error("%s: %s NULL", who, !x ? "x" : "delay");
        return LLZ_ERR_ARG;
    }
    if (tde_span(f, who, n, &f_lo, &f_hi) != LLZ_OK) return LLZ_ERR_ARG;
    const long frames = f_hi - f_lo;
    if (out_pitch < frames || out_pitch > 0x3fffffffL) {
        llzs_set_error("%s: out_pitch %ld below the %ld frames this call completes", who, out_pitch, frames);
        return LLZ_ERR_ARG;
    }
    const size_t xb = sizeof(float) * (size_t)f->channels * (size_t)n;
    const size_t ob = sizeof(float) * (size_t)f->pairs * (size_t)out_pitch;       /* a caller's output, as declared */
    const size_t sb = sizeof(float) * (size_t)f->pairs * (size_t)frames;          /* a staged one */
    const int prev = llzs_device_enter(f->head.device);
    const int x_dev = llzs_is_device_ptr(x), d_dev = llzs_is_device_ptr(delay), p_dev = peak ? llzs_is_device_ptr(peak) : 0;
    int rc = x_dev < 0 || d_dev < 0 || p_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;          /* a buffer of another GPU: refused, message set */
    if (rc == LLZ_OK) rc = llz_refuse_device_overlap(who, "x", x, xb, x_dev, "delay", delay, ob, d_dev);
    if (rc == LLZ_OK && peak) rc = llz_refuse_device_overlap(who, "x", x, xb, x_dev, "peak", peak, ob, p_dev);
    if (rc == LLZ_OK && peak) rc = llz_refuse_device_overlap(who, "delay", delay, ob, d_dev, "peak", peak, ob, p_dev);
    if (rc != LLZ_OK) {
        llzs_device_leave(prev);
        return rc;
    }
    const float *d_x = (const float *)llz_stage_in(&f->st_x, x, xb, x_dev, f->head.stream, &rc);
    float *d_delay = delay, *d_peak = peak;
    if (rc == LLZ_OK && frames > 0) {
        /* host outputs are staged with their rows `frames` apart, and only what the call wrote goes back */
        if (!d_dev) d_delay = (float *)llz_stage_out(&f->st_delay, NULL, sb, 0, &rc);
        if (peak && !p_dev) d_peak = (float *)llz_stage_out(&f->st_peak, NULL, sb, 0, &rc);
        if (rc == LLZ_OK)
            rc = llzs_tde_frames_f32(d_x, f->d_hist[f->cur], f->d_w, f->d_cs, f->d_pairs, f->d_state, f->d_curve, d_delay, d_peak,
                                     f->pairs, f->fft_len, f->hop, n, f->hops, f_lo, f_hi, d_dev ? out_pitch : frames, p_dev ? out_pitch : frames, f->max_lag,
                                     f->weight, f->k_lo, f->k_hi, f->lam, f->g, f->delta, f->head.stream);
    }
    /* history for the next call: the last fft_len - hop samples of concat(history, x) */
    if (rc == LLZ_OK && f->keep) {
        rc = llzs_fir_tail_f32(d_x, f->d_hist[f->cur], f->d_hist[f->cur ^ 1], f->channels, n, n, f->keep + 1, f->head.stream);
        if (rc == LLZ_OK) f->cur ^= 1;
    }
    if (rc == LLZ_OK) f->hops += n / f->hop;
    if (rc == LLZ_OK && frames > 0 && !d_dev) rc = tde_rows_back(f, delay, d_delay, frames, out_pitch);
    if (rc == LLZ_OK && frames > 0 && peak && !p_dev) rc = tde_rows_back(f, peak, d_peak, frames, out_pitch);
    if (rc == LLZ_OK && !x_dev) rc = llzs_sync(f->head.stream);         /* the stage may be reused by the next call */
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frames : rc;
}

int llz_tde_mc_read(unsigned long h, int what, float *out)
{
    static const char who[] = "llz_tde_mc_read";
    tdem_t *f = tde_handle(h, who);
    if (!f) return LLZ_ERR_ARG;
    if (what != LLZ_TDE_CURVE && what != LLZ_TDE_STATE) {
        llzs_set_error("%s: what %d (LLZ_TDE_CURVE, LLZ_TDE_STATE: 0..1)", who, what);
        return LLZ_ERR_ARG;
    }
    if (!out) {
        llzs_set_error("%s: out NULL", who);
        return LLZ_ERR_ARG;
    }
    if (tde_frames_at(f, f->hops) < 1) {
        llzs_set_error("%s: no frame yet (%ld of the first %d samples have arrived)", who, f->hops * f->hop, f->fft_len);
        return LLZ_ERR_ARG;
    }
    const float *src = what == LLZ_TDE_CURVE ? f->d_curve : f->d_state;
    const size_t bytes = what == LLZ_TDE_CURVE ? tde_curve_bytes(f) : tde_state_bytes(f);
    const int prev = llzs_device_enter(f->head.device);
    const int o_dev = llzs_is_device_ptr(out);
    int rc = o_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;
    if (rc == LLZ_OK) rc = o_dev ? llzs_d2d(out, src, bytes, f->head.stream) : llzs_d2h(out, src, bytes, f->head.stream);
    llzs_device_leave(prev);
    return rc;
}

int llz_tde_mc_set_forget(unsigned long h, float lam)
{
    tdem_t *f = tde_handle(h, "llz_tde_mc_set_forget");
    if (!f || tde_refuse_lam("llz_tde_mc_set_forget", lam)) return LLZ_ERR_ARG;
    f->lam = lam;
    f->g = (float)(1.0 - (double)lam);
    return LLZ_OK;
}

int llz_tde_mc_reset(unsigned long h)
{
    tdem_t *f = tde_handle(h, "llz_tde_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->head.device);
    const int rc = tde_clear(f);
    llzs_device_leave(prev);
    return rc;
}
