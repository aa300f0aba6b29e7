/*
 * llz_fir_host.c -- handle layer of the FIR path: the reference's single-channel `double` symbols
 * (reference libllzfilter/llz_fir.c:442-625) and the multi-channel float32 batch extension.  Plain C; the device
 * is reached only through llz_shim.h.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_fir.h"
#include "llz_host.h"

/* =====================================================================================================
 * Part 1: single channel, double, bit-exact with the reference (exact-order kernel k_fir_td_f64_exact)
 * ===================================================================================================== */

typedef struct {
    int tag;
    int flt_len, frame_len;
    double *h;          /* host taps */
    double *xbuf;       /* host: [flt_len-1 history | frame_len samples] */
    double *d_taps;     /* device taps */
    double *d_x;        /* device: same layout as xbuf */
    double *d_y;        /* device: frame_len outputs */
} fir1_t;

static void fir1_destroy(fir1_t *f)
{
    if (!f) return;
    free(f->h); free(f->xbuf);
    llzs_free(f->d_taps); llzs_free(f->d_x); llzs_free(f->d_y);
    f->tag = 0;
    free(f);
}

static unsigned long fir1_create(int kind, int frame_len, int flt_len, double fc1, double fc2, win_t win)
{
    if (frame_len < 1 || flt_len < 1) {
        llzs_set_error("llz_fir_filter_*_init: frame_len %d / flt_len %d", frame_len, flt_len);
        return LLZ_BAD_HANDLE;
    }
    fir1_t *f = (fir1_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIR1;
    f->frame_len = frame_len;
    f->flt_len = llz_host_design(kind, &f->h, flt_len, fc1, fc2, win);    /* stored length = returned length */
    if (f->flt_len < 1) {
        llzs_set_error("llz_fir_filter_*_init: tap design failed (win_type %d)", win);
        fir1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    /* flush feeds flt_len-1 zeros, so the frame area must hold max(frame_len, flt_len-1) samples */
    const int keep = f->flt_len - 1;
    const int span = keep + (frame_len > keep ? frame_len : keep) + 1;
    f->xbuf = (double *)calloc((size_t)span, sizeof(double));            /* zero history: llz_fir.c:459 */
    f->d_taps = (double *)llzs_malloc(sizeof(double) * (size_t)f->flt_len);
    f->d_x = (double *)llzs_malloc(sizeof(double) * (size_t)span);
    f->d_y = (double *)llzs_malloc(sizeof(double) * (size_t)(span - keep));
    if (!f->xbuf || !f->d_taps || !f->d_x || !f->d_y ||
        llzs_h2d(f->d_taps, f->h, sizeof(double) * (size_t)f->flt_len, NULL) != LLZ_OK) {
        fir1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_filter_lpf_init(int frame_len, int flt_len, double fc, win_t win_type)
{
    return fir1_create(LLZ_KIND_LPF, frame_len, flt_len, fc, 0.0, win_type);
}

unsigned long llz_fir_filter_hpf_init(int frame_len, int flt_len, double fc, win_t win_type)
{
    return fir1_create(LLZ_KIND_HPF, frame_len, flt_len, fc, 0.0, win_type);
}

unsigned long llz_fir_filter_bandpass_init(int frame_len, int flt_len, double fc1, double fc2, win_t win_type)
{
    return fir1_create(LLZ_KIND_BPF, frame_len, flt_len, fc1, fc2, win_type);
}

unsigned long llz_fir_filter_bandstop_init(int frame_len, int flt_len, double fc1, double fc2, win_t win_type)
{
    return fir1_create(LLZ_KIND_BSF, frame_len, flt_len, fc1, fc2, win_type);
}

void llz_fir_filter_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, fir1_t, LLZ_TAG_FIR1))
        fir1_destroy((fir1_t *)handle);
}

/* run `count` samples sitting behind the history in xbuf through the device; copy `emit` results out */
static int fir1_run(fir1_t *f, int count, double *dst, int emit)
{
    const int keep = f->flt_len - 1;
    const int span = count > emit ? count : emit;
    int rc = llzs_h2d(f->d_x, f->xbuf, sizeof(double) * (size_t)(keep + span), NULL);
    if (rc == LLZ_OK)
        rc = llzs_fir_td_f64(f->d_x + keep, f->d_y, f->d_x, f->d_taps, emit, f->flt_len, NULL);
    if (rc == LLZ_OK)
        rc = llzs_d2h(dst, f->d_y, sizeof(double) * (size_t)emit, NULL);
    /* new history = last keep samples of [history | the init frame length] (llz_fir.c:562-564) */
    memmove(f->xbuf, f->xbuf + count, sizeof(double) * (size_t)keep);
    return rc;
}

int llz_fir_filter(unsigned long handle, double *buf_in, double *buf_out, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, fir1_t, LLZ_TAG_FIR1) || !buf_in || !buf_out) {
        llzs_set_error("llz_fir_filter: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    fir1_t *f = (fir1_t *)handle;
    if (frame_len != f->frame_len) {
        /* the reference asserts frame_len <= init and mis-shifts its history for anything shorter */
        llzs_set_error("llz_fir_filter: frame_len %d != init frame_len %d", frame_len, f->frame_len);
        return LLZ_ERR_ARG;
    }
    memcpy(f->xbuf + (f->flt_len - 1), buf_in, sizeof(double) * (size_t)frame_len);
    const int rc = fir1_run(f, frame_len, buf_out, frame_len);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_fir_filter_flush(unsigned long handle, double *buf_out)
{
    if (!LLZ_HANDLE_OK(handle, fir1_t, LLZ_TAG_FIR1) || !buf_out) {
        llzs_set_error("llz_fir_filter_flush: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    fir1_t *f = (fir1_t *)handle;
    const int keep = f->flt_len - 1;
    if (keep == 0) return 0;
    /* llz_fir.c:608-622: a frame of zeros goes in, the first flt_len-1 outputs come out.  (The reference reads
     * past its buffer when flt_len-2 >= frame_len; here the frame area is always large enough and zeroed.) */
    const int zeros = f->frame_len > keep ? f->frame_len : keep;
    memset(f->xbuf + keep, 0, sizeof(double) * (size_t)zeros);
    const int rc = fir1_run(f, f->frame_len, buf_out, keep);
    return rc == LLZ_OK ? keep : rc;
}

/* =====================================================================================================
 * Part 2: multi-channel float32 batch (kernels K1 k_fir_td_f32 and K4 k_fir_ols_f32)
 * ===================================================================================================== */

typedef struct {
    int tag;                    /* LLZ_TAG_FIRM: one tap set for every channel; LLZ_TAG_FIRB: the filter bank of part 3 */
    const char *who;            /* the process symbol's name, for messages */
    int device;                 /* the device the handle's buffers live on: every call binds it */
    int channels, frame_len, flt_len, algo;
    float *d_taps;              /* flt_len floats zero-padded to a multiple of 16; a bank: [channels] such rows */
    llzs_ols_tables ols;        /* overlap-save tables (all NULL for the time-domain algorithms); a bank: twid alone */
    float *d_hbank;             /* a bank on overlap-save: [channels][LLZS_BANK_PITCH] complex, bins 0..512 of each spectrum */
    float *d_hist[2];           /* [channels][flt_len-1], ping-pong */
    int cur;
    float *d_zero;              /* [channels][flt_len-1] zeros: flush input */
    int part_n;                 /* LLZ_FIR_ALGO_PARTITIONED: transform points, fixed at init (0 for every other algo) */
    float *d_hpart, *d_ptw;     /* ... [P][part_n] partition spectra and [part_n / 2] twiddles (llzs_fir_part_f32); a bank:
                                 * [channels][P][part_n] (llzs_fir_part_bank_f32) and no d_taps */
    float *d_scratch;           /* ... block spectra of one pass of channels */
    size_t scratch_bytes;
    void *stream;
    llz_stage_t st_in, st_out;  /* only for callers passing host memory */
} firm_t;

static void firm_destroy(firm_t *f)
{
    if (!f) return;
    llzs_free(f->d_taps); llzs_free(f->d_hbank); llzs_free(f->ols.hfreq); llzs_free(f->ols.hreal); llzs_free(f->ols.twid); llzs_free(f->ols.tw2k); llzs_free(f->ols.tw4k);
    llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]); llzs_free(f->d_zero);
    llzs_free(f->d_hpart); llzs_free(f->d_ptw); llzs_free(f->d_scratch);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    f->tag = 0;
    free(f);
}

/* The overlap-save sizes: algo, transform points, the taps the rung accepts, and auto_max: AUTO takes the first rung whose
 * auto_max holds the filter (from 33 taps on; up to 32 the time domain).  auto_max is a crossover measured on 4096 ch x 2^20
 * (tools/fir_crossover.py), not the rung's limit.  Beyond the last rung AUTO takes the time domain: the matrix-core form where
 * the filter fits its LDS image (it never does there: that form ends at 1521 taps), else k_fir_td_f32, up to 25248 taps. */
static const struct firm_ols_rung {
    int algo, nfft, min_taps, max_taps, auto_max;
} FIRM_OLS[] = {
    /* time domain 6.0 / 6.4 / 7.9 / 9.5 ms at 9 / 17 / 33 / 63 taps, overlap-save 6.7 ms at any length up to 257; beyond 257
     * taps the matrix-core time domain takes 23.7 ms (31.9 ms on the VALU) */
    {LLZ_FIR_ALGO_OVERLAP_SAVE, 1024, 1, 257, 257},
    /* 2048 points with 512 of overlap 7.8 ms up to 513 taps (10.6 ms with 1024 of overlap); 4096 points 8.0 / 7.9 / 8.3 / 9.6 /
     * 11.3 / 14.7 / 19.5 ms with 512 / 768 / 1024 / 1536 / 2048 / 2560 / 3072 of overlap */
    {LLZ_FIR_ALGO_OVERLAP_SAVE_2048, 2048, 2, 1025, 513},
    /* 8192 points on pairs of waves: 9.1 / 10.9 / 10.9 / 11.3 / 13.8 ms with 1536 / 2304 / 2560 / 3072 / 4096 of overlap -> from
     * 1026 taps on (4096 points: 9.4 / 11.2 / 14.4 / 19.2 ms with 1536 / 2048 / 2560 / 3072) */
    {LLZ_FIR_ALGO_OVERLAP_SAVE_4096, 4096, 2, 3073, 1025},
    {LLZ_FIR_ALGO_OVERLAP_SAVE_8192, 8192, 2, 6145, 6145},
};
#define FIRM_OLS_RUNGS ((int)(sizeof(FIRM_OLS) / sizeof(FIRM_OLS[0])))

static const struct firm_ols_rung *firm_ols_rung(int algo)
{
    for (int i = 0; i < FIRM_OLS_RUNGS; i++)
        if (FIRM_OLS[i].algo == algo) return &FIRM_OLS[i];
    return NULL;
}

/* W_N^m = exp(-2 pi j m / N) as a float pair, from the cos / sin table of size N */
static void firm_w(float *dst, const double *cs, int m)
{
    dst[0] = (float)cs[2 * m];
    dst[1] = (float)(-cs[2 * m + 1]);
}

/* The real spectrum product of the 1024-point overlap-save.  Taps that are symmetric about a centre tap c have, centred at
 * index 0 (g[n] = taps[n + c], circularly in 1024), a real spectrum, and IFFT(FFT(x) G)[p] = y[p + c] for p in [c, 1023 - c]: the
 * stored samples y[256 .. 1023] of a block are all there, c samples early.  The kernels take the shift in whole register rows
 * of 32 samples, so the form is taken for c = 32 K, K = 1..4 (65, 129, 193, 257 taps: every length of that kind the library
 * designs is symmetric), and only where the float taps mirror bit for bit -- the dropped imaginary part is then rounding of
 * the cos / sin table alone.  Returns K, or 0 for the complex product (also under the ols_real_product = 0 tune). */
int llz_host_ols_real_rows(const float *taps, int flt_len)
{
    const int c = (flt_len - 1) / 2;
    if (llzs_tune(LLZS_TUNE_OLS_REAL_PRODUCT) == 0 || flt_len % 2 == 0 || c % 32 != 0 || c < 32 || c > 128) return 0;
    for (int i = 0; i < c; i++)
        if (memcmp(&taps[i], &taps[flt_len - 1 - i], sizeof(float)) != 0) return 0;
    return c / 32;
}

/* dst[k] = Re DFT_1024(g)[k] / 1024, k < 1024 in natural order, in double from cs = llz_host_cs_table(cs, 1024) (the device
 * table is its cast to float); *imag_max (may be NULL) = the largest |Im DFT_1024(g)[k]| / 1024 that is dropped */
void llz_host_ols_real_table(double *dst, double *imag_max, const float *taps, int flt_len, const double *cs)
{
    const int c = (flt_len - 1) / 2;
    double worst = 0.0;
    for (int k = 0; k < 1024; k++) {
        double re = 0.0, im = 0.0;
        for (int t = 0; t < flt_len; t++) {
            const int m = (int)(((long)k * (t - c + 1024)) % 1024);        /* g[t - c] = taps[t] */
            re += (double)taps[t] * cs[2 * m];
            im -= (double)taps[t] * cs[2 * m + 1];
        }
        dst[k] = re / 1024;
        if (fabs(im / 1024) > worst) worst = fabs(im / 1024);
    }
    if (imag_max) *imag_max = worst;
}

/* the tables of the N-point overlap-save (llzs_ols_tables): the spectrum of the (float-rounded) taps scaled by 1/N in
 * P = N / 1024 planes, the 32 x 32 twiddles W_1024^(ab) = W_N^(P ab), W_2048^n (N = 2048, 4096) and W_4096^n (N = 4096, 8192),
 * all from one quadrant-exact cos / sin table of size N.  Direct DFT in double (up to 6145 x 8192 terms), setup time only.  1024
 * points, K = llz_host_ols_real_rows > 0: the real table of the centred taps next to them (512 complex entries' worth). */
static int firm_build_ols_tables(firm_t *f, const float *taps, int N)
{
    const int P = N / 1024;
    const int K = N == 1024 ? llz_host_ols_real_rows(taps, f->flt_len) : 0;
    /* complex entries of hfreq, twid, tw2k, tw4k, hreal (0: the rung has no such table) */
    const int count[5] = {N, 1024, (N == 2048 || N == 4096) ? 1024 : 0, N >= 4096 ? 2048 : 0, K ? 512 : 0};
    float **dev[5] = {&f->ols.hfreq, &f->ols.twid, &f->ols.tw2k, &f->ols.tw4k, &f->ols.hreal};
    float *host[5];
    int rc = LLZ_OK;
    f->ols.real_rows = K;
    for (int i = 0; i < 5; i++) {
        host[i] = count[i] ? (float *)malloc(sizeof(float) * 2 * (size_t)count[i]) : NULL;
        if (count[i] && !host[i]) rc = LLZ_ERR_NOMEM;
    }
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    if (!cs) rc = LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        float *hf = host[0], *tw = host[1], *w2 = host[2], *w4 = host[3];
        llz_host_cs_table(cs, N);
        for (int k = 0; k < N; k++) {
            double re = 0.0, im = 0.0;
            for (int t = 0; t < f->flt_len; t++) {
                const int m = (int)(((long)k * t) % N);
                re += (double)taps[t] * cs[2 * m];
                im -= (double)taps[t] * cs[2 * m + 1];
            }
            const int dst = (k % P) * 1024 + k / P;                    /* bin k -> plane k mod P, row k / P */
            hf[2 * dst] = (float)(re / N);
            hf[2 * dst + 1] = (float)(im / N);
        }
        for (int a = 0; a < 32; a++)
            for (int b = 0; b < 32; b++) firm_w(&tw[2 * (a * 32 + b)], cs, (P * a * b) % N);
        for (int i = 0; i < count[2]; i++) firm_w(&w2[2 * i], cs, i * (N / 2048));
        for (int i = 0; i < count[3]; i++) firm_w(&w4[2 * i], cs, i * (N / 4096));
        double *g = K ? (double *)malloc(sizeof(double) * 1024) : NULL;
        if (K && !g) rc = LLZ_ERR_NOMEM;
        if (g) {
            llz_host_ols_real_table(g, NULL, taps, f->flt_len, cs);
            for (int k = 0; k < 1024; k++) host[4][k] = (float)g[k];
            free(g);
        }
        /* allocate, then upload in the order hfreq, twid, tw2k, tw4k, hreal: a sharded init records the tables in upload order */
        for (int i = 0; i < 5; i++)
            if (count[i] && !(*dev[i] = (float *)llzs_malloc(sizeof(float) * 2 * (size_t)count[i]))) rc = LLZ_ERR_NOMEM;
        for (int i = 0; i < 5 && rc == LLZ_OK; i++)
            if (count[i]) rc = llzs_h2d_table(*dev[i], host[i], sizeof(float) * 2 * (size_t)count[i]);
    }
    for (int i = 0; i < 5; i++) free(host[i]);
    free(cs);
    return rc;
}

/* ---- LLZ_FIR_ALGO_PARTITIONED: uniformly partitioned overlap-save (fir_part.hip) ---- */

/* transform points by tap count: the smallest size that keeps the filter within 4 partitions, 8192 beyond.  The product kernel
 * reads (16 + P - 1) / 16 spectra per output block, so few partitions keep its scratch traffic near one read per block, and a
 * smaller transform wastes less of a short call; from 16385 taps on only more partitions remain. */
static int firm_part_nfft(int flt_len)
{
    const int forced = llzs_tune(LLZS_TUNE_PART_NFFT);
    if (forced == 1024 || forced == 2048 || forced == 4096 || forced == 8192) return forced;
    int n = 1024;
    while (n < 8192 && flt_len > 4 * (n / 2)) n *= 2;
    return n;
}

/* the scratch cap in bytes: 1 GiB, or what the part_scratch_mb tune says (1 .. 1024 MiB) */
static size_t firm_part_cap(void)
{
    const int mb = llzs_tune(LLZS_TUNE_PART_SCRATCH_MB);
    return (size_t)((mb >= 1 && mb <= 1024) ? mb : 1024) << 20;
}

/* floats of one tap row's partition spectra: [P][part_n] complex */
static size_t firm_part_row(const firm_t *f)
{
    const int B = f->part_n / 2;
    return 2 * (size_t)((f->flt_len + B - 1) / B) * (size_t)f->part_n;
}

/* the transform size and the scratch bytes of an algo-7 handle, from the tunes set now; refuses a shape of which not one
 * channel fits the cap.  Touches no device.  who: the init's name, for messages. */
static int firm_part_size(firm_t *f, const char *who)
{
    const int N = firm_part_nfft(f->flt_len), keep = f->flt_len - 1;
    const size_t cap = firm_part_cap();
    size_t need = 0, need_flush = 0;            /* per channel: a frame, and the flush's flt_len - 1 zeros */
    if (llzs_fir_part_need(N, f->flt_len, f->frame_len, &need) != LLZ_OK) return LLZ_ERR_ARG;
    if (keep > 0 && llzs_fir_part_need(N, f->flt_len, keep, &need_flush) != LLZ_OK) return LLZ_ERR_ARG;
    if (need_flush > need) need = need_flush;
    if (need > cap) {
        llzs_set_error("%s: one channel of %d samples at %d taps (%d-point partitions) needs %zu B of scratch, "
                       "the cap is %zu B", who, f->frame_len > keep ? f->frame_len : keep, f->flt_len, N, need, cap);
        return LLZ_ERR_NOMEM;
    }
    f->part_n = N;
    f->scratch_bytes = need * (size_t)f->channels < cap ? need * (size_t)f->channels : cap;
    return LLZ_OK;
}

/* the partition spectra of `rows` tap rows (1: the shared-taps handle; channels: a bank), the twiddles and the scratch of a
 * handle that firm_part_size has sized */
static int firm_build_part(firm_t *f, const float *taps, int rows, const char *who)
{
    const int N = f->part_n, P = (f->flt_len + N / 2 - 1) / (N / 2);
    const size_t hbytes = sizeof(float) * 2 * (size_t)rows * (size_t)P * (size_t)N;
    float *tw = (float *)malloc(sizeof(float) * (size_t)N);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (tw && cs) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        llz_host_cs_table(cs, N);
        for (int m = 0; m < N / 2; m++) firm_w(&tw[2 * m], cs, m);
        f->d_hpart = (float *)llzs_malloc(hbytes);
        if (!f->d_hpart) {
            llzs_set_error("%s: no device memory for the partition spectra: %zu B asked for (%d rows x %d partitions x %d points)",
                           who, hbytes, rows, P, N);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) {
        f->d_ptw = (float *)llzs_malloc(sizeof(float) * (size_t)N);
        f->d_scratch = (float *)llzs_malloc(f->scratch_bytes);
        if (!f->d_ptw || !f->d_scratch) rc = LLZ_ERR_NOMEM;
    }
    /* tables through llzs_h2d_table, in a fixed order: a sharded init records and broadcasts them */
    if (rc == LLZ_OK) rc = llz_host_load_spectra(who, f->d_hpart, firm_part_row(f), rows, taps, f->flt_len, N, 0, 1, NULL);
    if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_ptw, tw, sizeof(float) * (size_t)N);
    free(tw); free(cs);
    return rc;
}

/* what a call of n samples may use of the scratch now: the allocation, or less under the part_scratch_mb tune */
static size_t firm_part_avail(const firm_t *f)
{
    const size_t cap = firm_part_cap();
    return cap < f->scratch_bytes ? cap : f->scratch_bytes;
}

unsigned long llz_fir_filter_mc_init(int channels, int frame_len, const float *taps, int flt_len, int algo)
{
    if (channels < 1 || channels > 65535 || frame_len < 1 || !taps || flt_len < 1) {
        llzs_set_error("llz_fir_filter_mc_init: channels %d frame_len %d flt_len %d", channels, frame_len, flt_len);
        return LLZ_BAD_HANDLE;
    }
    if (algo == LLZ_FIR_ALGO_PARTITIONED) {
        if (flt_len > LLZS_FIR_PART_MAX_TAPS) {
            llzs_set_error("llz_fir_filter_mc_init: the partitioned overlap-save takes 1..%d taps, not %d", LLZS_FIR_PART_MAX_TAPS,
                           flt_len);
            return LLZ_BAD_HANDLE;
        }
    } else if (!llzs_fir_td_f32_fits(flt_len)) {
        /* every such handle flushes through the time-domain kernel (and AUTO falls back to it): refuse here, not at the first
         * call.  The partitioned form flushes through itself. */
        llzs_set_error("llz_fir_filter_mc_init: %d taps exceed the time-domain kernel's LDS tile", flt_len);
        return LLZ_BAD_HANDLE;
    }
    if (algo == LLZ_FIR_ALGO_AUTO) {
        int i = 0;
        while (i < FIRM_OLS_RUNGS && flt_len > FIRM_OLS[i].auto_max) i++;
        if (flt_len <= 32) algo = LLZ_FIR_ALGO_TIME;
        else if (i < FIRM_OLS_RUNGS) algo = FIRM_OLS[i].algo;
        else algo = llzs_fir_mfma_f32_fits(flt_len, 1) ? LLZ_FIR_ALGO_TIME_MFMA : LLZ_FIR_ALGO_TIME;
    }
    const struct firm_ols_rung *ols = firm_ols_rung(algo);
    if (ols && (flt_len < ols->min_taps || flt_len > ols->max_taps)) {
        llzs_set_error("llz_fir_filter_mc_init: the %d-point overlap-save takes %d..%d taps", ols->nfft, ols->min_taps,
                       ols->max_taps);
        return LLZ_BAD_HANDLE;
    }
    if (algo == LLZ_FIR_ALGO_TIME_MFMA && !llzs_fir_mfma_f32_fits(flt_len, 1)) {
        llzs_set_error("llz_fir_filter_mc_init: %d taps do not fit the matrix-core kernel's LDS tile", flt_len);
        return LLZ_BAD_HANDLE;
    }
    if (!ols && algo != LLZ_FIR_ALGO_TIME && algo != LLZ_FIR_ALGO_TIME_MFMA && algo != LLZ_FIR_ALGO_PARTITIONED) {
        llzs_set_error("llz_fir_filter_mc_init: unknown algo %d", algo);
        return LLZ_BAD_HANDLE;
    }
    firm_t *f = (firm_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIRM;
    f->who = "llz_fir_filter_mc";
    f->device = llzs_device_get();
    f->channels = channels; f->frame_len = frame_len; f->flt_len = flt_len; f->algo = algo;

    const int tpad = (flt_len + 15) & ~15;
    const size_t hist_bytes = sizeof(float) * (size_t)channels * (size_t)(flt_len > 1 ? flt_len - 1 : 1);
    float *padded = (float *)calloc((size_t)tpad, sizeof(float));
    int rc = padded ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        memcpy(padded, taps, sizeof(float) * (size_t)flt_len);
        f->d_taps = (float *)llzs_malloc(sizeof(float) * (size_t)tpad);
        f->d_hist[0] = (float *)llzs_malloc(hist_bytes);
        f->d_hist[1] = (float *)llzs_malloc(hist_bytes);
        f->d_zero = (float *)llzs_malloc(hist_bytes);
        if (!f->d_taps || !f->d_hist[0] || !f->d_hist[1] || !f->d_zero) rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_taps, padded, sizeof(float) * (size_t)tpad);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[0], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[1], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_zero, 0, hist_bytes, NULL);
    if (rc == LLZ_OK && ols) rc = firm_build_ols_tables(f, taps, ols->nfft);
    if (rc == LLZ_OK && algo == LLZ_FIR_ALGO_PARTITIONED) rc = firm_part_size(f, "llz_fir_filter_mc_init");
    if (rc == LLZ_OK && algo == LLZ_FIR_ALGO_PARTITIONED) rc = firm_build_part(f, taps, 1, "llz_fir_filter_mc_init");
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    free(padded);
    if (rc != LLZ_OK) {
        firm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_filter_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len, int algo)
{
    if (!taps || flt_len < 1) {
        llzs_set_error("llz_fir_filter_mc_init_f64taps: no taps");
        return LLZ_BAD_HANDLE;
    }
    float *t = llz_host_taps_f32("llz_fir_filter_mc_init_f64taps", taps, (size_t)flt_len);
    if (!t) return LLZ_BAD_HANDLE;
    unsigned long h = llz_fir_filter_mc_init(channels, frame_len, t, flt_len, algo);
    free(t);
    return h;
}

static unsigned long firm_design_init(int kind, int channels, int frame_len, int flt_len, double fc1, double fc2,
                                      win_t win)
{
    double *h = NULL;
    const int n = llz_host_design(kind, &h, flt_len, fc1, fc2, win);
    if (n < 1) {
        llzs_set_error("llz_fir_filter_mc_*_init: tap design failed");
        return LLZ_BAD_HANDLE;
    }
    unsigned long handle = llz_fir_filter_mc_init_f64taps(channels, frame_len, h, n, LLZ_FIR_ALGO_AUTO);
    free(h);
    return handle;
}

unsigned long llz_fir_filter_mc_lpf_init(int channels, int frame_len, int flt_len, double fc, win_t win_type)
{
    return firm_design_init(LLZ_KIND_LPF, channels, frame_len, flt_len, fc, 0.0, win_type);
}

unsigned long llz_fir_filter_mc_hpf_init(int channels, int frame_len, int flt_len, double fc, win_t win_type)
{
    return firm_design_init(LLZ_KIND_HPF, channels, frame_len, flt_len, fc, 0.0, win_type);
}

unsigned long llz_fir_filter_mc_bandpass_init(int channels, int frame_len, int flt_len, double fc1, double fc2,
                                              win_t win_type)
{
    return firm_design_init(LLZ_KIND_BPF, channels, frame_len, flt_len, fc1, fc2, win_type);
}

unsigned long llz_fir_filter_mc_bandstop_init(int channels, int frame_len, int flt_len, double fc1, double fc2,
                                              win_t win_type)
{
    return firm_design_init(LLZ_KIND_BSF, channels, frame_len, flt_len, fc1, fc2, win_type);
}

void llz_fir_filter_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM)) {
        firm_t *f = (firm_t *)handle;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        firm_destroy(f);
        llzs_device_leave(prev);
    }
}

int llz_fir_filter_mc_flt_len(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) ? ((firm_t *)handle)->flt_len : LLZ_ERR_ARG;
}

int llz_fir_filter_mc_real_rows(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM)) return LLZ_ERR_ARG;
    const firm_t *f = (const firm_t *)handle;
    return f->algo == LLZ_FIR_ALGO_OVERLAP_SAVE ? llzs_fir_ols_real_rows(&f->ols) : 0;
}

int llz_fir_filter_mc_algo(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) ? ((firm_t *)handle)->algo : LLZ_ERR_ARG;
}

int llz_fir_filter_mc_partition_plan(unsigned long handle, int n, int out[4])
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) || ((firm_t *)handle)->algo != LLZ_FIR_ALGO_PARTITIONED || n < 1 || !out) {
        llzs_set_error("llz_fir_filter_mc_partition_plan: not a handle of LLZ_FIR_ALGO_PARTITIONED, n %d < 1 or no out", n);
        return LLZ_ERR_ARG;
    }
    const firm_t *f = (const firm_t *)handle;
    return llzs_fir_part_plan(f->part_n, f->flt_len, n, f->channels, firm_part_avail(f), out);
}

int llz_fir_filter_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM)) return LLZ_ERR_ARG;
    ((firm_t *)handle)->stream = stream;
    return LLZ_OK;
}

/* device-side body shared by process and flush */
static int firm_launch(firm_t *f, const float *d_in, float *d_out, int n, long pitch_in, long pitch_out, int algo)
{
    const float *hist = f->flt_len > 1 ? f->d_hist[f->cur] : NULL;
    const struct firm_ols_rung *ols = firm_ols_rung(algo);
    int rc;
    if (f->tag == LLZ_TAG_FIRB && algo == LLZ_FIR_ALGO_PARTITIONED)
        rc = llzs_fir_part_bank_f32(f->part_n, f->d_hpart, f->d_ptw, f->d_scratch, firm_part_avail(f), d_in, d_out, hist,
                                    f->channels, n, pitch_in, pitch_out, f->flt_len, f->stream);
    else if (f->tag == LLZ_TAG_FIRB)
        rc = ols ? llzs_fir_bank_ols_f32(f->d_hbank, f->ols.twid, d_in, d_out, hist, f->channels, n, pitch_in, pitch_out,
                                         f->flt_len, f->stream)
                 : llzs_fir_td_bank_f32(d_in, d_out, hist, f->d_taps, f->channels, n, pitch_in, pitch_out, f->flt_len,
                                        f->stream);
    else if (ols)
        rc = llzs_fir_ols_f32(ols->nfft, &f->ols, d_in, d_out, hist, f->channels, n, pitch_in, pitch_out, f->flt_len,
                              f->stream);
    else if (algo == LLZ_FIR_ALGO_PARTITIONED)
        rc = llzs_fir_part_f32(f->part_n, f->d_hpart, f->d_ptw, f->d_scratch, firm_part_avail(f), d_in, d_out, hist, f->channels, n,
                               pitch_in, pitch_out, f->flt_len, f->stream);
    else if (algo == LLZ_FIR_ALGO_TIME_MFMA)
        rc = llzs_fir_mfma_f32(d_in, d_out, hist, f->d_taps, f->channels, n, n, pitch_in, pitch_out, f->flt_len, 1,
                               1.0f, f->stream);
    else
        rc = llzs_fir_td_f32(d_in, d_out, hist, f->d_taps, f->channels, n, pitch_in, pitch_out, f->flt_len,
                             f->stream);
    if (rc == LLZ_OK && f->flt_len > 1) {
        rc = llzs_fir_tail_f32(d_in, f->d_hist[f->cur], f->d_hist[f->cur ^ 1], f->channels, n, pitch_in,
                               f->flt_len, f->stream);
        if (rc == LLZ_OK) f->cur ^= 1;
    }
    return rc;
}

static int firm_process(firm_t *f, const float *in, float *out, int frame_len);
static int firm_flush(firm_t *f, float *out);

int llz_fir_filter_mc(unsigned long handle, const float *in, float *out, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) || !in || !out) {
        llzs_set_error("llz_fir_filter_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    const int prev = llzs_device_enter(f->device);       /* the handle's device, whatever the caller has current */
    const int rc = firm_process(f, in, out, frame_len);
    llzs_device_leave(prev);
    return rc;
}

static int firm_process(firm_t *f, const float *in, float *out, int frame_len)
{
    if (frame_len != f->frame_len) {
        llzs_set_error("%s: frame_len %d != init frame_len %d", f->who, frame_len, f->frame_len);
        return LLZ_ERR_ARG;
    }
    if (in == out) {
        llzs_set_error("%s: in-place filtering is not supported", f->who);
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)frame_len;
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    if (in_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;            /* a buffer of another GPU: refused, message set */
    if (llz_refuse_device_overlap(f->who, "in", in, bytes, in_dev, "out", out, bytes, out_dev)) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = llz_stage_in(&f->st_in, in, bytes, in_dev, f->stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc == LLZ_OK) rc = firm_launch(f, d_in, d_out, frame_len, frame_len, frame_len, f->algo);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->stream);
    return rc == LLZ_OK ? frame_len : rc;
}

/* rows of larger device buffers: the launch of firm_process with the caller's pitches, nothing staged */
int llz_fir_filter_mc_pitched(unsigned long handle, const float *in, float *out, int frame_len, long in_pitch, long out_pitch)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) || !in || !out) {
        llzs_set_error("llz_fir_filter_mc_pitched: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    if (frame_len != f->frame_len || in_pitch < frame_len || out_pitch < frame_len) {
        llzs_set_error("llz_fir_filter_mc_pitched: frame_len %d != init frame_len %d, or a pitch (%ld, %ld) below it", frame_len,
                       f->frame_len, in_pitch, out_pitch);
        return LLZ_ERR_ARG;
    }
    const int prev = llzs_device_enter(f->device);
    const size_t in_bytes = sizeof(float) * ((size_t)(f->channels - 1) * (size_t)in_pitch + (size_t)frame_len);
    const size_t out_bytes = sizeof(float) * ((size_t)(f->channels - 1) * (size_t)out_pitch + (size_t)frame_len);
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    int rc = LLZ_OK;
    if (in_dev != 1 || out_dev != 1) {
        if (in_dev >= 0 && out_dev >= 0) llzs_set_error("llz_fir_filter_mc_pitched: in and out must be device memory");
        rc = LLZ_ERR_ARG;
    } else if (llz_refuse_device_overlap("llz_fir_filter_mc_pitched", "in", in, in_bytes, in_dev, "out", out, out_bytes, out_dev)) {
        rc = LLZ_ERR_ARG;
    } else {
        rc = firm_launch(f, in, out, frame_len, in_pitch, out_pitch, f->algo);
    }
    llzs_device_leave(prev);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_fir_filter_mc_flush(unsigned long handle, float *out)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRM) || !out) {
        llzs_set_error("llz_fir_filter_mc_flush: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = firm_flush(f, out);
    llzs_device_leave(prev);
    return rc;
}

static int firm_flush(firm_t *f, float *out)
{
    const int keep = f->flt_len - 1;
    if (keep == 0) return 0;
    const size_t bytes = sizeof(float) * (size_t)f->channels * (size_t)keep;
    const int out_dev = llzs_is_device_ptr(out);
    if (out_dev < 0) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc != LLZ_OK) return rc;
    /* flt_len-1 zeros per channel through the time-domain kernel (tiny; same arithmetic as the frames); a partitioned handle
     * through the partitioned launcher at every length: above 25248 taps the time-domain kernel cannot hold the filter */
    rc = firm_launch(f, f->d_zero, d_out, keep, keep, keep,
                     f->algo == LLZ_FIR_ALGO_PARTITIONED ? LLZ_FIR_ALGO_PARTITIONED : LLZ_FIR_ALGO_TIME);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->stream);
    return rc == LLZ_OK ? keep : rc;
}

/* =====================================================================================================
 * Part 3: the filter bank -- the batch of part 2 with a tap set per channel (kernels k_fir_td_f32<true> and K4c
 * k_fir_bank_ols_f32).  A bank is a firm_t under its own tag: staging, history, tail update and flush are part 2's.
 * ===================================================================================================== */

enum { FIRB_N = 1024 };

/* dst[0 .. 512] = DFT_1024(taps)[k] / 1024 as float pairs: a radix-2 transform in double (decimation in time, twiddles from
 * the table), rounded once.  The direct DFT of firm_build_ols_tables costs 513 x flt_len terms per filter here: 4096 filters
 * of 257 taps took 0.54 s of host time that way and 0.09 s this way, with every float32 entry equal in 256 random filters
 * (profiles/fir_bank/time_fir_bank.txt).  z: 2 x 1024 doubles. */
static void firb_spectrum(float *dst, const float *taps, int flt_len, const double *cs, double *z)
{
    for (int i = 0; i < FIRB_N; i++) {
        int r = 0;
        for (int b = 0; b < 10; b++) r |= ((i >> b) & 1) << (9 - b);
        z[2 * r] = i < flt_len ? (double)taps[i] : 0.0;
        z[2 * r + 1] = 0.0;
    }
    for (int half = 1; half < FIRB_N; half *= 2) {
        const int step = FIRB_N / (2 * half);
        for (int base = 0; base < FIRB_N; base += 2 * half)
            for (int j = 0; j < half; j++) {
                const double wr = cs[2 * j * step], wi = -cs[2 * j * step + 1];
                double *a = z + 2 * (base + j), *b = a + 2 * half;
                const double tr = b[0] * wr - b[1] * wi, ti = b[0] * wi + b[1] * wr;
                b[0] = a[0] - tr; b[1] = a[1] - ti;
                a[0] += tr; a[1] += ti;
            }
    }
    for (int k = 0; k < LLZS_BANK_BINS; k++) {
        dst[2 * k] = (float)(z[2 * k] / FIRB_N);
        dst[2 * k + 1] = (float)(z[2 * k + 1] / FIRB_N);
    }
}

/* build the table rows of channels [first, first + count) from taps [count][flt_len] and upload them: at init as tables
 * (stream NULL), from set_taps on the handle's stream behind the calls already issued */
static int firb_load_rows(firm_t *f, int first, int count, const float *taps, int at_init)
{
    const int tpad = (f->flt_len + 15) & ~15;
    const size_t tbytes = sizeof(float) * (size_t)count * (size_t)tpad;
    const size_t hbytes = f->d_hbank ? sizeof(float) * 2 * (size_t)count * LLZS_BANK_PITCH : 0;
    float *pt = (float *)calloc((size_t)count * (size_t)tpad, sizeof(float));
    float *hb = hbytes ? (float *)calloc((size_t)count * LLZS_BANK_PITCH * 2, sizeof(float)) : NULL;
    double *work = hbytes ? (double *)malloc(sizeof(double) * 4 * FIRB_N) : NULL;
    int rc = (pt && (!hbytes || (hb && work))) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        if (hbytes) llz_host_cs_table(work + 2 * FIRB_N, FIRB_N);
        for (int c = 0; c < count; c++) {
            const float *row = taps + (size_t)c * (size_t)f->flt_len;
            memcpy(pt + (size_t)c * (size_t)tpad, row, sizeof(float) * (size_t)f->flt_len);
            if (hbytes) firb_spectrum(hb + (size_t)c * LLZS_BANK_PITCH * 2, row, f->flt_len, work + 2 * FIRB_N, work);
        }
        float *d_t = f->d_taps + (size_t)first * (size_t)tpad;
        float *d_h = hbytes ? f->d_hbank + (size_t)first * LLZS_BANK_PITCH * 2 : NULL;
        rc = at_init ? llzs_h2d_table(d_t, pt, tbytes) : llzs_h2d(d_t, pt, tbytes, f->stream);
        if (rc == LLZ_OK && hbytes) rc = at_init ? llzs_h2d_table(d_h, hb, hbytes) : llzs_h2d(d_h, hb, hbytes, f->stream);
    }
    free(pt); free(hb); free(work);
    return rc;
}

unsigned long llz_fir_bank_mc_init(int channels, int frame_len, const float *taps, int flt_len, int algo)
{
    if (channels < 1 || channels > 65535 || frame_len < 1 || !taps || flt_len < 1) {
        llzs_set_error("llz_fir_bank_mc_init: channels %d frame_len %d flt_len %d%s", channels, frame_len, flt_len,
                       taps ? "" : ", no taps");
        return LLZ_BAD_HANDLE;
    }
    if (!llzs_fir_td_f32_fits(flt_len)) {
        llzs_set_error("llz_fir_bank_mc_init: %d taps exceed the time-domain kernel's LDS tile", flt_len);
        return LLZ_BAD_HANDLE;
    }
    /* AUTO: the crossover of the shared form, confirmed for the bank on 4096 ch x 2^20 (tools/time_fir_bank.py,
     * profiles/fir_bank/time_fir_bank.txt, runs A / B): time domain 5.97 / 6.17 ms at 9 taps, 6.48 / 6.58 at 32, 8.03 / 8.07 at
     * 33 (K1 pads to 48) and 9.72 / 9.96 at 63, overlap-save 6.47 / 6.70 ms at every length up to 257 */
    if (algo == LLZ_FIR_ALGO_AUTO) algo = (flt_len > 32 && flt_len <= 257) ? LLZ_FIR_ALGO_OVERLAP_SAVE : LLZ_FIR_ALGO_TIME;
    if (algo != LLZ_FIR_ALGO_TIME && algo != LLZ_FIR_ALGO_OVERLAP_SAVE) {
        llzs_set_error("llz_fir_bank_mc_init: algo %d is not built for a bank; accepted: LLZ_FIR_ALGO_AUTO (0), LLZ_FIR_ALGO_TIME "
                       "(1), LLZ_FIR_ALGO_OVERLAP_SAVE (2, 1..257 taps); a partitioned bank (1..%d taps) comes from "
                       "llz_fir_pbank_mc_init", algo, LLZS_FIR_PART_MAX_TAPS);
        return LLZ_BAD_HANDLE;
    }
    if (algo == LLZ_FIR_ALGO_OVERLAP_SAVE && flt_len > 257) {
        llzs_set_error("llz_fir_bank_mc_init: the 1024-point overlap-save takes 1..257 taps, not %d (LLZ_FIR_ALGO_TIME does)",
                       flt_len);
        return LLZ_BAD_HANDLE;
    }
    firm_t *f = (firm_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIRB;
    f->who = "llz_fir_bank_mc";
    f->device = llzs_device_get();
    f->channels = channels; f->frame_len = frame_len; f->flt_len = flt_len; f->algo = algo;

    const int tpad = (flt_len + 15) & ~15;
    const size_t hist_bytes = sizeof(float) * (size_t)channels * (size_t)(flt_len > 1 ? flt_len - 1 : 1);
    int rc = LLZ_OK;
    f->d_taps = (float *)llzs_malloc(sizeof(float) * (size_t)channels * (size_t)tpad);
    f->d_hist[0] = (float *)llzs_malloc(hist_bytes);
    f->d_hist[1] = (float *)llzs_malloc(hist_bytes);
    f->d_zero = (float *)llzs_malloc(hist_bytes);
    if (!f->d_taps || !f->d_hist[0] || !f->d_hist[1] || !f->d_zero) rc = LLZ_ERR_NOMEM;
    if (rc == LLZ_OK && algo == LLZ_FIR_ALGO_OVERLAP_SAVE) {
        f->d_hbank = (float *)llzs_malloc(sizeof(float) * 2 * (size_t)channels * LLZS_BANK_PITCH);
        f->ols.twid = (float *)llzs_malloc(sizeof(float) * 2 * 1024);
        double *cs = (double *)malloc(sizeof(double) * 2 * FIRB_N);
        float *tw = (float *)malloc(sizeof(float) * 2 * 1024);
        if (!f->d_hbank || !f->ols.twid || !cs || !tw) rc = LLZ_ERR_NOMEM;
        if (rc == LLZ_OK) {
            llz_host_cs_table(cs, FIRB_N);
            for (int a = 0; a < 32; a++)
                for (int b = 0; b < 32; b++) firm_w(&tw[2 * (a * 32 + b)], cs, (a * b) % FIRB_N);
            rc = llzs_h2d_table(f->ols.twid, tw, sizeof(float) * 2 * 1024);
        }
        free(cs); free(tw);
    }
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[0], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[1], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_zero, 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = firb_load_rows(f, 0, channels, taps, 1);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        firm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_bank_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len, int algo)
{
    if (!taps || flt_len < 1 || channels < 1 || channels > 65535) {
        llzs_set_error("llz_fir_bank_mc_init_f64taps: channels %d flt_len %d%s", channels, flt_len, taps ? "" : ", no taps");
        return LLZ_BAD_HANDLE;
    }
    float *t = llz_host_taps_f32("llz_fir_bank_mc_init_f64taps", taps, (size_t)channels * (size_t)flt_len);
    if (!t) return LLZ_BAD_HANDLE;
    unsigned long h = llz_fir_bank_mc_init(channels, frame_len, t, flt_len, algo);
    free(t);
    return h;
}

void llz_fir_bank_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB)) {
        firm_t *f = (firm_t *)handle;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        firm_destroy(f);
        llzs_device_leave(prev);
    }
}

int llz_fir_bank_mc(unsigned long handle, const float *in, float *out, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) || !in || !out) {
        llzs_set_error("llz_fir_bank_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = firm_process(f, in, out, frame_len);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_bank_mc_flush(unsigned long handle, float *out)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) || !out) {
        llzs_set_error("llz_fir_bank_mc_flush: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = firm_flush(f, out);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_bank_mc_set_taps(unsigned long handle, int first, int count, const float *taps)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) || !taps) {
        llzs_set_error("llz_fir_bank_mc_set_taps: bad handle or NULL taps");
        return LLZ_ERR_ARG;
    }
    firm_t *f = (firm_t *)handle;
    if (first < 0 || count < 1 || first >= f->channels || count > f->channels - first) {
        llzs_set_error("llz_fir_bank_mc_set_taps: channels [%d, %d + %d) outside the bank's [0, %d)", first, first, count,
                       f->channels);
        return LLZ_ERR_ARG;
    }
    const int prev = llzs_device_enter(f->device);
    /* on the handle's stream, behind the calls already issued */
    const int rc = f->algo == LLZ_FIR_ALGO_PARTITIONED
        ? llz_host_load_spectra("llz_fir_bank_mc_set_taps", f->d_hpart + (size_t)first * firm_part_row(f), firm_part_row(f), count,
                                taps, f->flt_len, f->part_n, 0, 0, f->stream)
        : firb_load_rows(f, first, count, taps, 0);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_bank_mc_flt_len(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) ? ((firm_t *)handle)->flt_len : LLZ_ERR_ARG;
}

int llz_fir_bank_mc_algo(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) ? ((firm_t *)handle)->algo : LLZ_ERR_ARG;
}

int llz_fir_bank_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB)) return LLZ_ERR_ARG;
    ((firm_t *)handle)->stream = stream;
    return LLZ_OK;
}

/* =====================================================================================================
 * Part 4: the partitioned bank -- a bank handle (LLZ_TAG_FIRB) of LLZ_FIR_ALGO_PARTITIONED: part 2's partitioned form with
 * the spectra of every channel's own taps ([channels][P][N], k_fir_part_mac<true>).  No time-domain tap table: the flush
 * runs through the partitioned launcher.  Every other call is part 3's.
 * ===================================================================================================== */

unsigned long llz_fir_pbank_mc_init(int channels, int frame_len, const float *taps, int flt_len)
{
    if (channels < 1 || channels > 65535 || frame_len < 1 || !taps) {
        llzs_set_error("llz_fir_pbank_mc_init: channels %d (1..65535) frame_len %d%s", channels, frame_len, taps ? "" : ", no taps");
        return LLZ_BAD_HANDLE;
    }
    if (flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("llz_fir_pbank_mc_init: the partitioned overlap-save takes 1..%d taps, not %d", LLZS_FIR_PART_MAX_TAPS,
                       flt_len);
        return LLZ_BAD_HANDLE;
    }
    firm_t *f = (firm_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIRB;
    f->who = "llz_fir_bank_mc";
    f->device = llzs_device_get();
    f->channels = channels; f->frame_len = frame_len; f->flt_len = flt_len; f->algo = LLZ_FIR_ALGO_PARTITIONED;

    const size_t hist_bytes = sizeof(float) * (size_t)channels * (size_t)(flt_len > 1 ? flt_len - 1 : 1);
    int rc = firm_part_size(f, "llz_fir_pbank_mc_init");          /* a scratch cap too small is refused before any allocation */
    if (rc == LLZ_OK) {
        f->d_hist[0] = (float *)llzs_malloc(hist_bytes);
        f->d_hist[1] = (float *)llzs_malloc(hist_bytes);
        f->d_zero = (float *)llzs_malloc(hist_bytes);
        if (!f->d_hist[0] || !f->d_hist[1] || !f->d_zero) rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[0], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_hist[1], 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_zero, 0, hist_bytes, NULL);
    if (rc == LLZ_OK) rc = firm_build_part(f, taps, channels, "llz_fir_pbank_mc_init");
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        firm_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_pbank_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len)
{
    if (!taps || channels < 1 || channels > 65535 || flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("llz_fir_pbank_mc_init_f64taps: channels %d (1..65535), flt_len %d (1..%d)%s", channels, flt_len,
                       LLZS_FIR_PART_MAX_TAPS, taps ? "" : ", no taps");
        return LLZ_BAD_HANDLE;
    }
    float *t = llz_host_taps_f32("llz_fir_pbank_mc_init_f64taps", taps, (size_t)channels * (size_t)flt_len);
    if (!t) return LLZ_BAD_HANDLE;
    unsigned long h = llz_fir_pbank_mc_init(channels, frame_len, t, flt_len);
    free(t);
    return h;
}

int llz_fir_pbank_mc_plan(unsigned long handle, int n, int out[4])
{
    if (!LLZ_HANDLE_OK(handle, firm_t, LLZ_TAG_FIRB) || ((firm_t *)handle)->algo != LLZ_FIR_ALGO_PARTITIONED || n < 1 || !out) {
        llzs_set_error("llz_fir_pbank_mc_plan: not a handle of llz_fir_pbank_mc_init, n %d < 1 or no out", n);
        return LLZ_ERR_ARG;
    }
    const firm_t *f = (const firm_t *)handle;
    return llzs_fir_part_plan(f->part_n, f->flt_len, n, f->channels, firm_part_avail(f), out);
}
