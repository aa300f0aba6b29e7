/* Every init and every call of the transform and analysis host layer (llz_fft_host.c, llz_mdct_host.c, llz_mdct_fixed_host.c,
 * llz_asmodel_host.c, llz_corr_host.c, llz_lpc_host.c, llz_lpc_filter_host.c, llz_spectral_host.c, llz_pcm_host.c) over the tracing
 * shim stub that tests/test_host_calls_host.py generates, under AddressSanitizer + UBSan.  Only the public headers are used (and
 * the stub's own stub_* functions), so the same file builds against another commit's host sources.
 *
 * A scenario is one handle's life, or one one-shot call: init, the calls, uninit.  Its buffers are host memory (mode 0), "device"
 * memory (mode 1: llz_hip_malloc of the stub) or, for the handles whose kernels take rows on a 16-byte boundary, device memory 4
 * bytes off (mode 2).  Per scenario one line goes to stdout, `scenario <name> lines <n> fnv <hash of the trace> tables <hash of the
 * uploaded tables' sizes and bytes>`, and for a handle one more in front of it, `<name>.init`, for the init alone.  The refusals
 * of overlapping device pairs are checked here: the message, and that no line but llzs_device_* was written.  Then every init and
 * every one-shot call is repeated with its k-th device allocation failing, k = 0 .. the number it makes: each must be refused and
 * leave no device allocation behind.
 *   host_calls                   all scenarios, then the fault injection
 *   host_calls --trace [name]    the full trace of every scenario, or of one */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "llz_fft.h"
#include "llz_fft_fixed.h"
#include "llz_corr.h"
#include "llz_asmodel.h"
#include "llz_mdct.h"
#include "llz_mdct_fixed.h"
#include "llz_levinson.h"
#include "llz_lpc.h"
#include "llz_spectral.h"
#include "llz_pcm.h"

void stub_begin(int print);
void stub_cut(int *lines, unsigned long long *hash, unsigned long long *tables);
int stub_work(void);
int stub_mallocs(void);
int stub_live(void);
int stub_bad_frees(void);
void stub_fail_malloc(int k);
void *stub_host(size_t n);
void stub_host_free(void *p);

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

/* ---- a scenario's buffers ---- */
enum { HOST = 0, DEV = 1, DEV4 = 2, MIXED = 3 };       /* MIXED (llz_autocorr_mc): the input on the device, the output not */
static struct { void *base; int dev; } g_buf[64];
static int g_nbuf;
static void *g_stream;          /* the stream the one-shot calls and set_stream get: non-NULL in the device scenarios */

static void *buf(int mode, size_t bytes)
{
    void *p = mode == HOST ? stub_host(bytes) : llz_hip_malloc(bytes + 16);
    g_buf[g_nbuf].base = p; g_buf[g_nbuf++].dev = mode != HOST;
    return mode == DEV4 ? (char *)p + 4 : p;
}

static void free_bufs(void)
{
    while (g_nbuf > 0) {
        g_nbuf--;
        if (g_buf[g_nbuf].dev) llz_hip_free(g_buf[g_nbuf].base); else stub_host_free(g_buf[g_nbuf].base);
    }
}

/* the refusal of an overlapping device pair: code, message, and nothing staged or launched */
static int g_work0;
static void refusal_begin(void) { g_work0 = stub_work(); }
static int refused(long rc, const char *who, const char *out, const char *in)
{
    char want[160];
    snprintf(want, sizeof want, "%s: %s may not overlap %s (device memory)", who, out, in);
    if (rc == LLZ_ERR_ARG && !strcmp(want, llz_hip_last_error()) && stub_work() == g_work0) return 1;
    fprintf(stderr, "driver: rc %ld, message '%s' instead of '%s', %d lines\n", rc, llz_hip_last_error(), want, stub_work() - g_work0);
    return 0;
}

/* ---- the handles ---- */
enum { K_FFT1, K_FFTB, K_FFTX, K_MDCT1, K_MDCB, K_MDCX, K_ASMA, K_ASMS, K_AMDA, K_AMDS, K_STFT, K_AMDM, K_ACF1, K_ACFM, K_XCFM,
       K_LPC1, K_LPCF, K_CSD };
static const int g_pairs[4] = {0, 1, 1, 1};

static unsigned long mk(int kind, int arg)
{
    switch (kind) {
    case K_FFT1: return llz_fft_init(arg);
    case K_FFTB: return llz_fft_batch_init(arg);
    case K_FFTX: return llz_fft_fixed_init(arg);
    case K_MDCT1: return llz_mdct_init(arg, 64);
    case K_MDCB: return llz_mdct_batch_init(arg);
    case K_MDCX: return llz_mdct_fixed_init(arg, 64);
    case K_ASMA: return llz_analysis_fft_init(arg >= 4096 ? LLZ_OVERLAP_LOW : LLZ_OVERLAP_HIGH, arg, arg >= 4096 ? HAMMING : KAISER);
    case K_ASMS: return llz_synthesis_fft_init(LLZ_OVERLAP_LOW, arg, BLACKMAN);
    case K_AMDA: return llz_analysis_mdct_init(arg, MDCT_SINE);
    case K_AMDS: return llz_synthesis_mdct_init(arg, MDCT_KBD);
    case K_STFT: return llz_stft_mc_init(arg >= 4096 ? 1 : 2, LLZ_OVERLAP_LOW, arg, HAMMING);
    case K_AMDM: return llz_mdct_frames_mc_init(2, arg, arg == 128 ? MDCT_SINE : MDCT_KBD);
    case K_ACF1: return llz_autocorr_fast_init(arg);
    case K_ACFM: return llz_autocorr_fast_mc_init(3, arg);
    case K_XCFM: return llz_crosscorr_fast_mc_init(3, arg);
    case K_LPC1: return llz_lpc_init(arg);
    case K_LPCF: return llz_lpc_filter_mc_init(2, 32, arg);
    default: return llz_csd_mc_init(2, 2, g_pairs, 64, arg, arg == 64 ? BLACKMAN : HAMMING);
    }
}

static void rm(int kind, unsigned long h)
{
    switch (kind) {
    case K_FFT1: llz_fft_uninit(h); break;
    case K_FFTB: llz_fft_batch_uninit(h); break;
    case K_FFTX: llz_fft_fixed_uninit(h); break;
    case K_MDCT1: llz_mdct_uninit(h); break;
    case K_MDCB: llz_mdct_batch_uninit(h); break;
    case K_MDCX: llz_mdct_fixed_uninit(h); break;
    case K_ASMA: llz_analysis_fft_uninit(h); break;
    case K_ASMS: llz_synthesis_fft_uninit(h); break;
    case K_AMDA: llz_analysis_mdct_uninit(h); break;
    case K_AMDS: llz_synthesis_mdct_uninit(h); break;
    case K_STFT: llz_stft_mc_uninit(h); break;
    case K_AMDM: llz_mdct_frames_mc_uninit(h); break;
    case K_ACF1: llz_autocorr_fast_uninit(h); break;
    case K_ACFM: llz_autocorr_fast_mc_uninit(h); break;
    case K_XCFM: llz_crosscorr_fast_mc_uninit(h); break;
    case K_LPC1: llz_lpc_uninit(h); break;
    case K_LPCF: llz_lpc_filter_mc_uninit(h); break;
    default: llz_csd_mc_uninit(h); break;
    }
}

static int set_stream(int kind, unsigned long h)
{
    switch (kind) {
    case K_FFTB: return llz_fft_batch_set_stream(h, g_stream);
    case K_FFTX: return llz_fft_fixed_set_stream(h, g_stream);
    case K_MDCB: return llz_mdct_batch_set_stream(h, g_stream);
    case K_MDCX: return llz_mdct_fixed_set_stream(h, g_stream);
    case K_STFT: return llz_stft_mc_set_stream(h, g_stream);
    case K_AMDM: return llz_mdct_frames_mc_set_stream(h, g_stream);
    case K_ACFM: return llz_autocorr_fast_mc_set_stream(h, g_stream);
    case K_XCFM: return llz_crosscorr_fast_mc_set_stream(h, g_stream);
    case K_LPCF: return llz_lpc_filter_mc_set_stream(h, g_stream);
    case K_CSD: return llz_csd_mc_set_stream(h, g_stream);
    default: return LLZ_OK;                                          /* no stream: the reference's symbols */
    }
}

/* ---- the calls of a handle: mode as above; the reference's symbols take host memory only ---- */
static int use(int kind, int arg, unsigned long h, int m)
{
    const size_t fb = sizeof(float), db = sizeof(double), ib = sizeof(int);
    switch (kind) {
    case K_FFT1: { double *d = buf(HOST, db * 2 * arg); llz_fft(h, d); llz_ifft(h, d); return 0; }
    case K_FFTB: { float *d = buf(m, fb * 2 * arg * 2); CHECK(llz_fft_batch(h, d, 2) == LLZ_OK); CHECK(llz_ifft_batch(h, d, 2) == LLZ_OK); return 0; }
    case K_FFTX: {
        int *d = buf(m, ib * 2 * arg * 2);
        CHECK(llz_fft_fixed_batch(h, d, 2) == LLZ_OK); CHECK(llz_ifft_fixed_batch(h, d, 2) == LLZ_OK);
        if (m == HOST) { llz_fft_fixed(h, d); llz_ifft_fixed(h, d); }
        return 0;
    }
    case K_MDCT1: { double *x = buf(HOST, db * 64), *X = buf(HOST, db * 32); llz_mdct(h, x, X); llz_imdct(h, X, x); return 0; }
    case K_MDCB: {
        float *x = buf(m, fb * 3 * arg), *X = buf(m, fb * 3 * arg / 2);
        CHECK(llz_mdct_batch(h, x, X, 3) == 3); CHECK(llz_imdct_batch(h, X, x, 3) == 3);
        if (m == DEV) { refusal_begin(); CHECK(refused(llz_mdct_batch(h, x, x + 8, 3), "llz_mdct_batch", "out", "in")); }
        return 0;
    }
    case K_MDCX: {
        int *x = buf(m, ib * 2 * 64), *X = buf(m, ib * 2 * 32);
        CHECK(llz_mdct_fixed_batch(h, x, X, 2) == 2); CHECK(llz_imdct_fixed_batch(h, X, x, 2) == 2);
        if (m == HOST) { llz_mdct_fixed(h, x, X); llz_imdct_fixed(h, X, x); }
        if (m == DEV) { refusal_begin(); CHECK(refused(llz_imdct_fixed_batch(h, x, x + 8, 2), "llz_imdct_fixed_batch", "out", "in")); }
        return 0;
    }
    case K_ASMA: case K_ASMS: {
        const int bins = (kind == K_ASMA && arg < 4096 ? 2 * arg : arg) + 1;
        double *x = buf(HOST, db * arg), *re = buf(HOST, db * bins), *im = buf(HOST, db * bins);
        for (int i = 0; i < 2; i++) { if (kind == K_ASMA) llz_analysis_fft(h, x, re, im); else llz_synthesis_fft(h, re, im, x); }
        return 0;
    }
    case K_AMDA: case K_AMDS: {
        double *x = buf(HOST, db * arg), *X = buf(HOST, db * arg);
        for (int i = 0; i < 2; i++) { if (kind == K_AMDA) llz_analysis_mdct(h, x, X); else llz_synthesis_mdct(h, X, x); }
        return 0;
    }
    case K_STFT: {
        const int ch = arg >= 4096 ? 1 : 2, frames = arg >= 4096 ? 2 : 3, bins = llz_stft_mc_bins(h);
        CHECK(bins == arg + 1);
        float *x = buf(m, fb * ch * frames * arg), *re = buf(m, fb * ch * frames * bins), *im = buf(m, fb * ch * frames * bins);
        for (int i = 0; i < 2; i++) {
            CHECK(llz_stft_mc_analysis(h, x, re, im, frames) == frames);
            CHECK(llz_stft_mc_synthesis(h, re, im, x, frames) == frames);
        }
        if (m == DEV) {
            refusal_begin(); CHECK(refused(llz_stft_mc_analysis(h, re, re + 4, im, 1), "llz_stft_mc_analysis", "re", "x"));
            refusal_begin(); CHECK(refused(llz_stft_mc_analysis(h, im, re, im + 4, 1), "llz_stft_mc_analysis", "im", "x"));
            refusal_begin(); CHECK(refused(llz_stft_mc_synthesis(h, re, im, im + 4, 1), "llz_stft_mc_synthesis", "x", "im"));
        }
        return 0;
    }
    case K_AMDM: {
        float *x = buf(m, fb * 2 * 2 * arg), *X = buf(m, fb * 2 * 2 * arg);
        for (int i = 0; i < 2; i++) {
            CHECK(llz_mdct_frames_mc_analysis(h, x, X, 2) == 2);
            CHECK(llz_mdct_frames_mc_synthesis(h, X, x, 2) == 2);
        }
        if (m == DEV) { refusal_begin(); CHECK(refused(llz_mdct_frames_mc_synthesis(h, x, x + 4, 1), "llz_mdct_frames_mc_synthesis", "out", "in")); }
        return 0;
    }
    case K_ACF1: { double *x = buf(HOST, db * arg), *r = buf(HOST, db * 6); llz_autocorr_fast(h, x, arg, 5, r); return 0; }
    case K_ACFM: {
        float *x = buf(m, fb * 3 * arg), *r = buf(m, fb * 3 * 6);
        CHECK(llz_autocorr_fast_mc(h, x, r, 5) == LLZ_OK);
        if (m == DEV) { refusal_begin(); CHECK(refused(llz_autocorr_fast_mc(h, x, x + 4, 5), "llz_autocorr_fast_mc", "r", "x")); }
        return 0;
    }
    case K_XCFM: {
        float *x = buf(m, fb * 3 * arg), *y = buf(m, fb * 3 * arg), *r = buf(m, fb * 3 * 11);
        CHECK(llz_crosscorr_fast_mc(h, x, y, r, 5, 0) == LLZ_OK);
        CHECK(llz_crosscorr_fast_mc(h, x, y, r, 5, 1) == LLZ_OK);
        CHECK(llz_crosscorr_fast_mc(h, x, x, r, 5, 1) == LLZ_OK);
        if (m == DEV) { refusal_begin(); CHECK(refused(llz_crosscorr_fast_mc(h, x, y, y + 4, 5, 0), "llz_crosscorr_fast_mc", "r", "y")); }
        return 0;
    }
    case K_LPC1: {
        double *x = buf(HOST, db * 64), *a = buf(HOST, db * (arg + 1)), *k = buf(HOST, db * (arg + 1)), err;
        (void)llz_lpc(h, x, 64, a, k, &err); (void)llz_lpc(h, x, 48, a, k, &err);
        return 0;
    }
    case K_LPCF: {
        float *x = buf(m, fb * 2 * 2 * 32), *a = buf(m, fb * 2 * 2 * (arg + 1)), *e = buf(m, fb * 2 * 2 * 32);
        for (int i = 0; i < 2; i++) {
            CHECK(llz_lpc_residual_mc(h, x, a, e, 2) == 2);
            CHECK(llz_lpc_synth_mc(h, e, a, x, 2) == 2);
        }
        CHECK(llz_lpc_filter_mc_reset(h) == LLZ_OK);
        if (m == DEV) {
            refusal_begin(); CHECK(refused(llz_lpc_residual_mc(h, x, a, x + 4, 1), "llz_lpc_residual_mc", "e", "x"));
            refusal_begin(); CHECK(refused(llz_lpc_synth_mc(h, e, a, a + 1, 1), "llz_lpc_synth_mc", "y", "acof"));
        }
        return 0;
    }
    default: {
        float *x = buf(m, fb * 2 * 5 * arg), *o = buf(m, fb * 2 * 2 * 33);
        double *raw = buf(m, db * 4 * 2 * 33);
        int plan[4];
        CHECK(llz_csd_mc_plan(h, 5L * arg, plan) == LLZ_OK);
        for (int i = 0; i < 2; i++) CHECK(llz_csd_mc_update(h, x, 5L * arg) > 0);
        for (int what = LLZ_SPEC_PXX; what <= LLZ_SPEC_TF; what++) CHECK(llz_csd_mc_read(h, what, o) == LLZ_OK);
        CHECK(llz_csd_mc_read_raw(h, raw) == LLZ_OK);
        CHECK(llz_csd_mc_frames(h) > 0);
        CHECK(llz_csd_mc_reset(h) == LLZ_OK);
        return 0;
    }
    }
}

static void report(const char *name, const char *part)
{
    int lines;
    unsigned long long hash, tables;
    stub_cut(&lines, &hash, &tables);
    printf("scenario %s%s lines %d fnv %016llx tables %016llx\n", name, part, lines, hash, tables);
}

static int handle_scenario(const char *name, int kind, int arg, int m)
{
    unsigned long h = mk(kind, arg);
    CHECK(h != BAD);
    report(name, ".init");
    if (m != HOST) CHECK(set_stream(kind, h) == LLZ_OK);
    const int rc = use(kind, arg, h, m);
    rm(kind, h);
    return rc;
}

/* ---- the one-shot calls: arg picks the variant ---- */
enum { O_ACORR, O_XCORR, O_COF, O_LPC, O_PCM, O_REF };

static int one_shot(int what, int arg, int m, int must_pass)
{
    const size_t fb = sizeof(float);
    void *st = m == HOST ? NULL : g_stream;
    long rc = 0;
    switch (what) {
    case O_ACORR: {                                     /* arg: p (5: register form, 40: LDS form) */
        float *x = buf(m == MIXED ? DEV : m, fb * 3 * 80), *r = buf(m == MIXED ? HOST : m, fb * 3 * (arg + 1));
        rc = llz_autocorr_mc(x, r, 3, 80, arg, st);
        if (m == DEV && must_pass) { refusal_begin(); CHECK(refused(llz_autocorr_mc(x, x + 8, 3, 80, arg, st), "llz_autocorr_mc", "r", "x")); }
        break;
    }
    case O_XCORR: {                                     /* arg: bit 0 two-sided, bit 1 y == x */
        float *x = buf(m, fb * 3 * 80), *y = arg & 2 ? x : buf(m, fb * 3 * 80), *r = buf(m, fb * 3 * 11);
        rc = llz_crosscorr_mc(x, y, r, 3, 80, 5, arg & 1, st);
        if (m == DEV && must_pass && !(arg & 2)) {
            refusal_begin(); CHECK(refused(llz_crosscorr_mc(x, y, x + 8, 3, 80, 5, 0, st), "llz_crosscorr_mc", "r", "x"));
            refusal_begin(); CHECK(refused(llz_crosscorr_mc(x, y, y + 8, 3, 80, 5, 0, st), "llz_crosscorr_mc", "r", "y"));
        }
        break;
    }
    case O_COF: {                                       /* arg: 1 = b == a */
        float *a = buf(m, fb * 3 * 80), *b = arg ? a : buf(m, fb * 3 * 80), *c = buf(m, fb * 3);
        rc = llz_corr_cof_mc(a, b, c, 3, 80, st);
        if (m == DEV && must_pass && !arg) { refusal_begin(); CHECK(refused(llz_corr_cof_mc(a, b, b + 1, 3, 80, st), "llz_corr_cof_mc", "c", "b")); }
        break;
    }
    case O_LPC: {                                       /* arg: bit 0 split (p = 40), bit 1 window, bit 2 optional outputs NULL */
        const int p = arg & 1 ? 40 : 4, n = 64, opt = !(arg & 4);
        float *x = buf(m, fb * 3 * n), *w = arg & 2 ? buf(m, fb * n) : NULL, *a = buf(m, fb * 3 * (p + 1));
        float *k = opt ? buf(m, fb * 3 * p) : NULL, *e = opt ? buf(m, fb * 3) : NULL, *g = opt ? buf(m, fb * 3) : NULL;
        float *r = opt ? buf(m, fb * 3 * (p + 1)) : NULL;
        rc = llz_lpc_mc(x, w, a, k, e, g, r, 3, n, p, st);
        if (m == DEV && must_pass && opt) {
            refusal_begin(); CHECK(refused(llz_lpc_mc(x, w, x + 4, k, e, g, r, 3, n, p, st), "llz_lpc_mc", "acof", "x"));
            refusal_begin(); CHECK(refused(llz_lpc_mc(x, w, a, k, e, g, x + 4, 3, n, p, st), "llz_lpc_mc", "r", "x"));
        }
        break;
    }
    case O_PCM: {                                       /* arg: 1 = deinterleave */
        short *s = buf(m, sizeof(short) * 3 * 17);
        float *f = buf(m, fb * 3 * 17);
        rc = arg ? llz_pcm_deinterleave_i16_f32(s, f, 3, 17, 1.0f / 32768, st) : llz_pcm_interleave_f32_i16(f, s, 3, 17, 32768.0f, st);
        if (m == DEV && must_pass) {
            refusal_begin();
            if (arg) CHECK(refused(llz_pcm_deinterleave_i16_f32(s, (float *)s + 1, 1, 8, 1.0f, st), "llz_pcm_deinterleave_i16_f32", "out", "in"));
            else CHECK(refused(llz_pcm_interleave_f32_i16(f, (short *)f + 2, 1, 8, 1.0f, st), "llz_pcm_interleave_f32_i16", "out", "in"));
        }
        break;
    }
    default: {                                          /* the reference's symbols of llz_corr.h: host memory, void */
        double *x = buf(HOST, sizeof(double) * 30), *y = buf(HOST, sizeof(double) * 30), *r = buf(HOST, sizeof(double) * 6);
        llz_autocorr(x, 30, 5, r);
        llz_crosscorr(x, y, 30, 5, r);
        (void)llz_corr_cof(x, y, 30);
        break;
    }
    }
    if (must_pass) CHECK(rc == LLZ_OK);
    return rc < 0 ? -1 : 0;
}

/* ---- the list ---- */
typedef struct { const char *name; int handle, what, arg, mode; } scenario_t;
#define H3(n, k, a) {n "_host", 1, k, a, HOST}, {n "_dev", 1, k, a, DEV}, {n "_dev4", 1, k, a, DEV4}
#define H2(n, k, a) {n "_host", 1, k, a, HOST}, {n "_dev", 1, k, a, DEV}
#define H1(n, k, a) {n, 1, k, a, HOST}
#define O2(n, w, a) {n "_host", 0, w, a, HOST}, {n "_dev", 0, w, a, DEV}
static const scenario_t g_list[] = {
    H1("fft_8", K_FFT1, 8), H1("fft_4096", K_FFT1, 4096), H1("fft_8192", K_FFT1, 8192),
    H3("fft_batch_8", K_FFTB, 8), H3("fft_batch_4096", K_FFTB, 4096), H3("fft_batch_8192", K_FFTB, 8192),
    H3("fft_fixed_64", K_FFTX, 64),
    H1("mdct_origin", K_MDCT1, MDCT_ORIGIN), H1("mdct_fft", K_MDCT1, MDCT_FFT), H1("mdct_fft4", K_MDCT1, MDCT_FFT4),
    H3("mdct_batch_32", K_MDCB, 32),
    H2("mdct_fixed_origin", K_MDCX, MDCT_FIXED_ORIGIN), H2("mdct_fixed_fft", K_MDCX, MDCT_FIXED_FFT),
    H2("mdct_fixed_fft4", K_MDCX, MDCT_FIXED_FFT4),
    H1("analysis_fft_16", K_ASMA, 16), H1("analysis_fft_4096", K_ASMA, 4096), H1("synthesis_fft_16", K_ASMS, 16),
    H1("synthesis_fft_4096", K_ASMS, 4096), H1("analysis_mdct_8", K_AMDA, 8), H1("synthesis_mdct_8", K_AMDS, 8),
    H2("stft_mc_32", K_STFT, 32), H2("stft_mc_2048", K_STFT, 2048), H2("stft_mc_4096", K_STFT, 4096),
    H3("mdct_frames_mc_128", K_AMDM, 128), H3("mdct_frames_mc_256", K_AMDM, 256),
    H1("autocorr_fast_30", K_ACF1, 30), H2("autocorr_fast_mc_30", K_ACFM, 30), H2("crosscorr_fast_mc_30", K_XCFM, 30),
    H1("lpc_4", K_LPC1, 4), H2("lpc_filter_mc_4", K_LPCF, 4), H2("lpc_filter_mc_0", K_LPCF, 0),
    H2("csd_mc_hop32", K_CSD, 32), H2("csd_mc_hop64", K_CSD, 64),
    {"corr_reference", 0, O_REF, 0, HOST},
    O2("autocorr_mc_p5", O_ACORR, 5), {"autocorr_mc_p5_dev_in_host_out", 0, O_ACORR, 5, MIXED}, O2("autocorr_mc_p40", O_ACORR, 40),
    O2("crosscorr_mc", O_XCORR, 0), O2("crosscorr_mc_two_sided", O_XCORR, 1),
    {"crosscorr_mc_host_alias", 0, O_XCORR, 3, HOST}, {"crosscorr_mc_dev_alias", 0, O_XCORR, 3, DEV},
    O2("corr_cof_mc", O_COF, 0), {"corr_cof_mc_host_alias", 0, O_COF, 1, HOST}, {"corr_cof_mc_dev_alias", 0, O_COF, 1, DEV},
    O2("lpc_mc_fused", O_LPC, 0), O2("lpc_mc_split", O_LPC, 1), O2("lpc_mc_fused_win", O_LPC, 2), O2("lpc_mc_split_win", O_LPC, 3),
    O2("lpc_mc_fused_bare", O_LPC, 4), O2("lpc_mc_split_bare", O_LPC, 5), O2("lpc_mc_split_win_bare", O_LPC, 7),
    O2("pcm_deinterleave", O_PCM, 1), O2("pcm_interleave", O_PCM, 0),
};
enum { N_LIST = sizeof(g_list) / sizeof(g_list[0]) };

int main(int argc, char **argv)
{
    const int trace = argc > 1 && !strcmp(argv[1], "--trace");
    const char *only = argc > 2 ? argv[2] : NULL;
    int stream_token;
    g_stream = &stream_token;
    for (int i = 0; i < N_LIST; i++) {
        const scenario_t *s = &g_list[i];
        if (only && strcmp(only, s->name)) continue;
        if (trace) printf("==== %s\n", s->name);
        stub_begin(trace);
        const int rc = s->handle ? handle_scenario(s->name, s->what, s->arg, s->mode) : one_shot(s->what, s->arg, s->mode, 1);
        free_bufs();
        if (rc) { fprintf(stderr, "driver: scenario %s failed\n", s->name); return 1; }
        CHECK(stub_live() == 0);
        report(s->name, "");
    }
    printf("SCENARIOS_DONE\n");
    if (trace) return 0;

    /* the k-th device allocation fails: every init (once per handle form) and every one-shot call on host buffers, and the split
     * LPC on device buffers for its two scratch buffers */
    int refusals = 0, scenarios = 0, bad = 0, frees0 = stub_bad_frees();
    CHECK(frees0 == 0);
    for (int i = 0; i < N_LIST; i++) {
        const scenario_t *s = &g_list[i];
        if (s->what == O_REF && !s->handle) continue;
        if (s->handle ? (s->mode != HOST) : (s->mode != HOST && !(s->what == O_LPC && (s->arg & 1)))) continue;
        scenarios++;
        for (int k = 0; ; k++) {
            stub_begin(0);
            stub_fail_malloc(k);
            int passed;
            if (s->handle) {
                unsigned long h = mk(s->what, s->arg);
                passed = h != BAD;
                if (passed) rm(s->what, h);
            } else {
                passed = one_shot(s->what, s->arg, s->mode, 0) == 0;
                free_bufs();
            }
            const int reached = stub_mallocs() > k;
            if (stub_bad_frees() != frees0) { printf("FAULT %s k=%d: a device pointer freed twice\n", s->name, k); bad++; frees0 = stub_bad_frees(); }
            if (stub_live()) { printf("FAULT %s k=%d: %d device allocations left behind\n", s->name, k, stub_live()); bad++; }
            if (!reached) {
                if (!passed) { printf("FAULT %s: fails with no allocation refused\n", s->name); bad++; }
                break;
            }
            if (passed) { printf("FAULT %s k=%d: not refused\n", s->name, k); bad++; }
            refusals++;
        }
    }
    printf("fault injection: %d refused allocations over %d scenarios, %d faults\n", refusals, scenarios, bad);
    if (bad) return 1;
    printf("HOST_CALLS_OK\n");
    return 0;
}
