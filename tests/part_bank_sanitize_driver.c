/* The partitioned bank's host layer under AddressSanitizer + UBSan with the device shim stubbed out (the stub of
 * tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without computing), at
 * 1, 513 and 131073 taps:
 *   * llz_host_part_spectra, the one builder of the partition spectra (shared-taps handle and bank), into a buffer of exactly
 *     [P][N] complex floats, every entry of sampled bins against a direct DFT in double: entry i of row p is bin bitrev(i) of
 *     DFT_N(taps[p B .. p B + B), zero-padded) / N, rounded to float once;
 *   * llz_fir_pbank_mc_init / _init_f64taps / _plan and the bank calls on such a handle: row chunks of the table upload,
 *     set_taps on a sub-range, host-buffer staging, flush, refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "host/llz_host.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static unsigned g_seed = 12345u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

static int own_nfft(int T)
{
    int n = 1024;
    while (n < 8192 && T > 4 * (n / 2)) n *= 2;
    return n;
}

static int bitrev(int i, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

static int pin_builder(int T)
{
    const int N = own_nfft(T), B = N / 2, P = (T + B - 1) / B;
    int bits = 0;
    while ((1 << bits) < N) bits++;
    float *taps = malloc(sizeof(float) * (size_t)T);
    float *H = malloc(sizeof(float) * 2 * (size_t)P * (size_t)N);          /* exactly [P][N] complex */
    double *cs = malloc(sizeof(double) * 2 * (size_t)N), *z = malloc(sizeof(double) * 2 * (size_t)N);
    CHECK(taps && H && cs && z);
    for (int i = 0; i < T; i++) taps[i] = rnd();
    for (int i = 0; i < N; i++) {
        const double ang = 2.0 * M_PI * (double)i / (double)N;
        cs[2 * i] = (i == N / 4 || i == 3 * N / 4) ? 0.0 : cos(ang);
        cs[2 * i + 1] = (i == 0 || i == N / 2) ? 0.0 : sin(ang);
    }
    llz_host_part_spectra(H, taps, T, N, cs, z);
    double worst = 0.0;
    for (int p = 0; p < P; p++)
        for (int s = 0; s < 48; s++) {
            /* entries 0, 1, N - 1 and a spread of others */
            const int i = s == 0 ? 0 : s == 1 ? 1 : s == 2 ? N - 1 : (int)(((long)s * 2654435761u + (unsigned)p * 97u) % (unsigned)N);
            const int k = bitrev(i, bits);
            double re = 0.0, im = 0.0, mag = 0.0;
            for (int t = 0; t < B && (long)p * B + t < T; t++) {
                const int m = (int)(((long)k * t) % N);
                const double h = (double)taps[(long)p * B + t];
                re += h * cs[2 * m];
                im -= h * cs[2 * m + 1];
                mag += fabs(h);
            }
            re /= N; im /= N; mag /= N;
            /* one float rounding of the value (2^-24 relative) and the double transform's own error (far below 1e-12 mag) */
            const double lim_re = ldexp(fabs(re), -24) + 1e-12 * mag + 1e-45, lim_im = ldexp(fabs(im), -24) + 1e-12 * mag + 1e-45;
            const double er = fabs((double)H[2 * ((size_t)p * N + i)] - re), ei = fabs((double)H[2 * ((size_t)p * N + i) + 1] - im);
            if (er / lim_re > worst) worst = er / lim_re;
            if (ei / lim_im > worst) worst = ei / lim_im;
            if (er > lim_re || ei > lim_im) {
                fprintf(stderr, "driver: T=%d partition %d entry %d (bin %d): got %.9g %+.9gj, direct DFT %.17g %+.17gj\n", T, p, i, k,
                        (double)H[2 * ((size_t)p * N + i)], (double)H[2 * ((size_t)p * N + i) + 1], re, im);
                return 1;
            }
        }
    printf("spectrum builder T=%d N=%d P=%d: worst ratio to one float rounding %.3g\n", T, N, P, worst);
    free(taps); free(H); free(cs); free(z);
    return 0;
}

static int drive_handle(int T)
{
    enum { CH = 3, FRAME = 1000 };
    const int keep = T - 1, span = keep > FRAME ? keep : FRAME;
    float *taps = malloc(sizeof(float) * CH * (size_t)T);
    double *taps64 = malloc(sizeof(double) * CH * (size_t)T);
    float *x = calloc((size_t)CH * FRAME, sizeof(float)), *y = calloc((size_t)CH * (size_t)span, sizeof(float));
    int plan[4] = {0, 0, 0, 0};
    CHECK(taps && taps64 && x && y);
    for (size_t i = 0; i < CH * (size_t)T; i++) taps64[i] = taps[i] = rnd();
    unsigned long h = llz_fir_pbank_mc_init(CH, FRAME, taps, T);
    CHECK(h != BAD);
    CHECK(llz_fir_bank_mc_algo(h) == LLZ_FIR_ALGO_PARTITIONED && llz_fir_bank_mc_flt_len(h) == T);
    CHECK(llz_fir_filter_mc_algo(h) < 0);                          /* a bank handle, not a shared-taps one */
    CHECK(llz_fir_pbank_mc_plan(h, FRAME, plan) == 0);
    CHECK(llz_fir_pbank_mc_plan(h, 0, plan) < 0 && llz_fir_pbank_mc_plan(h, FRAME, NULL) < 0);
    CHECK(llz_fir_filter_mc_partition_plan(h, FRAME, plan) < 0);
    CHECK(llz_fir_bank_mc(h, x, y, FRAME) == FRAME);
    CHECK(llz_fir_bank_mc(h, x, y, FRAME - 1) < 0);
    CHECK(llz_fir_bank_mc_set_taps(h, 1, 2, taps) == 0);           /* rows 1 and 2: the last rows of the table */
    CHECK(llz_fir_bank_mc_set_taps(h, 0, CH, taps) == 0);
    CHECK(llz_fir_bank_mc_set_taps(h, 2, 2, taps) < 0 && llz_fir_bank_mc_set_taps(h, -1, 1, taps) < 0);
    CHECK(llz_fir_bank_mc_set_taps(h, 0, 0, taps) < 0 && llz_fir_bank_mc_set_taps(h, 0, 1, NULL) < 0);
    CHECK(llz_fir_bank_mc(h, x, y, FRAME) == FRAME);
    CHECK(llz_fir_bank_mc_flush(h, y) == keep);
    CHECK(llz_fir_bank_mc_set_stream(h, NULL) == 0);
    llz_fir_bank_mc_uninit(h);
    h = llz_fir_pbank_mc_init_f64taps(CH, FRAME, taps64, T);
    CHECK(h != BAD);
    CHECK(llz_fir_bank_mc_flush(h, y) == keep);
    llz_fir_bank_mc_uninit(h);
    free(taps); free(taps64); free(x); free(y);
    return 0;
}

int main(void)
{
    const int T[3] = {1, 513, 131073};
    for (int i = 0; i < 3; i++) {
        if (pin_builder(T[i])) return 1;
        if (drive_handle(T[i])) return 1;
    }
    {   /* more rows than one staging chunk holds (8 MiB: 3 rows at 131073 taps, so 7 rows go in chunks of 3, 3 and 1) */
        const int Tl = 131073, ch = 7;
        float *taps = calloc((size_t)ch * Tl, sizeof(float));
        CHECK(taps);
        unsigned long h = llz_fir_pbank_mc_init(ch, 64, taps, Tl);
        CHECK(h != BAD);
        CHECK(llz_fir_bank_mc_set_taps(h, 2, 5, taps) == 0);
        llz_fir_bank_mc_uninit(h);
        /* refusals: each leaves a message of its own */
        CHECK(llz_fir_pbank_mc_init(0, 64, taps, 63) == BAD && strstr(llz_hip_last_error(), "llz_fir_pbank_mc_init"));
        CHECK(llz_fir_pbank_mc_init(65536, 64, taps, 63) == BAD);
        CHECK(llz_fir_pbank_mc_init(2, 0, taps, 63) == BAD);
        CHECK(llz_fir_pbank_mc_init(2, 64, NULL, 63) == BAD);
        CHECK(llz_fir_pbank_mc_init(2, 64, taps, 0) == BAD && strstr(llz_hip_last_error(), "1..131073"));
        CHECK(llz_fir_pbank_mc_init(2, 64, taps, Tl + 1) == BAD && strstr(llz_hip_last_error(), "1..131073"));
        CHECK(llz_fir_pbank_mc_init_f64taps(2, 64, NULL, 63) == BAD);
        CHECK(llz_fir_pbank_mc_init_f64taps(2, 64, (const double *)taps, Tl + 1) == BAD && strstr(llz_hip_last_error(), "1..131073"));
        /* the bank's own init keeps refusing algo 7, and its handles are refused by the plan query */
        CHECK(llz_fir_bank_mc_init(2, 64, taps, 63, LLZ_FIR_ALGO_PARTITIONED) == BAD);
        h = llz_fir_bank_mc_init(2, 64, taps, 63, LLZ_FIR_ALGO_TIME);
        CHECK(h != BAD);
        int plan[4];
        CHECK(llz_fir_pbank_mc_plan(h, 64, plan) < 0);
        llz_fir_bank_mc_uninit(h);
        h = llz_fir_filter_mc_init(2, 64, taps, 1300, LLZ_FIR_ALGO_PARTITIONED);
        CHECK(h != BAD);
        CHECK(llz_fir_pbank_mc_plan(h, 64, plan) < 0);
        llz_fir_filter_mc_uninit(h);
        CHECK(llz_fir_pbank_mc_plan(0, 64, plan) < 0 && llz_fir_pbank_mc_plan(BAD, 64, plan) < 0);
        free(taps);
    }
    printf("PART_BANK_SANITIZE_OK\n");
    return 0;
}
