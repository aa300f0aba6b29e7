/* The stream convolver's host layer (llz_fir_stream_host.c) under AddressSanitizer + UBSan with the device shim stubbed out (the
 * stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without computing),
 * at (block, taps) = (64, 1), (64, 65), (512, 513), (128, 131073):
 *   * llz_host_stream_spectra, the one builder of the tap spectra (shared and per-channel handles), into a buffer of exactly
 *     [P][block] complex floats; sampled entries of every partition, packed bin 0 always among them, against a direct real DFT
 *     in double: entry i > 0 of row p is bin bitrev(i) of DFT_N(taps[p B .. p B + B), zero-padded) / (2 N), N = 2 B, entry 0 is
 *     (bin 0, bin B) of it, both real; each rounded to float once;
 *   * llz_fir_stream_mc_init / _init_f64taps and every call on such handles: row chunks of the table upload, set_taps ranges,
 *     host-buffer staging, flush, reset, plan, refusals. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "host/llz_host.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static unsigned g_seed = 24680u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

static int bitrev(int i, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

/* |got - want| against one float rounding of the value and the double transform's own error */
static int within(double got, double want, double mag, double *worst)
{
    const double lim = ldexp(fabs(want), -24) + 1e-12 * mag + 1e-45, err = fabs(got - want);
    if (err / lim > *worst) *worst = err / lim;
    return err <= lim;
}

static int pin_builder(int B, int T)
{
    const int N = 2 * B, P = (T + B - 1) / B;
    int bits = 0;
    while ((1 << bits) < B) bits++;
    float *taps = malloc(sizeof(float) * (size_t)T);
    float *H = malloc(sizeof(float) * 2 * (size_t)P * (size_t)B);          /* exactly [P][B] complex */
    double *cs = malloc(sizeof(double) * 2 * (size_t)N), *z = malloc(sizeof(double) * 2 * (size_t)N);
    CHECK(taps && H && cs && z);
    for (int i = 0; i < T; i++) taps[i] = rnd();
    for (int i = 0; i < N; i++) {
        const double ang = 2.0 * M_PI * (double)i / (double)N;
        cs[2 * i] = (i == N / 4 || i == 3 * N / 4) ? 0.0 : cos(ang);
        cs[2 * i + 1] = (i == 0 || i == N / 2) ? 0.0 : sin(ang);
    }
    llz_host_stream_spectra(H, taps, T, B, cs, z);
    double worst = 0.0;
    for (int p = 0; p < P; p++)
        for (int s = 0; s < 24; s++) {
            /* entries 0 (the packed bin), 1, B - 1 and a spread of others */
            const int i = s == 0 ? 0 : s == 1 ? 1 : s == 2 ? B - 1 : (int)(((long)s * 2654435761u + (unsigned)p * 97u) % (unsigned)B);
            const int k = bitrev(i, bits);
            double re = 0.0, im = 0.0, ny = 0.0, mag = 0.0;
            for (int t = 0; t < B && (long)p * B + t < T; t++) {
                const int m = (int)(((long)k * t) % N);
                const double h = (double)taps[(long)p * B + t];
                re += h * cs[2 * m];
                im -= h * cs[2 * m + 1];
                ny += (t & 1) ? -h : h;                            /* bin B: W_N^(B t) = (-1)^t */
                mag += fabs(h);
            }
            re /= 2.0 * N; im /= 2.0 * N; ny /= 2.0 * N; mag /= 2.0 * N;
            const double gr = (double)H[2 * ((size_t)p * B + i)], gi = (double)H[2 * ((size_t)p * B + i) + 1];
            const int ok = i ? within(gr, re, mag, &worst) && within(gi, im, mag, &worst)
                             : within(gr, re, mag, &worst) && within(gi, ny, mag, &worst);
            if (!ok) {
                fprintf(stderr, "driver: block %d T=%d partition %d entry %d (bin %d): got %.9g %+.9gj, direct DFT %.17g %+.17gj\n", B, T,
                        p, i, k, gr, gi, re, i ? im : ny);
                return 1;
            }
        }
    printf("stream spectra block=%d T=%d P=%d: worst ratio to one float rounding %.3g\n", B, T, P, worst);
    free(taps); free(H); free(cs); free(z);
    return 0;
}

static int drive_handle(int B, int T)
{
    enum { CH = 3, K = 2 };
    const int frame = K * B, keep = T - 1, span = keep > frame ? keep : frame, P = (T + B - 1) / B;
    float *taps = malloc(sizeof(float) * CH * (size_t)T);
    double *taps64 = malloc(sizeof(double) * CH * (size_t)T);
    float *x = calloc((size_t)CH * (size_t)frame, sizeof(float)), *y = calloc((size_t)CH * (size_t)span + 1, sizeof(float));
    int plan[4] = {0, 0, 0, 0};
    CHECK(taps && taps64 && x && y);
    for (size_t i = 0; i < CH * (size_t)T; i++) taps64[i] = taps[i] = rnd();
    /* a tap set per channel */
    unsigned long h = llz_fir_stream_mc_init(CH, B, frame, taps, CH, T);
    CHECK(h != BAD);
    CHECK(llz_fir_stream_mc_flt_len(h) == T);
    CHECK(llz_fir_filter_mc_algo(h) < 0 && llz_fir_bank_mc_algo(h) < 0);      /* a handle of its own kind */
    CHECK(llz_fir_stream_mc_plan(h, plan) == 0 && plan[0] == 2 * B && plan[1] == P && plan[2] == P + K - 1 && plan[3] == K);
    CHECK(llz_fir_stream_mc_plan(h, NULL) < 0);
    for (int c = 0; c < 2 * (P + K); c += K) CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);     /* the head wraps */
    CHECK(llz_fir_stream_mc(h, x, y, frame - B) < 0 && llz_fir_stream_mc(h, x, y, B + 1) < 0);
    CHECK(llz_fir_stream_mc(h, x, x, frame) < 0 && llz_fir_stream_mc(h, NULL, y, frame) < 0 && llz_fir_stream_mc(h, x, NULL, frame) < 0);
    CHECK(llz_fir_stream_mc_set_taps(h, 1, 2, taps) == 0);         /* rows 1 and 2: the last rows of the table */
    CHECK(llz_fir_stream_mc_set_taps(h, 0, CH, taps) == 0);
    CHECK(llz_fir_stream_mc_set_taps(h, 2, 2, taps) < 0 && llz_fir_stream_mc_set_taps(h, -1, 1, taps) < 0);
    CHECK(llz_fir_stream_mc_set_taps(h, 0, 0, taps) < 0 && llz_fir_stream_mc_set_taps(h, 0, 1, NULL) < 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    CHECK(keep ? llz_fir_stream_mc_flush(h, NULL) < 0 : llz_fir_stream_mc_flush(h, NULL) == 0);   /* one tap: nothing to emit */
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);             /* reused after the flush */
    CHECK(llz_fir_stream_mc_reset(h) == 0);
    CHECK(llz_fir_stream_mc_set_stream(h, NULL) == 0);
    llz_fir_stream_mc_uninit(h);
    /* one tap set for all channels, double taps */
    h = llz_fir_stream_mc_init_f64taps(CH, B, B, taps64, 1, T);
    CHECK(h != BAD);
    CHECK(llz_fir_stream_mc_plan(h, plan) == 0 && plan[2] == P && plan[3] == 1);
    CHECK(llz_fir_stream_mc(h, x, y, B) == B);
    CHECK(llz_fir_stream_mc_set_taps(h, 0, 1, taps) == 0);
    CHECK(llz_fir_stream_mc_set_taps(h, 1, 1, taps) < 0 && strstr(llz_hip_last_error(), "llz_fir_stream_mc_set_taps"));
    CHECK(llz_fir_stream_mc_set_taps(h, 0, CH, taps) < 0);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    llz_fir_stream_mc_uninit(h);
    h = llz_fir_stream_mc_init_f64taps(CH, B, frame, taps64, CH, T);
    CHECK(h != BAD);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    llz_fir_stream_mc_uninit(h);
    free(taps); free(taps64); free(x); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][2] = {{64, 1}, {64, 65}, {512, 513}, {128, 131073}};
    for (int i = 0; i < 4; i++) {
        if (pin_builder(shapes[i][0], shapes[i][1])) return 1;
        if (drive_handle(shapes[i][0], shapes[i][1])) return 1;
    }
    {   /* more rows than one staging chunk holds (8 MiB: 7 rows of 1 MB and a bit at 131073 taps, so 19 rows go in three chunks) */
        const int Tl = 131073, ch = 19;
        float *taps = calloc((size_t)ch * Tl, sizeof(float));
        CHECK(taps);
        unsigned long h = llz_fir_stream_mc_init(ch, 4096, 4096, taps, ch, Tl);
        CHECK(h != BAD);
        CHECK(llz_fir_stream_mc_set_taps(h, 2, 17, taps) == 0);
        llz_fir_stream_mc_uninit(h);
        /* refusals: each names the init and its range */
        CHECK(llz_fir_stream_mc_init(0, 64, 64, taps, 1, 63) == BAD && strstr(llz_hip_last_error(), "llz_fir_stream_mc_init") &&
              strstr(llz_hip_last_error(), "1..65535"));
        CHECK(llz_fir_stream_mc_init(2, 96, 96, taps, 1, 63) == BAD && strstr(llz_hip_last_error(), "64..4096"));
        CHECK(llz_fir_stream_mc_init(2, 64, 100, taps, 1, 63) == BAD && strstr(llz_hip_last_error(), "frame_len"));
        CHECK(llz_fir_stream_mc_init(2, 64, 64, taps, 1, Tl + 1) == BAD && strstr(llz_hip_last_error(), "1..131073"));
        CHECK(llz_fir_stream_mc_init(3, 64, 64, taps, 2, 63) == BAD && strstr(llz_hip_last_error(), "rows"));
        CHECK(llz_fir_stream_mc_init(2, 64, 64, NULL, 1, 63) == BAD && strstr(llz_hip_last_error(), "no taps"));
        CHECK(llz_fir_stream_mc_init_f64taps(2, 64, 64, NULL, 1, 63) == BAD && strstr(llz_hip_last_error(), "llz_fir_stream_mc_init_f64taps"));
        /* handles of the other forms are not stream handles, and the other way round */
        int plan[4];
        h = llz_fir_filter_mc_init(2, 64, taps, 1300, LLZ_FIR_ALGO_PARTITIONED);
        CHECK(h != BAD);
        CHECK(llz_fir_stream_mc_plan(h, plan) < 0 && llz_fir_stream_mc_reset(h) < 0 && llz_fir_stream_mc_flt_len(h) < 0);
        llz_fir_filter_mc_uninit(h);
        CHECK(llz_fir_stream_mc_plan(0, plan) < 0 && llz_fir_stream_mc_plan(BAD, plan) < 0);
        free(taps);
    }
    printf("STREAM_SANITIZE_OK\n");
    return 0;
}
