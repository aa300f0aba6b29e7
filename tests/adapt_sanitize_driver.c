/* The adaptive filter's host layer (llz_adapt_host.c, and llz_host_stream_taps of llz_spectra.c) under AddressSanitizer + UBSan
 * with the device shim stubbed out (the stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy,
 * kernels return LLZ_OK without computing), at (block, taps) = (64, 1), (64, 65), (512, 513), (128, 131073):
 *   * llz_adapt_mc_init and every call on such handles: calls of every length up to the init's, with and without y, the head
 *     wrapping, set_step / set_taps / get_taps ranges, reset, plan, refusals, handles of the other kinds;
 *   * set_taps -> get_taps: the spectra are built by the one builder, rounded to float once (|eps_k| <= u |H_k|, u = 2^-24) and
 *     inverted in double; by Cauchy-Schwarz and Parseval a tap comes back within u |h_p|_2, plus its own rounding: every tap
 *     within 2 u |h|_2 of what went in. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "llz_adapt.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)
#define REFUSED(c, text) CHECK((c) && strstr(llz_hip_last_error(), text))

static unsigned g_seed = 13579u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

static int drive(int B, int T)
{
    enum { CH = 3, K = 3 };
    const int frame = K * B, P = (T + B - 1) / B;
    const size_t nt = (size_t)CH * (size_t)T;
    float *taps = malloc(sizeof(float) * nt), *back = malloc(sizeof(float) * nt + sizeof(float));
    float *x = calloc((size_t)CH * (size_t)frame, sizeof(float)), *d = calloc((size_t)CH * (size_t)frame, sizeof(float));
    float *e = calloc((size_t)CH * (size_t)frame, sizeof(float)), *y = calloc((size_t)CH * (size_t)frame, sizeof(float));
    int plan[4] = {0, 0, 0, 0};
    CHECK(taps && back && x && d && e && y);
    for (size_t i = 0; i < nt; i++) taps[i] = rnd() * expf(-(float)(i % (size_t)T) / (float)(T / 4 + 1));
    unsigned long h = llz_adapt_mc_init(CH, B, frame, T, 0.5f, 1e-3f * (float)B);
    CHECK(h != BAD);
    CHECK(llz_adapt_mc_plan(h, plan) == 0 && plan[0] == 2 * B && plan[1] == P && plan[2] == P + K - 1 && plan[3] == K);
    REFUSED(llz_adapt_mc_plan(h, NULL) < 0, "llz_adapt_mc_plan");
    /* a handle of its own kind */
    CHECK(llz_fir_stream_mc_plan(h, plan) < 0 && llz_fir_stream_mc_reset(h) < 0 && llz_fir_filter_mc_algo(h) < 0 && llz_fir_bank_mc_algo(h) < 0);
    for (int c = 0; c < 2 * (P + K); c++) {                           /* the head wraps; every call length */
        const int n = (1 + c % K) * B;
        CHECK(llz_adapt_mc(h, x, d, e, c & 1 ? y : NULL, n) == n);
    }
    REFUSED(llz_adapt_mc(h, x, d, e, y, frame + B) < 0, "frame_len");
    REFUSED(llz_adapt_mc(h, x, d, e, y, B + 1) < 0, "frame_len");
    REFUSED(llz_adapt_mc(h, x, d, e, y, 0) < 0, "frame_len");
    REFUSED(llz_adapt_mc(h, x, d, x, y, B) < 0, "in-place");
    REFUSED(llz_adapt_mc(h, x, d, e, d, B) < 0, "in-place");
    REFUSED(llz_adapt_mc(h, x, d, e, e, B) < 0, "in-place");
    REFUSED(llz_adapt_mc(h, NULL, d, e, y, B) < 0, "NULL");
    REFUSED(llz_adapt_mc(h, x, NULL, e, y, B) < 0, "NULL");
    REFUSED(llz_adapt_mc(h, x, d, NULL, y, B) < 0, "NULL");
    /* step sizes */
    const float mus[CH] = {0.f, 2.f, 0.25f}, frozen[CH] = {0.f, 0.f, 0.f}, neg = -0.5f, big = 2.5f, nan = NAN;
    CHECK(llz_adapt_mc_set_step(h, 0, CH, mus) == 0 && llz_adapt_mc_set_step(h, CH - 1, 1, mus) == 0);
    REFUSED(llz_adapt_mc_set_step(h, 1, CH, mus) < 0, "llz_adapt_mc_set_step");
    REFUSED(llz_adapt_mc_set_step(h, -1, 1, mus) < 0, "channels");
    REFUSED(llz_adapt_mc_set_step(h, 0, 0, mus) < 0, "channels");
    REFUSED(llz_adapt_mc_set_step(h, 0, 1, NULL) < 0, "NULL");
    REFUSED(llz_adapt_mc_set_step(h, 0, 1, &neg) < 0, "0..2");
    REFUSED(llz_adapt_mc_set_step(h, 1, 1, &big) < 0, "0..2");
    REFUSED(llz_adapt_mc_set_step(h, 2, 1, &nan) < 0, "0..2");
    CHECK(llz_adapt_mc(h, x, d, e, y, B) == B);
    CHECK(llz_adapt_mc_set_step(h, 0, CH, frozen) == 0 && llz_adapt_mc(h, x, d, e, y, frame) == frame);    /* no update launched */
    /* set_taps -> get_taps */
    CHECK(llz_adapt_mc_set_taps(h, 0, CH, taps) == 0);
    CHECK(llz_adapt_mc_set_taps(h, 1, 2, taps + T) == 0);
    REFUSED(llz_adapt_mc_set_taps(h, 2, 2, taps) < 0, "llz_adapt_mc_set_taps");
    REFUSED(llz_adapt_mc_set_taps(h, 0, 1, NULL) < 0, "NULL");
    back[nt] = 12345.f;
    CHECK(llz_adapt_mc_get_taps(h, 0, CH, back) == 0 && back[nt] == 12345.f);
    REFUSED(llz_adapt_mc_get_taps(h, 0, CH + 1, back) < 0, "llz_adapt_mc_get_taps");
    REFUSED(llz_adapt_mc_get_taps(h, CH, 1, back) < 0, "channels");
    REFUSED(llz_adapt_mc_get_taps(h, 0, 1, NULL) < 0, "NULL");
    double worst = 0.0;
    for (int c = 0; c < CH; c++) {
        double norm = 0.0;
        for (int t = 0; t < T; t++) norm += (double)taps[(size_t)c * T + t] * (double)taps[(size_t)c * T + t];
        const double lim = 2.0 * ldexp(sqrt(norm), -24);
        for (int t = 0; t < T; t++) {
            const double err = fabs((double)back[(size_t)c * T + t] - (double)taps[(size_t)c * T + t]);
            if (err / lim > worst) worst = err / lim;
            if (err > lim) {
                fprintf(stderr, "driver: block %d T=%d channel %d tap %d: %.9g came back as %.9g, limit %.3g\n", B, T, c, t,
                        (double)taps[(size_t)c * T + t], (double)back[(size_t)c * T + t], lim);
                return 1;
            }
        }
    }
    /* one channel from the middle; the delay line's reset keeps the taps, clear_taps zeroes them */
    float *mid = malloc(sizeof(float) * (size_t)T);                    /* exactly one row */
    CHECK(mid && llz_adapt_mc_get_taps(h, 1, 1, mid) == 0 && memcmp(mid, back + T, sizeof(float) * (size_t)T) == 0);
    free(mid);
    CHECK(llz_adapt_mc_reset(h, 0) == 0 && llz_adapt_mc_get_taps(h, 0, CH, back) == 0);
    for (int c = 0; c < CH; c++) CHECK(fabs((double)back[(size_t)c * T] - (double)taps[(size_t)c * T]) <= 1e-6);
    CHECK(llz_adapt_mc_reset(h, 1) == 0 && llz_adapt_mc_get_taps(h, 0, CH, back) == 0);
    for (size_t i = 0; i < nt; i++) CHECK(back[i] == 0.f);
    CHECK(llz_adapt_mc(h, x, d, e, y, frame) == frame);
    CHECK(llz_adapt_mc_set_stream(h, NULL) == 0);
    llz_adapt_mc_uninit(h);
    printf("adapt round trip block=%d T=%d P=%d: worst ratio to 2 u |h| %.3g\n", B, T, P, worst);
    free(taps); free(back); free(x); free(d); free(e); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][2] = {{64, 1}, {64, 65}, {512, 513}, {128, 131073}};
    for (int i = 0; i < 4; i++)
        if (drive(shapes[i][0], shapes[i][1])) return 1;
    {   /* the init's refusals: each names the init and its range */
        const char *who = "llz_adapt_mc_init";
        REFUSED(llz_adapt_mc_init(0, 64, 64, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "1..65535");
        REFUSED(llz_adapt_mc_init(65536, 64, 64, 63, 0.5f, 0.1f) == BAD, "1..65535");
        REFUSED(llz_adapt_mc_init(2, 96, 96, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "64..2048");
        REFUSED(llz_adapt_mc_init(2, 32, 32, 63, 0.5f, 0.1f) == BAD, "64..2048");
        REFUSED(llz_adapt_mc_init(2, 4096, 4096, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "4096 is not built");
        REFUSED(llz_adapt_mc_init(2, 64, 100, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "frame_len");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 0, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "1..131073");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 131074, 0.5f, 0.1f) == BAD, "1..131073");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, -0.1f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "mu");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, 2.1f, 0.1f) == BAD, "0..2");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, NAN, 0.1f) == BAD, "0..2");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, 0.5f, 0.f) == BAD && strstr(llz_hip_last_error(), who), "delta");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, 0.5f, -1.f) == BAD, "delta");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, 0.5f, INFINITY) == BAD, "delta");
        REFUSED(llz_adapt_mc_init(2, 64, 64, 63, 0.5f, NAN) == BAD, "delta");
        /* handles of the other forms are not adaptive handles */
        int plan[4];
        float buf[64] = {0}, one = 1.f;
        unsigned long s = llz_fir_stream_mc_init(1, 64, 64, &one, 1, 1);
        CHECK(s != BAD);
        const unsigned long bad[3] = {s, 0, BAD};
        for (int i = 0; i < 3; i++) {
            REFUSED(llz_adapt_mc_plan(bad[i], plan) < 0, "llz_adapt_mc_plan");
            REFUSED(llz_adapt_mc_reset(bad[i], 0) < 0, "llz_adapt_mc_reset");
            REFUSED(llz_adapt_mc(bad[i], buf, buf, buf, NULL, 64) < 0, "llz_adapt_mc:");
            REFUSED(llz_adapt_mc_set_step(bad[i], 0, 1, &one) < 0, "llz_adapt_mc_set_step");
            REFUSED(llz_adapt_mc_set_taps(bad[i], 0, 1, &one) < 0, "llz_adapt_mc_set_taps");
            REFUSED(llz_adapt_mc_get_taps(bad[i], 0, 1, buf) < 0, "llz_adapt_mc_get_taps");
            REFUSED(llz_adapt_mc_set_stream(bad[i], NULL) < 0, "llz_adapt_mc_set_stream");
            llz_adapt_mc_uninit(bad[i]);                                /* nothing happens */
        }
        CHECK(llz_fir_stream_mc_plan(s, plan) == 0);
        llz_fir_stream_mc_uninit(s);
    }
    printf("ADAPT_SANITIZE_OK\n");
    return 0;
}
