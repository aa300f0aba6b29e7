/* The multi-reference adaptive filter's host layer (llz_adapt_matrix_host.c, and llz_host_stream_taps of llz_spectra.c) under
 * AddressSanitizer + UBSan with the device shim stubbed out (the stub of tests/test_host_sanitizers.py: device memory is malloc,
 * copies are memcpy, kernels return LLZ_OK without computing), at (block, taps) = (64, 1), (64, 65), (512, 513), (128, 131073),
 * 3 inputs into 2 outputs:
 *   * llz_adapt_matrix_mc_init and every call on such handles: calls of every length up to the init's, with and without y, the
 *     head wrapping, set_step / set_taps / get_taps ranges, reset, plan, refusals, handles of the other kinds both ways;
 *   * set_taps -> get_taps of the whole matrix and of a sub-matrix: the spectra are built by the one builder, rounded to float
 *     once (|eps_k| <= u |H_k|, u = 2^-24) and inverted in double; by Cauchy-Schwarz and Parseval a tap comes back within
 *     u |h_p|_2, plus its own rounding: every tap within 2 u |h|_2 of what went in, h its path. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"
#include "llz_adapt.h"
#include "llz_adapt_matrix.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)
#define REFUSED(c, text) CHECK((c) && strstr(llz_hip_last_error(), text))

static unsigned g_seed = 24680u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

/* the worst ratio of |back - taps| to 2 u |h| over `paths` paths of T taps, or -1 with a message */
static double round_trip(const float *taps, const float *back, int paths, int T, int B)
{
    double worst = 0.0;
    for (int c = 0; c < paths; c++) {
        double norm = 0.0;
        for (int t = 0; t < T; t++) norm += (double)taps[(size_t)c * T + t] * (double)taps[(size_t)c * T + t];
        const double lim = 2.0 * ldexp(sqrt(norm), -24);
        for (int t = 0; t < T; t++) {
            const double err = fabs((double)back[(size_t)c * T + t] - (double)taps[(size_t)c * T + t]);
            if (err / lim > worst) worst = err / lim;
            if (err > lim) {
                fprintf(stderr, "driver: block %d T=%d path %d tap %d: %.9g came back as %.9g, limit %.3g\n", B, T, c, t,
                        (double)taps[(size_t)c * T + t], (double)back[(size_t)c * T + t], lim);
                return -1.0;
            }
        }
    }
    return worst;
}

static int drive(int B, int T)
{
    enum { IN = 3, OUT = 2, K = 3 };
    const int frame = K * B, P = (T + B - 1) / B;
    const size_t nt = (size_t)OUT * IN * (size_t)T;
    float *taps = malloc(sizeof(float) * nt), *back = malloc(sizeof(float) * nt + sizeof(float));
    float *x = calloc((size_t)IN * (size_t)frame, sizeof(float)), *d = calloc((size_t)OUT * (size_t)frame, sizeof(float));
    float *e = calloc((size_t)OUT * (size_t)frame, sizeof(float)), *y = calloc((size_t)OUT * (size_t)frame, sizeof(float));
    int plan[6] = {0, 0, 0, 0, 0, 0};
    CHECK(taps && back && x && d && e && y);
    for (size_t i = 0; i < nt; i++) taps[i] = rnd() * expf(-(float)(i % (size_t)T) / (float)(T / 4 + 1));
    unsigned long h = llz_adapt_matrix_mc_init(IN, OUT, B, frame, T, 0.5f, 1e-3f * (float)B * IN);
    CHECK(h != BAD);
    CHECK(llz_adapt_matrix_mc_plan(h, plan) == 0 && plan[0] == 2 * B && plan[1] == P && plan[2] == P + K - 1 && plan[3] == K);
    CHECK(plan[4] >= 1 && plan[5] >= 1 && plan[4] * plan[5] >= IN && (plan[4] - 1) * plan[5] < IN);
    REFUSED(llz_adapt_matrix_mc_plan(h, NULL) < 0, "llz_adapt_matrix_mc_plan");
    /* a handle of its own kind */
    CHECK(llz_fir_stream_mc_plan(h, plan) < 0 && llz_fir_matrix_mc_plan(h, plan) < 0 && llz_fir_matrix_mc_reset(h) < 0);
    CHECK(llz_adapt_mc_plan(h, plan) < 0 && llz_adapt_mc_reset(h, 0) < 0 && llz_fir_filter_mc_algo(h) < 0);
    for (int c = 0; c < 2 * (P + K); c++) {                           /* the head wraps; every call length */
        const int n = (1 + c % K) * B;
        CHECK(llz_adapt_matrix_mc(h, x, d, e, c & 1 ? y : NULL, n) == n);
    }
    REFUSED(llz_adapt_matrix_mc(h, x, d, e, y, frame + B) < 0, "multiple of block");
    REFUSED(llz_adapt_matrix_mc(h, x, d, e, y, B + 1) < 0, "multiple of block");
    REFUSED(llz_adapt_matrix_mc(h, x, d, e, y, 0) < 0, "multiple of block");
    REFUSED(llz_adapt_matrix_mc(h, x, d, x, y, B) < 0, "in-place");
    REFUSED(llz_adapt_matrix_mc(h, x, d, e, d, B) < 0, "in-place");
    REFUSED(llz_adapt_matrix_mc(h, x, d, e, e, B) < 0, "in-place");
    REFUSED(llz_adapt_matrix_mc(h, NULL, d, e, y, B) < 0, "NULL");
    REFUSED(llz_adapt_matrix_mc(h, x, NULL, e, y, B) < 0, "NULL");
    REFUSED(llz_adapt_matrix_mc(h, x, d, NULL, y, B) < 0, "NULL");
    /* step sizes */
    const float mus[OUT] = {0.f, 2.f}, frozen[OUT] = {0.f, 0.f}, neg = -0.5f, big = 2.5f, nan = NAN;
    CHECK(llz_adapt_matrix_mc_set_step(h, 0, OUT, mus) == 0 && llz_adapt_matrix_mc_set_step(h, OUT - 1, 1, mus) == 0);
    REFUSED(llz_adapt_matrix_mc_set_step(h, 1, OUT, mus) < 0, "llz_adapt_matrix_mc_set_step");
    REFUSED(llz_adapt_matrix_mc_set_step(h, -1, 1, mus) < 0, "outputs");
    REFUSED(llz_adapt_matrix_mc_set_step(h, 0, 0, mus) < 0, "outputs");
    REFUSED(llz_adapt_matrix_mc_set_step(h, 0, 1, NULL) < 0, "NULL");
    REFUSED(llz_adapt_matrix_mc_set_step(h, 0, 1, &neg) < 0, "0..2");
    REFUSED(llz_adapt_matrix_mc_set_step(h, 1, 1, &big) < 0, "0..2");
    REFUSED(llz_adapt_matrix_mc_set_step(h, 1, 1, &nan) < 0, "0..2");
    CHECK(llz_adapt_matrix_mc(h, x, d, e, y, B) == B);
    CHECK(llz_adapt_matrix_mc_set_step(h, 0, OUT, frozen) == 0 && llz_adapt_matrix_mc(h, x, d, e, y, frame) == frame);   /* no update */
    /* set_taps -> get_taps, the whole matrix */
    CHECK(llz_adapt_matrix_mc_set_taps(h, 0, OUT, 0, IN, taps) == 0);
    REFUSED(llz_adapt_matrix_mc_set_taps(h, 1, OUT, 0, 1, taps) < 0, "outputs");
    REFUSED(llz_adapt_matrix_mc_set_taps(h, 0, 1, 2, 2, taps) < 0, "inputs");
    REFUSED(llz_adapt_matrix_mc_set_taps(h, 0, 1, -1, 1, taps) < 0, "inputs");
    REFUSED(llz_adapt_matrix_mc_set_taps(h, 0, 1, 0, 0, taps) < 0, "llz_adapt_matrix_mc_set_taps");
    REFUSED(llz_adapt_matrix_mc_set_taps(h, 0, 1, 0, 1, NULL) < 0, "NULL");
    back[nt] = 12345.f;
    CHECK(llz_adapt_matrix_mc_get_taps(h, 0, OUT, 0, IN, back) == 0 && back[nt] == 12345.f);
    REFUSED(llz_adapt_matrix_mc_get_taps(h, 0, OUT + 1, 0, 1, back) < 0, "llz_adapt_matrix_mc_get_taps");
    REFUSED(llz_adapt_matrix_mc_get_taps(h, OUT, 1, 0, 1, back) < 0, "outputs");
    REFUSED(llz_adapt_matrix_mc_get_taps(h, 0, 1, IN, 1, back) < 0, "inputs");
    REFUSED(llz_adapt_matrix_mc_get_taps(h, 0, 1, 0, 1, NULL) < 0, "NULL");
    double worst = round_trip(taps, back, OUT * IN, T, B);
    if (worst < 0.0) return 1;
    /* a sub-matrix: both outputs x inputs 1 and 2 get new taps ([2][2][T]); the paths of input 0 keep theirs to the bit, and the
     * sub-matrix comes back through a buffer of exactly its size */
    {
        const size_t ns = (size_t)OUT * 2 * (size_t)T;
        float *sub = malloc(sizeof(float) * ns), *sback = malloc(sizeof(float) * ns), *all = malloc(sizeof(float) * nt);
        CHECK(sub && sback && all);
        for (size_t i = 0; i < ns; i++) sub[i] = rnd() * expf(-(float)(i % (size_t)T) / (float)(T / 4 + 1));
        CHECK(llz_adapt_matrix_mc_set_taps(h, 0, OUT, 1, 2, sub) == 0);
        CHECK(llz_adapt_matrix_mc_get_taps(h, 0, OUT, 1, 2, sback) == 0 && llz_adapt_matrix_mc_get_taps(h, 0, OUT, 0, IN, all) == 0);
        const double w2 = round_trip(sub, sback, OUT * 2, T, B);
        if (w2 < 0.0) return 1;
        if (w2 > worst) worst = w2;
        for (int o = 0; o < OUT; o++) {
            CHECK(memcmp(all + ((size_t)o * IN) * T, back + ((size_t)o * IN) * T, sizeof(float) * (size_t)T) == 0);
            CHECK(memcmp(all + ((size_t)o * IN + 1) * T, sback + ((size_t)o * 2) * T, sizeof(float) * 2 * (size_t)T) == 0);
        }
        /* one path from the middle, exactly one row */
        float *mid = malloc(sizeof(float) * (size_t)T);
        CHECK(mid && llz_adapt_matrix_mc_get_taps(h, 1, 1, 1, 1, mid) == 0 && memcmp(mid, all + ((size_t)IN + 1) * T, sizeof(float) * (size_t)T) == 0);
        free(mid); free(sub); free(sback);
        /* the delay lines' reset keeps the taps, clear_taps zeroes them */
        CHECK(llz_adapt_matrix_mc_reset(h, 0) == 0 && llz_adapt_matrix_mc_get_taps(h, 0, OUT, 0, IN, back) == 0);
        CHECK(memcmp(all, back, sizeof(float) * nt) == 0);
        free(all);
    }
    CHECK(llz_adapt_matrix_mc_reset(h, 1) == 0 && llz_adapt_matrix_mc_get_taps(h, 0, OUT, 0, IN, back) == 0);
    for (size_t i = 0; i < nt; i++) CHECK(back[i] == 0.f);
    CHECK(llz_adapt_matrix_mc(h, x, d, e, y, frame) == frame);
    CHECK(llz_adapt_matrix_mc_set_stream(h, NULL) == 0);
    llz_adapt_matrix_mc_uninit(h);
    printf("adapt matrix round trip block=%d T=%d P=%d: worst ratio to 2 u |h| %.3g\n", B, T, P, worst);
    free(taps); free(back); free(x); free(d); free(e); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][2] = {{64, 1}, {64, 65}, {512, 513}, {128, 131073}};
    for (int i = 0; i < 4; i++)
        if (drive(shapes[i][0], shapes[i][1])) return 1;
    {   /* the init's refusals: each names the init and its range */
        const char *who = "llz_adapt_matrix_mc_init";
        REFUSED(llz_adapt_matrix_mc_init(0, 2, 64, 64, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "inputs 0 outside 1..4096");
        REFUSED(llz_adapt_matrix_mc_init(4097, 2, 64, 64, 63, 0.5f, 0.1f) == BAD, "inputs 4097 outside 1..4096");
        REFUSED(llz_adapt_matrix_mc_init(2, 0, 64, 64, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "outputs 0 outside 1..4096");
        REFUSED(llz_adapt_matrix_mc_init(2, 4097, 64, 64, 63, 0.5f, 0.1f) == BAD, "outputs 4097 outside 1..4096");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 96, 96, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "64..2048");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 32, 32, 63, 0.5f, 0.1f) == BAD, "64..2048");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 4096, 4096, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "4096 is not built");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 100, 63, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "frame_len");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64 * 65536, 63, 0.5f, 0.1f) == BAD, "frame_len");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 0, 0.5f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "1..131073");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 131074, 0.5f, 0.1f) == BAD, "1..131073");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, -0.1f, 0.1f) == BAD && strstr(llz_hip_last_error(), who), "mu");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, 2.1f, 0.1f) == BAD, "0..2");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, NAN, 0.1f) == BAD, "0..2");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, 0.5f, 0.f) == BAD && strstr(llz_hip_last_error(), who), "delta");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, 0.5f, -1.f) == BAD, "delta");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, 0.5f, INFINITY) == BAD, "delta");
        REFUSED(llz_adapt_matrix_mc_init(2, 2, 64, 64, 63, 0.5f, NAN) == BAD, "delta");
        /* handles of the other forms are not handles of this one */
        int plan[6];
        float buf[64] = {0}, one = 1.f;
        unsigned long s = llz_fir_stream_mc_init(1, 64, 64, &one, 1, 1);
        unsigned long a = llz_adapt_mc_init(1, 64, 64, 1, 0.5f, 0.1f);
        unsigned long m = llz_fir_matrix_mc_init(1, 1, 64, 64, &one, 1);
        CHECK(s != BAD && a != BAD && m != BAD);
        const unsigned long bad[5] = {s, a, m, 0, BAD};
        for (int i = 0; i < 5; i++) {
            REFUSED(llz_adapt_matrix_mc_plan(bad[i], plan) < 0, "llz_adapt_matrix_mc_plan");
            REFUSED(llz_adapt_matrix_mc_reset(bad[i], 0) < 0, "llz_adapt_matrix_mc_reset");
            REFUSED(llz_adapt_matrix_mc(bad[i], buf, buf, buf, NULL, 64) < 0, "llz_adapt_matrix_mc:");
            REFUSED(llz_adapt_matrix_mc_set_step(bad[i], 0, 1, &one) < 0, "llz_adapt_matrix_mc_set_step");
            REFUSED(llz_adapt_matrix_mc_set_taps(bad[i], 0, 1, 0, 1, &one) < 0, "llz_adapt_matrix_mc_set_taps");
            REFUSED(llz_adapt_matrix_mc_get_taps(bad[i], 0, 1, 0, 1, buf) < 0, "llz_adapt_matrix_mc_get_taps");
            REFUSED(llz_adapt_matrix_mc_set_stream(bad[i], NULL) < 0, "llz_adapt_matrix_mc_set_stream");
            llz_adapt_matrix_mc_uninit(bad[i]);                         /* nothing happens */
        }
        CHECK(llz_fir_stream_mc_plan(s, plan) == 0 && llz_adapt_mc_plan(a, plan) == 0 && llz_fir_matrix_mc_plan(m, plan) == 0);
        llz_fir_stream_mc_uninit(s);
        llz_adapt_mc_uninit(a);
        llz_fir_matrix_mc_uninit(m);
    }
    printf("ADAPT_MATRIX_SANITIZE_OK\n");
    return 0;
}
