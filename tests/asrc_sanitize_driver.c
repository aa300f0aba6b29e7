/* asrc_sanitize_driver.c -- the host layer of llz_asrc_mc (csrc/host/llz_asrc_host.c) over the generated stub of the device shim,
 * built with -fsanitize=address,undefined by tests/test_asrc_host.py and never loaded into Python.  It runs the script named by
 * argv[1], one command per line,
 *     init <channels> <frame_len> <taps> <phases> <cutoff> <gain> <win> <step>
 *     step <first> <count> <value> <ramp>        the same value for every channel of the range
 *     call <n_in> <out_pitch>
 *     reset
 * and prints, per call, the return value, the counts and the time of every channel's next output; the test compares them with
 * the integer model of tests/asrc_checks.py.  The stub's kernels compute nothing: a staged output row comes back as zeros up to
 * its count, and the driver checks that the caller's row is untouched behind it and that out_len had announced the counts. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_asrc.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)

static int print_state(unsigned long h, int C, long ret, long n_in, const int *counts)
{
    long long *whole = (long long *)malloc(sizeof(long long) * (size_t)C);
    unsigned int *frac = (unsigned int *)malloc(sizeof(unsigned int) * (size_t)C);
    if (!whole || !frac || llz_asrc_mc_next_time(h, 0, C, whole, frac) != LLZ_OK) { free(whole); free(frac); return 1; }
    printf("call %ld ret %ld counts", n_in, ret);
    for (int c = 0; c < C; c++) printf(" %d", counts[c]);
    printf(" times");
    for (int c = 0; c < C; c++) printf(" %lld:%u", whole[c], frac[c]);
    printf("\n");
    free(whole); free(frac);
    return 0;
}

static int refusals(unsigned long h, int C)
{
    int plan[4], n;
    float one[4];
    double st[2] = { 1.0, 99.0 };
    long left[2];
    long long w[2];
    if (llz_asrc_mc_plan(h, plan) != LLZ_OK || plan[2] != plan[0] - 1) FAIL("plan");
    if (llz_asrc_mc_plan(h, NULL) >= 0 || llz_asrc_mc_plan(0, plan) >= 0) FAIL("plan refusals");
    if (llz_asrc_mc_get_table(h, one, 4) >= 0) FAIL("get_table with a short buffer");
    n = (plan[1] + 1) * plan[0];
    float *g = (float *)malloc(sizeof(float) * (size_t)n);
    if (!g || llz_asrc_mc_get_table(h, g, n) != n) FAIL("get_table");
    free(g);
    if (llz_asrc_mc_set_step(h, 0, 1, st + 1, 0) >= 0 || llz_asrc_mc_set_step(h, C, 1, st, 0) >= 0 || llz_asrc_mc_set_step(h, 0, C + 1, st, 0) >= 0 ||
        llz_asrc_mc_set_step(h, 0, 1, st, -1) >= 0 || llz_asrc_mc_set_step(h, 0, 1, NULL, 0) >= 0 || llz_asrc_mc_set_step(h, -1, 1, st, 0) >= 0)
        FAIL("set_step refusals");
    st[1] = NAN;
    if (llz_asrc_mc_set_step(h, 0, 1, st + 1, 0) >= 0) FAIL("set_step NaN");
    if (llz_asrc_mc_get_step(h, 0, 1, st, left) != LLZ_OK || llz_asrc_mc_get_step(h, 0, C + 1, st, NULL) >= 0) FAIL("get_step");
    if (llz_asrc_mc_next_time(h, 0, 1, w, NULL) != LLZ_OK || llz_asrc_mc_next_time(h, C - 1, 2, w, NULL) >= 0) FAIL("next_time");
    if (llz_asrc_mc_out_len(h, -1, NULL) >= 0 || llz_asrc_mc(h, one, -1, one, 4, NULL) >= 0) FAIL("n_in refusals");
    if (llz_asrc_mc_set_stream(h, NULL) != LLZ_OK) FAIL("set_stream");
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int C = 0, frame_len = 0;
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, d, win;
        long n_in, pitch, ramp;
        double cutoff, gain, step;
        if (sscanf(line, "init %d %d %d %d %lf %lf %d %lf", &a, &b, &c, &d, &cutoff, &gain, &win, &step) == 8) {
            if (h != LLZ_BAD_HANDLE) llz_asrc_mc_uninit(h);
            h = llz_asrc_mc_init(a, b, c, d, cutoff, gain, win, step);
            if (h == LLZ_BAD_HANDLE) FAIL("init");
            C = a; frame_len = b;
            if (refusals(h, C)) return 1;
            printf("init %d %d %d %d\n", a, b, c, d);
        } else if (sscanf(line, "step %d %d %lf %ld", &a, &b, &step, &ramp) == 4) {
            double *st = (double *)malloc(sizeof(double) * (size_t)b);
            if (!st) return 1;
            for (int i = 0; i < b; i++) st[i] = step;
            if (llz_asrc_mc_set_step(h, a, b, st, ramp) != LLZ_OK) FAIL("set_step");
            free(st);
        } else if (sscanf(line, "call %ld %ld", &n_in, &pitch) == 2) {
            int *announced = (int *)malloc(sizeof(int) * (size_t)C), *counts = (int *)malloc(sizeof(int) * (size_t)C);
            float *in = (float *)malloc(sizeof(float) * (size_t)C * (size_t)(n_in ? n_in : 1));
            float *out = (float *)malloc(sizeof(float) * (size_t)C * (size_t)(pitch ? pitch : 1));
            if (!announced || !counts || !in || !out || n_in > frame_len) return 1;
            for (long i = 0; i < (long)C * n_in; i++) in[i] = (float)(i % 97) - 48.f;
            for (long i = 0; i < (long)C * pitch; i++) out[i] = CANARY;
            const long most = llz_asrc_mc_out_len(h, n_in, announced);
            if (most < 0) FAIL("out_len");
            memcpy(counts, announced, sizeof(int) * (size_t)C);
            const long ret = llz_asrc_mc(h, in, n_in, out, pitch, counts);
            if (ret < 0) {
                if (most <= pitch) FAIL("a call with room was refused");
                printf("refused: %s\n", llz_hip_last_error());
            } else if (ret != most || memcmp(counts, announced, sizeof(int) * (size_t)C)) {
                FAIL("the call's counts differ from out_len's");
            }
            for (int ch = 0; ch < C; ch++)
                for (long i = 0; i < pitch; i++) {
                    const float want = ret >= 0 && i < counts[ch] ? 0.f : CANARY;
                    if (out[(size_t)ch * (size_t)pitch + (size_t)i] != want) FAIL("channel %d element %ld of the output row", ch, i);
                }
            if (print_state(h, C, ret, n_in, announced)) FAIL("next_time");
            free(announced); free(counts); free(in); free(out);
        } else if (strncmp(line, "reset", 5) == 0) {
            if (llz_asrc_mc_reset(h) != LLZ_OK) FAIL("reset");
        }
    }
    fclose(fp);
    llz_asrc_mc_uninit(h);
    llz_asrc_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    printf("ASRC_SANITIZE_OK\n");
    return 0;
}
