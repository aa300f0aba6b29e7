/* kalman_bands_sanitize_driver.c -- the host layer of llz_kalman_bands_mc (csrc/host/llz_kalman_bands_host.c) over the generated
 * stub of the device shim, built with -fsanitize=address,undefined by tests/test_kalman_bands_host.py and never loaded into
 * Python.  It runs the script named by argv[1], one command per line,
 *     init <channels> <bins> <taps>
 *     call <frames> <with_y>
 *     taps                        set_taps of a pattern on a channel range, get_taps of all: the pattern comes back
 *     variance                    the same for set_variance / get_variance, with a negative and a NaN value refused; get_noise
 *     adapt                       set_adapt on a channel range
 *     reset <clear>
 * and prints the frame counter behind every command; the test compares it with its own count.  Every caller buffer is host
 * memory of exactly the size the header states, so a staging copy of another length is an error the sanitizer reports.  Each
 * output has one element more than the call may touch, holding a canary. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_kalman_bands.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)
#define INIT(c, b, k) llz_kalman_bands_mc_init(c, b, k, 0.999f, 0.9f, 1.f, 1e-3f)

static int counter(unsigned long h, const char *what)
{
    long long n = -1;
    if (llz_kalman_bands_mc_frames(h, &n) != LLZ_OK) return 1;
    printf("%s frames %lld\n", what, n);
    return 0;
}

static int refusals(unsigned long h, int channels, int bins)
{
    int plan[4], flag[1] = { 1 };
    long long n;
    float one[4] = { 0 };
    if (llz_kalman_bands_mc_plan(h, NULL) >= 0 || llz_kalman_bands_mc_plan(0, plan) >= 0) FAIL("plan refusals");
    if (llz_kalman_bands_mc_plan(h, plan) != LLZ_OK) FAIL("plan");
    if (llz_kalman_bands_mc(h, one, one, one, one, one, one, NULL, NULL, -1) >= 0) FAIL("negative frames");
    if (bins > 1 && llz_kalman_bands_mc(h, one, one, one, one, one, one, NULL, NULL, 2147483647 / bins + 1) >= 0) FAIL("frames x bins");
    if (llz_kalman_bands_mc(h, NULL, one, one, one, one, one, NULL, NULL, 1) >= 0 ||
        llz_kalman_bands_mc(h, one, one, one, NULL, one, one, NULL, NULL, 1) >= 0 ||
        llz_kalman_bands_mc(h, one, one, one, one, one, NULL, NULL, NULL, 1) >= 0) FAIL("NULL buffers");
    if (llz_kalman_bands_mc(h, one, one, one, one, one, one, one, NULL, 1) >= 0 ||
        llz_kalman_bands_mc(h, one, one, one, one, one, one, NULL, one, 0) >= 0) FAIL("half a y");
    if (llz_kalman_bands_mc(h, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != 0) FAIL("a call of no frames");
    if (llz_kalman_bands_mc_set_adapt(h, -1, 1, flag) >= 0 || llz_kalman_bands_mc_set_adapt(h, 0, channels + 1, flag) >= 0 ||
        llz_kalman_bands_mc_set_adapt(h, channels, 1, flag) >= 0 || llz_kalman_bands_mc_set_adapt(h, 0, 0, flag) >= 0 ||
        llz_kalman_bands_mc_set_adapt(h, 0, 1, NULL) >= 0) FAIL("set_adapt ranges");
    if (llz_kalman_bands_mc_set_taps(h, 0, channels + 1, one, one) >= 0 || llz_kalman_bands_mc_set_taps(h, 0, 1, one, NULL) >= 0 ||
        llz_kalman_bands_mc_get_taps(h, channels, 1, one, one) >= 0 || llz_kalman_bands_mc_get_taps(h, 0, 1, NULL, one) >= 0)
        FAIL("taps ranges");
    if (llz_kalman_bands_mc_set_variance(h, 0, channels + 1, one) >= 0 || llz_kalman_bands_mc_set_variance(h, 0, 1, NULL) >= 0 ||
        llz_kalman_bands_mc_get_variance(h, channels, 1, one) >= 0 || llz_kalman_bands_mc_get_variance(h, 0, 1, NULL) >= 0 ||
        llz_kalman_bands_mc_get_noise(h, -1, 1, one) >= 0 || llz_kalman_bands_mc_get_noise(h, 0, 1, NULL) >= 0)
        FAIL("variance and noise ranges");
    if (llz_kalman_bands_mc_set_stream(h, NULL) != LLZ_OK || llz_kalman_bands_mc_set_stream(0, NULL) >= 0) FAIL("set_stream");
    if (llz_kalman_bands_mc_frames(h, NULL) >= 0 || llz_kalman_bands_mc_frames(0, &n) >= 0 || llz_kalman_bands_mc_reset(0, 1) >= 0 ||
        llz_kalman_bands_mc_reset(LLZ_BAD_HANDLE, 0) >= 0) FAIL("bad handles");
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int C = 0, B = 0, K = 0;
    if (INIT(0, 33, 8) != LLZ_BAD_HANDLE || INIT(2, 4098, 8) != LLZ_BAD_HANDLE || INIT(2, 33, 33) != LLZ_BAD_HANDLE ||
        INIT(2, 33, 65) != LLZ_BAD_HANDLE || INIT(2, 33, 0) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_mc_init(2, 33, 8, 0.f, 0.9f, 1.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_mc_init(2, 33, 8, 0.999f, 1.f, 1.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_mc_init(2, 33, 8, 0.999f, 0.9f, 0.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_mc_init(2, 33, 8, 0.999f, 0.9f, 1.f, 0.f) != LLZ_BAD_HANDLE)
        FAIL("an init that must be refused gave a handle");
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, frames, with_y, clear;
        if (sscanf(line, "init %d %d %d", &a, &b, &c) == 3) {
            if (h != LLZ_BAD_HANDLE) llz_kalman_bands_mc_uninit(h);
            h = INIT(a, b, c);
            if (h == LLZ_BAD_HANDLE) FAIL("init");
            C = a; B = b; K = c;
            if (refusals(h, C, B)) return 1;
            if (counter(h, "init")) FAIL("frames");
        } else if (sscanf(line, "call %d %d", &frames, &with_y) == 2) {
            const size_t n = (size_t)C * (size_t)frames * (size_t)B;
            float *in[4], *out[4];
            for (int k = 0; k < 4; k++) {
                in[k] = (float *)malloc(sizeof(float) * n + 1);           /* exact-size inputs: a copy that reads past them is reported */
                out[k] = (float *)malloc(sizeof(float) * (n + 1));        /* one element more than the call may touch */
                if (!in[k] || !out[k]) return 1;
                for (size_t i = 0; i < n; i++) in[k][i] = (float)((i + (size_t)k) % 97) - 48.f;
                for (size_t i = 0; i <= n; i++) out[k][i] = CANARY;
            }
            const int ret = llz_kalman_bands_mc(h, in[0], in[1], in[2], in[3], out[0], out[1], with_y ? out[2] : NULL,
                                                with_y ? out[3] : NULL, frames);
            if (ret != frames) FAIL("a call of %d frames returned %d", frames, ret);
            for (int k = 0; k < 4; k++) {
                if (out[k][n] != CANARY) FAIL("the element behind output %d was written", k);
                if (k >= 2 && !with_y)
                    for (size_t i = 0; i < n; i++)
                        if (out[k][i] != CANARY) FAIL("a y buffer that was not passed was written");
                free(in[k]); free(out[k]);
            }
            if (counter(h, "call")) FAIL("frames");
        } else if (strncmp(line, "taps", 4) == 0 || strncmp(line, "variance", 8) == 0) {
            const int var = line[0] == 'v', first = C > 1 ? 1 : 0, count = C > 2 ? C - 2 : 1;
            const size_t row = (size_t)K * (size_t)B, n = row * (size_t)count, all = row * (size_t)C;
            float *wre = (float *)malloc(sizeof(float) * n), *wim = (float *)malloc(sizeof(float) * n);
            float *gre = (float *)malloc(sizeof(float) * (all + 1)), *gim = (float *)malloc(sizeof(float) * (all + 1));
            float *psi = (float *)malloc(sizeof(float) * ((size_t)C * (size_t)B + 1));
            if (!wre || !wim || !gre || !gim || !psi) return 1;
            for (size_t i = 0; i < n; i++) { wre[i] = (float)(i % 31) + 1.f; wim[i] = -(float)(i % 29) - 1.f; }
            gre[all] = gim[all] = psi[(size_t)C * (size_t)B] = CANARY;
            if (var) {
                if (llz_kalman_bands_mc_set_variance(h, first, count, wre) != LLZ_OK) FAIL("set_variance");
                if (llz_kalman_bands_mc_set_variance(h, first, count, wim) >= 0) FAIL("negative variances were taken");
                wre[n - 1] = NAN;
                if (llz_kalman_bands_mc_set_variance(h, first, count, wre) >= 0) FAIL("a NaN variance was taken");
                wre[n - 1] = INFINITY;
                if (llz_kalman_bands_mc_set_variance(h, first, count, wre) >= 0) FAIL("an infinite variance was taken");
                wre[n - 1] = 0.f;
                if (llz_kalman_bands_mc_set_variance(h, first, count, wre) != LLZ_OK) FAIL("a variance of 0 was refused");
                if (llz_kalman_bands_mc_get_variance(h, 0, C, gre) != LLZ_OK) FAIL("get_variance");
                if (memcmp(gre + (size_t)first * row, wre, sizeof(float) * n)) FAIL("get_variance does not return set_variance");
                if (llz_kalman_bands_mc_get_noise(h, 0, C, psi) != LLZ_OK || llz_kalman_bands_mc_get_noise(h, C - 1, 1, psi) != LLZ_OK)
                    FAIL("get_noise");
            } else {
                if (llz_kalman_bands_mc_set_taps(h, first, count, wre, wim) != LLZ_OK) FAIL("set_taps");
                if (llz_kalman_bands_mc_get_taps(h, 0, C, gre, gim) != LLZ_OK) FAIL("get_taps");
                if (memcmp(gre + (size_t)first * row, wre, sizeof(float) * n) || memcmp(gim + (size_t)first * row, wim, sizeof(float) * n))
                    FAIL("get_taps does not return set_taps");
                if (llz_kalman_bands_mc_get_taps(h, C - 1, 1, gre, gim) != LLZ_OK) FAIL("get_taps of the last channel");
            }
            if (gre[all] != CANARY || gim[all] != CANARY || psi[(size_t)C * (size_t)B] != CANARY) FAIL("a get wrote behind its buffer");
            free(wre); free(wim); free(gre); free(gim); free(psi);
            if (counter(h, var ? "variance" : "taps")) FAIL("frames");
        } else if (strncmp(line, "adapt", 5) == 0) {
            int *on = (int *)malloc(sizeof(int) * (size_t)C);
            if (!on) return 1;
            for (int i = 0; i < C; i++) on[i] = i % 2 ? 0 : 7;
            if (llz_kalman_bands_mc_set_adapt(h, 0, C, on) != LLZ_OK || llz_kalman_bands_mc_set_adapt(h, C - 1, 1, on) != LLZ_OK) FAIL("set_adapt");
            free(on);
            if (counter(h, "adapt")) FAIL("frames");
        } else if (sscanf(line, "reset %d", &clear) == 1) {
            if (llz_kalman_bands_mc_reset(h, clear) != LLZ_OK) FAIL("reset");
            if (counter(h, "reset")) FAIL("frames");
        }
    }
    fclose(fp);
    llz_kalman_bands_mc_uninit(h);
    llz_kalman_bands_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    printf("KALMAN_BANDS_SANITIZE_OK\n");
    return 0;
}
