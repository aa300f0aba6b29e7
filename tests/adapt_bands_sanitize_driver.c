/* adapt_bands_sanitize_driver.c -- the host layer of llz_adapt_bands_mc (csrc/host/llz_adapt_bands_host.c) over the generated
 * stub of the device shim, built with -fsanitize=address,undefined by tests/test_adapt_bands_host.py and never loaded into
 * Python.  It runs the script named by argv[1], one command per line,
 *     init <channels> <bins> <taps>
 *     call <frames> <with_y>
 *     taps                        set_taps of a pattern on a channel range, get_taps of all: the pattern comes back
 *     step                        set_step on a channel range, with a refused value
 *     reset <clear_taps>
 * and prints the frame counter behind every command; the test compares it with its own count.  Every caller buffer is host
 * memory of exactly the size the header states, so a staging copy of another length is an error the sanitizer reports.  Each
 * output has one element more than the call may touch, holding a canary. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_adapt_bands.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)

static int counter(unsigned long h, const char *what)
{
    long long n = -1;
    if (llz_adapt_bands_mc_frames(h, &n) != LLZ_OK) return 1;
    printf("%s frames %lld\n", what, n);
    return 0;
}

static int refusals(unsigned long h, int channels, int bins)
{
    int plan[4];
    long long n;
    float one[4] = { 0 };
    if (llz_adapt_bands_mc_plan(h, NULL) >= 0 || llz_adapt_bands_mc_plan(0, plan) >= 0) FAIL("plan refusals");
    if (llz_adapt_bands_mc_plan(h, plan) != LLZ_OK) FAIL("plan");
    if (llz_adapt_bands_mc(h, one, one, one, one, one, one, NULL, NULL, -1) >= 0) FAIL("negative frames");
    if (bins > 1 && llz_adapt_bands_mc(h, one, one, one, one, one, one, NULL, NULL, 2147483647 / bins + 1) >= 0) FAIL("frames x bins");
    if (llz_adapt_bands_mc(h, NULL, one, one, one, one, one, NULL, NULL, 1) >= 0 ||
        llz_adapt_bands_mc(h, one, one, one, NULL, one, one, NULL, NULL, 1) >= 0 ||
        llz_adapt_bands_mc(h, one, one, one, one, one, NULL, NULL, NULL, 1) >= 0) FAIL("NULL buffers");
    if (llz_adapt_bands_mc(h, one, one, one, one, one, one, one, NULL, 1) >= 0 ||
        llz_adapt_bands_mc(h, one, one, one, one, one, one, NULL, one, 0) >= 0) FAIL("half a y");
    if (llz_adapt_bands_mc(h, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != 0) FAIL("a call of no frames");
    if (llz_adapt_bands_mc_set_step(h, -1, 1, one) >= 0 || llz_adapt_bands_mc_set_step(h, 0, channels + 1, one) >= 0 ||
        llz_adapt_bands_mc_set_step(h, channels, 1, one) >= 0 || llz_adapt_bands_mc_set_step(h, 0, 0, one) >= 0 ||
        llz_adapt_bands_mc_set_step(h, 0, 1, NULL) >= 0) FAIL("set_step ranges");
    if (llz_adapt_bands_mc_set_taps(h, 0, channels + 1, one, one) >= 0 || llz_adapt_bands_mc_set_taps(h, 0, 1, one, NULL) >= 0 ||
        llz_adapt_bands_mc_get_taps(h, channels, 1, one, one) >= 0 || llz_adapt_bands_mc_get_taps(h, 0, 1, NULL, one) >= 0)
        FAIL("taps ranges");
    if (llz_adapt_bands_mc_set_stream(h, NULL) != LLZ_OK || llz_adapt_bands_mc_set_stream(0, NULL) >= 0) FAIL("set_stream");
    if (llz_adapt_bands_mc_frames(h, NULL) >= 0 || llz_adapt_bands_mc_frames(0, &n) >= 0 || llz_adapt_bands_mc_reset(0, 1) >= 0 ||
        llz_adapt_bands_mc_reset(LLZ_BAD_HANDLE, 0) >= 0) FAIL("bad handles");
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int C = 0, B = 0, K = 0;
    if (llz_adapt_bands_mc_init(0, 33, 8, 0.5f, 1e-3f) != LLZ_BAD_HANDLE || llz_adapt_bands_mc_init(2, 4098, 8, 0.5f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_adapt_bands_mc_init(2, 33, 65, 0.5f, 1e-3f) != LLZ_BAD_HANDLE || llz_adapt_bands_mc_init(2, 33, 0, 0.5f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_adapt_bands_mc_init(2, 33, 8, 2.5f, 1e-3f) != LLZ_BAD_HANDLE || llz_adapt_bands_mc_init(2, 33, 8, 0.5f, 0.f) != LLZ_BAD_HANDLE)
        FAIL("an init that must be refused gave a handle");
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, frames, with_y, clear;
        if (sscanf(line, "init %d %d %d", &a, &b, &c) == 3) {
            if (h != LLZ_BAD_HANDLE) llz_adapt_bands_mc_uninit(h);
            h = llz_adapt_bands_mc_init(a, b, c, 0.5f, 1e-3f);
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
            const int ret = llz_adapt_bands_mc(h, in[0], in[1], in[2], in[3], out[0], out[1], with_y ? out[2] : NULL,
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
        } else if (strncmp(line, "taps", 4) == 0) {
            const int first = C > 1 ? 1 : 0, count = C > 2 ? C - 2 : 1;
            const size_t row = (size_t)K * (size_t)B;
            float *wre = (float *)malloc(sizeof(float) * row * (size_t)count), *wim = (float *)malloc(sizeof(float) * row * (size_t)count);
            float *gre = (float *)malloc(sizeof(float) * (row * (size_t)C + 1)), *gim = (float *)malloc(sizeof(float) * (row * (size_t)C + 1));
            if (!wre || !wim || !gre || !gim) return 1;
            for (size_t i = 0; i < row * (size_t)count; i++) { wre[i] = (float)(i % 31) + 1.f; wim[i] = -(float)(i % 29) - 1.f; }
            gre[row * (size_t)C] = gim[row * (size_t)C] = CANARY;
            if (llz_adapt_bands_mc_set_taps(h, first, count, wre, wim) != LLZ_OK) FAIL("set_taps");
            if (llz_adapt_bands_mc_get_taps(h, 0, C, gre, gim) != LLZ_OK) FAIL("get_taps");
            if (memcmp(gre + (size_t)first * row, wre, sizeof(float) * row * (size_t)count) ||
                memcmp(gim + (size_t)first * row, wim, sizeof(float) * row * (size_t)count)) FAIL("get_taps does not return set_taps");
            if (gre[row * (size_t)C] != CANARY || gim[row * (size_t)C] != CANARY) FAIL("get_taps wrote behind its buffers");
            if (llz_adapt_bands_mc_get_taps(h, C - 1, 1, gre, gim) != LLZ_OK) FAIL("get_taps of the last channel");
            free(wre); free(wim); free(gre); free(gim);
            if (counter(h, "taps")) FAIL("frames");
        } else if (strncmp(line, "step", 4) == 0) {
            float *mu = (float *)malloc(sizeof(float) * (size_t)C);
            if (!mu) return 1;
            for (int i = 0; i < C; i++) mu[i] = i % 2 ? 0.f : 1.f;
            if (llz_adapt_bands_mc_set_step(h, 0, C, mu) != LLZ_OK || llz_adapt_bands_mc_set_step(h, C - 1, 1, mu) != LLZ_OK) FAIL("set_step");
            mu[C - 1] = 2.5f;
            if (llz_adapt_bands_mc_set_step(h, 0, C, mu) >= 0) FAIL("a mu of 2.5 was taken");
            free(mu);
            if (counter(h, "step")) FAIL("frames");
        } else if (sscanf(line, "reset %d", &clear) == 1) {
            if (llz_adapt_bands_mc_reset(h, clear) != LLZ_OK) FAIL("reset");
            if (counter(h, "reset")) FAIL("frames");
        }
    }
    fclose(fp);
    llz_adapt_bands_mc_uninit(h);
    llz_adapt_bands_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    printf("ADAPT_BANDS_SANITIZE_OK\n");
    return 0;
}
