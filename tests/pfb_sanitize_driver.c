/* pfb_sanitize_driver.c -- the host layer of llz_pfb_mc (csrc/host/llz_pfb_host.c) over the generated stub of the device shim,
 * built with -fsanitize=address,undefined by tests/test_pfb_host.py and never loaded into Python.  It runs the script named by
 * argv[1], one command per line,
 *     init <channels> <bands> <hop> <taps_per_band> <phase> <own_g>
 *     analysis <frames>
 *     synthesis <frames>
 *     reset
 * and prints the two frame counters behind every command; the test compares them with its own count.  Every caller buffer is
 * host memory of exactly the size the header states, so a staging copy of another length is an error the sanitizer reports.  Each
 * output has one element more than the call may touch, holding a canary. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_pfb.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)

static int counters(unsigned long h, const char *what, int frames)
{
    long long a = -1, s = -1;
    if (llz_pfb_mc_frames(h, &a, &s) != LLZ_OK || llz_pfb_mc_frames(h, NULL, NULL) != LLZ_OK) return 1;
    printf("%s %d frames %lld %lld\n", what, frames, a, s);
    return 0;
}

static int refusals(unsigned long h)
{
    int plan[8];
    float one[4] = { 0 };
    if (llz_pfb_mc_plan(h, 0, plan) >= 0 || llz_pfb_mc_plan(h, 4, NULL) >= 0 || llz_pfb_mc_plan(0, 4, plan) >= 0) FAIL("plan refusals");
    if (llz_pfb_mc_plan(h, 4, plan) != LLZ_OK) FAIL("plan");
    if (llz_pfb_mc_analysis(h, one, one, one, -1) >= 0 || llz_pfb_mc_synthesis(h, one, one, one, -1) >= 0) FAIL("negative frames");
    if (llz_pfb_mc_analysis(h, NULL, one, one, 1) >= 0 || llz_pfb_mc_analysis(h, one, NULL, one, 1) >= 0 ||
        llz_pfb_mc_synthesis(h, one, one, NULL, 1) >= 0 || llz_pfb_mc_synthesis(h, one, NULL, one, 1) >= 0) FAIL("NULL buffers");
    if (llz_pfb_mc_analysis(h, NULL, NULL, NULL, 0) != 0 || llz_pfb_mc_synthesis(h, NULL, NULL, NULL, 0) != 0) FAIL("calls of no frames");
    if (llz_pfb_mc_set_stream(h, NULL) != LLZ_OK || llz_pfb_mc_set_stream(0, NULL) >= 0) FAIL("set_stream");
    if (llz_pfb_mc_bins(0) >= 0 || llz_pfb_mc_delay(LLZ_BAD_HANDLE) >= 0 || llz_pfb_mc_reset(0) >= 0 || llz_pfb_mc_frames(0, NULL, NULL) >= 0)
        FAIL("bad handles");
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int C = 0, M = 0, D = 0, P = 0;
    float bad[8] = { 0 };
    if (llz_pfb_mc_init(0, 64, 32, 4, bad, NULL, 0) != LLZ_BAD_HANDLE || llz_pfb_mc_init(2, 48, 24, 1, bad, NULL, 0) != LLZ_BAD_HANDLE ||
        llz_pfb_mc_init(2, 64, 4, 1, bad, NULL, 0) != LLZ_BAD_HANDLE || llz_pfb_mc_init(2, 64, 32, 17, bad, NULL, 0) != LLZ_BAD_HANDLE ||
        llz_pfb_mc_init(2, 4096, 4096, 9, bad, NULL, 0) != LLZ_BAD_HANDLE || llz_pfb_mc_init(2, 64, 32, 4, NULL, bad, 0) != LLZ_BAD_HANDLE ||
        llz_pfb_mc_init(2, 64, 32, 4, bad, NULL, 2) != LLZ_BAD_HANDLE)
        FAIL("an init that must be refused gave a handle");
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, d, phase, own_g, frames;
        if (sscanf(line, "init %d %d %d %d %d %d", &a, &b, &c, &d, &phase, &own_g) == 6) {
            if (h != LLZ_BAD_HANDLE) llz_pfb_mc_uninit(h);
            const size_t L = (size_t)b * (size_t)d;
            float *w = (float *)malloc(sizeof(float) * L), *g = (float *)malloc(sizeof(float) * L);
            if (!w || !g) return 1;
            for (size_t i = 0; i < L; i++) { w[i] = (float)(i % 13) - 6.f; g[i] = 1.f; }
            h = llz_pfb_mc_init(a, b, c, d, w, own_g ? g : NULL, phase);
            free(w); free(g);                                       /* the windows are copied: the handle must not read them again */
            if (h == LLZ_BAD_HANDLE) FAIL("init");
            C = a; M = b; D = c; P = d;
            if (llz_pfb_mc_bins(h) != M / 2 + 1 || llz_pfb_mc_delay(h) != P * M - D) FAIL("bins %d delay %d", llz_pfb_mc_bins(h), llz_pfb_mc_delay(h));
            if (refusals(h)) return 1;
            if (counters(h, "init", 0)) FAIL("frames");
        } else if (sscanf(line, "analysis %d", &frames) == 1 || sscanf(line, "synthesis %d", &frames) == 1) {
            const int ana = line[0] == 'a';
            const size_t nx = (size_t)C * (size_t)frames * (size_t)D, ns = (size_t)C * (size_t)frames * (size_t)(M / 2 + 1);
            /* one element more than the call may touch, holding a canary, at the end of each output */
            float *x = (float *)malloc(sizeof(float) * (nx + 1)), *re = (float *)malloc(sizeof(float) * (ns + 1));
            float *im = (float *)malloc(sizeof(float) * (ns + 1));
            if (!x || !re || !im) return 1;
            for (size_t i = 0; i <= nx; i++) x[i] = ana ? (float)(i % 97) - 48.f : CANARY;
            for (size_t i = 0; i <= ns; i++) re[i] = im[i] = ana ? CANARY : (float)(i % 89) - 44.f;
            /* exact-size inputs: a staging copy that reads past them is reported */
            float *in0 = (float *)malloc(sizeof(float) * (ana ? nx : ns) + 1), *in1 = (float *)malloc(sizeof(float) * ns + 1);
            if (!in0 || !in1) return 1;
            memcpy(in0, ana ? x : re, sizeof(float) * (ana ? nx : ns));
            memcpy(in1, im, sizeof(float) * ns);
            const int ret = ana ? llz_pfb_mc_analysis(h, in0, re, im, frames) : llz_pfb_mc_synthesis(h, in0, in1, x, frames);
            if (ret != frames) FAIL("%s of %d frames returned %d", ana ? "analysis" : "synthesis", frames, ret);
            /* (the stages serve both directions and the stub's kernels write nothing: only the canaries are known) */
            if (ana ? (re[ns] != CANARY || im[ns] != CANARY) : (x[nx] != CANARY)) FAIL("the element behind an output was written");
            if (counters(h, ana ? "analysis" : "synthesis", frames)) FAIL("frames");
            free(x); free(re); free(im); free(in0); free(in1);
        } else if (strncmp(line, "reset", 5) == 0) {
            if (llz_pfb_mc_reset(h) != LLZ_OK) FAIL("reset");
            if (counters(h, "reset", 0)) FAIL("frames");
        }
    }
    fclose(fp);
    llz_pfb_mc_uninit(h);
    llz_pfb_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    printf("PFB_SANITIZE_OK\n");
    return 0;
}
