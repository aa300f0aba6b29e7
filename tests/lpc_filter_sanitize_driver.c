/* The LPC filters' host layer (llz_lpc_filter_host.c) under AddressSanitizer + UBSan with the device shim stubbed out (the stub
 * of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without computing):
 * init at the least and at odd sizes, both calls with host pointers in buffers of exactly the documented sizes (so a staging
 * copy one element too long is a heap overflow), growing and shrinking calls on one handle, reset, set_stream, every refusal
 * with its message, uninit.  synth_host() is the plain C loop of the pinned synthesis recursion (one core, no numpy) that
 * tools/time_lpc_filter.py quotes next to the device's figures; here it runs under the sanitizers on the same shapes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_lpc.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static unsigned g_seed = 13579u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

/* y[t] = e[t] - sum a_f[k] yd[t-k], k = p .. 1, double state yd[c][i] = y(-1 - i) (this file is built with contraction off) */
static void synth_host(const float *e, const float *acof, float *y, double *state, int channels, int frames, int frame_len, int p)
{
    const long T = (long)frames * frame_len;
    for (int c = 0; c < channels; c++) {
        double *yd = state + (size_t)c * 64;
        for (long t = 0; t < T; t++) {
            const float *a = acof + ((size_t)c * frames + (size_t)(t / frame_len)) * (p + 1);
            double acc = (double)e[c * T + t];
            for (int k = p; k >= 1; k--) {
                const double prod = (double)a[k] * yd[k - 1];
                acc = acc - prod;
            }
            for (int k = p - 1; k >= 1; k--) yd[k] = yd[k - 1];
            if (p) yd[0] = acc;
            y[c * T + t] = (float)acc;
        }
    }
}

static int has(const char *needle) { return strstr(llz_hip_last_error(), needle) != NULL; }

static int walk(int channels, int frame_len, int p, int max_frames)
{
    unsigned long h = llz_lpc_filter_mc_init(channels, frame_len, p);
    CHECK(h != BAD && h != 0);
    const int plan[5] = {1, max_frames, 2 > max_frames ? 1 : 2, max_frames, 1};
    for (int i = 0; i < 5; i++) {
        const int frames = plan[i];
        const size_t n = (size_t)channels * frames * frame_len, nc = (size_t)channels * frames * (p + 1);
        float *x = malloc(sizeof(float) * n), *e = malloc(sizeof(float) * n), *y = malloc(sizeof(float) * n);
        float *a = malloc(sizeof(float) * nc);
        double *state = calloc((size_t)channels * 64, sizeof(double));
        CHECK(x && e && y && a && state);
        for (size_t j = 0; j < n; j++) x[j] = rnd();
        for (size_t j = 0; j < nc; j++) a[j] = j % (size_t)(p + 1) ? 0.5f * rnd() / (float)(p + 1) : 1.0f;
        CHECK(llz_lpc_residual_mc(h, x, a, e, frames) == frames);
        CHECK(llz_lpc_synth_mc(h, x, a, y, frames) == frames);
        synth_host(x, a, y, state, channels, frames, frame_len, p);
        if (i == 2) CHECK(llz_lpc_filter_mc_reset(h) == LLZ_OK);
        if (i == 3) CHECK(llz_lpc_filter_mc_set_stream(h, NULL) == LLZ_OK);
        /* refusals on a live handle: nothing staged, each with its own message */
        CHECK(llz_lpc_residual_mc(h, x, a, e, 0) < 0 && has("llz_lpc_residual_mc") && has("frames 0"));
        CHECK(llz_lpc_synth_mc(h, x, a, y, -3) < 0 && has("llz_lpc_synth_mc") && has("frames -3"));
        CHECK(llz_lpc_residual_mc(h, NULL, a, e, frames) < 0 && has("NULL"));
        CHECK(llz_lpc_residual_mc(h, x, NULL, e, frames) < 0 && has("NULL"));
        CHECK(llz_lpc_synth_mc(h, x, a, NULL, frames) < 0 && has("llz_lpc_synth_mc") && has("NULL"));
        free(x); free(e); free(y); free(a); free(state);
    }
    llz_lpc_filter_mc_uninit(h);
    printf("lpc filter channels=%d frame_len=%d p=%d frames<=%d ok\n", channels, frame_len, p, max_frames);
    return 0;
}

int main(void)
{
    /* the least sizes, odd ones, the largest order */
    if (walk(1, 1, 0, 1) || walk(1, 2, 1, 3) || walk(3, 50, 7, 5) || walk(37, 17, 16, 7) || walk(5, 65, 64, 2) ||
        walk(2, 1023, 33, 3))
        return 1;
    CHECK(llz_lpc_filter_mc_init(0, 10, 2) == BAD && has("llz_lpc_filter_mc_init") && has("channels 0"));
    CHECK(llz_lpc_filter_mc_init(2, 10, -1) == BAD && has("p -1"));
    CHECK(llz_lpc_filter_mc_init(2, 100, 65) == BAD && has("p 65"));
    CHECK(llz_lpc_filter_mc_init(2, 16, 16) == BAD && has("frame_len 16"));
    float one[4] = {1, 0, 0, 0};
    const unsigned long bad[2] = {0, BAD};
    for (int i = 0; i < 2; i++) {
        CHECK(llz_lpc_residual_mc(bad[i], one, one, one, 1) < 0 && has("llz_lpc_residual_mc") && has("bad handle"));
        CHECK(llz_lpc_synth_mc(bad[i], one, one, one, 1) < 0 && has("llz_lpc_synth_mc") && has("bad handle"));
        CHECK(llz_lpc_filter_mc_reset(bad[i]) < 0 && has("llz_lpc_filter_mc_reset"));
        CHECK(llz_lpc_filter_mc_set_stream(bad[i], NULL) < 0 && has("llz_lpc_filter_mc_set_stream"));
        llz_lpc_filter_mc_uninit(bad[i]);
    }
    /* a handle of another kind fails the tag check */
    unsigned long other = llz_lpc_init(4);
    CHECK(other != BAD);
    CHECK(llz_lpc_residual_mc(other, one, one, one, 1) < 0 && has("bad handle"));
    llz_lpc_filter_mc_uninit(other);
    llz_lpc_uninit(other);
    printf("LPC_FILTER_SANITIZE_OK\n");
    return 0;
}
