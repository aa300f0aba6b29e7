/* The time-delay estimator's host layer (llz_tde_host.c) under AddressSanitizer + UBSan with the device shim stubbed out (the
 * stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without computing):
 * init at every size and hop, scripted streams of ragged call sizes with host buffers of exactly the documented sizes (a staging
 * copy one element too long is a heap overflow), the frame counts and frames_for against the integer model of the frame grid,
 * the tail of every output row behind the frames written, reset, set_forget, both read-outs into exact buffers, refused calls
 * that leave the frame count where it was, every refusal with its message, uninit. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_lpc.h"
#include "llz_tde.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static int has(const char *needle) { return strstr(llz_hip_last_error(), needle) != NULL; }

static long frames_after(long hops, int N, int hop)
{
    const long lead = N / hop - 1;
    return hops > lead ? hops - lead : 0;
}

/* one call of hops_in_call hops with exact host buffers, out_pitch = frames + extra; the tail of every row must keep its fill */
static long feed(unsigned long h, int channels, int pairs, int hop, long hops_in_call, long expect, long extra, int with_peak)
{
    const size_t n = (size_t)hops_in_call * hop;
    const long pitch = expect + extra;
    float *x = malloc(sizeof(float) * channels * n);
    float *delay = malloc(sizeof(float) * (size_t)pairs * (pitch ? pitch : 1));
    float *peak = malloc(sizeof(float) * (size_t)pairs * (pitch ? pitch : 1));
    if (!x || !delay || !peak) return -100;
    for (size_t j = 0; j < channels * n; j++) x[j] = (float)(j % 17) - 8.0f;
    for (long j = 0; j < pairs * pitch; j++) delay[j] = peak[j] = 77.0f;
    long got = llz_tde_mc_frames_for(h, (long)n);
    if (got == expect) got = llz_tde_mc_process(h, x, (long)n, delay, with_peak ? peak : NULL, pitch);
    for (int p = 0; p < pairs && got == expect; p++)
        for (long j = expect; j < pitch; j++)
            if (delay[p * pitch + j] != 77.0f || peak[p * pitch + j] != 77.0f) got = -200;
    free(x); free(delay); free(peak);
    return got;
}

static int walk(int channels, int pairs, int N, int hop, int weight)
{
    int *table = malloc(sizeof(int) * 2 * pairs);
    CHECK(table);
    for (int p = 0; p < 2 * pairs; p++) table[p] = (p * 7 + p / 2) % channels;
    const int L = N / 2 - 1 - (N / 64) % 5;
    unsigned long h = llz_tde_mc_init(channels, pairs, table, N, hop, (win_t)(N / 64 % 3), L, weight, 1, N / 2 - 1, 0.9f, 0.0f);
    free(table);                                                    /* the handle keeps its own copy */
    CHECK(h != BAD && h != 0);
    const int bins = N / 2 + 1;
    float *curve = malloc(sizeof(float) * pairs * (2 * L + 1));
    float *state = malloc(sizeof(float) * 4 * pairs * bins);
    CHECK(curve && state);
    CHECK(llz_tde_mc_frames(h) == 0);
    CHECK(llz_tde_mc_read(h, LLZ_TDE_CURVE, curve) == LLZ_ERR_ARG && has("llz_tde_mc_read") && has("no frame yet"));
    /* one hop at a time up to the first frames, then ragged calls */
    const long calls[] = {1, 1, 1, 1, 20, 15, 69, 1};
    long hops = 0;
    for (unsigned i = 0; i < sizeof(calls) / sizeof(calls[0]); i++) {
        const long lo = frames_after(hops, N, hop), hi = frames_after(hops + calls[i], N, hop);
        hops += calls[i];
        CHECK(feed(h, channels, pairs, hop, calls[i], hi - lo, (long)(i % 3), i % 2 == 0) == hi - lo);
        CHECK(llz_tde_mc_frames(h) == hi);
        if (hi > 0) {
            CHECK(llz_tde_mc_read(h, LLZ_TDE_CURVE, curve) == LLZ_OK);
            CHECK(llz_tde_mc_read(h, LLZ_TDE_STATE, state) == LLZ_OK);
        }
        if (i == 4) CHECK(llz_tde_mc_set_forget(h, 0.5f) == LLZ_OK);
        if (i == 5) CHECK(llz_tde_mc_set_stream(h, NULL) == LLZ_OK && llz_tde_mc_set_forget(h, 0.0f) == LLZ_OK);
    }
    /* refusals on a live handle: the frame count stays */
    const long at = llz_tde_mc_frames(h);
    float one[8] = {0}, out[8] = {0};
    CHECK(llz_tde_mc_process(h, one, hop + 1, out, NULL, 8) == LLZ_ERR_ARG && has("llz_tde_mc_process") && has("multiple of hop"));
    CHECK(llz_tde_mc_process(h, one, 0, out, NULL, 8) == LLZ_ERR_ARG && has("llz_tde_mc_process"));
    CHECK(llz_tde_mc_process(h, NULL, hop, out, NULL, 8) == LLZ_ERR_ARG && has("x NULL"));
    CHECK(llz_tde_mc_process(h, one, hop, NULL, NULL, 8) == LLZ_ERR_ARG && has("delay NULL"));
    CHECK(llz_tde_mc_process(h, one, hop, out, NULL, 0) == LLZ_ERR_ARG && has("out_pitch 0"));
    CHECK(llz_tde_mc_frames_for(h, hop / 2) == LLZ_ERR_ARG && has("llz_tde_mc_frames_for"));
    CHECK(llz_tde_mc_read(h, 2, curve) == LLZ_ERR_ARG && has("what 2"));
    CHECK(llz_tde_mc_read(h, LLZ_TDE_STATE, NULL) == LLZ_ERR_ARG && has("NULL"));
    CHECK(llz_tde_mc_set_forget(h, 1.0f) == LLZ_ERR_ARG && has("llz_tde_mc_set_forget") && has("lam 1"));
    CHECK(llz_tde_mc_set_forget(h, -0.1f) == LLZ_ERR_ARG);
    CHECK(llz_tde_mc_frames(h) == at);
    CHECK(llz_tde_mc_reset(h) == LLZ_OK && llz_tde_mc_frames(h) == 0);
    CHECK(llz_tde_mc_read(h, LLZ_TDE_STATE, state) == LLZ_ERR_ARG && has("no frame yet"));
    CHECK(feed(h, channels, pairs, hop, N / hop, 1, 2, 1) == 1);
    CHECK(llz_tde_mc_read(h, LLZ_TDE_CURVE, curve) == LLZ_OK);
    free(curve); free(state);
    llz_tde_mc_uninit(h);
    printf("tde channels=%d pairs=%d fft_len=%d hop=%d ok\n", channels, pairs, N, hop);
    return 0;
}

int main(void)
{
    if (walk(1, 1, 64, 64, LLZ_TDE_CC) || walk(2, 3, 64, 16, LLZ_TDE_PHAT) || walk(3, 5, 128, 64, LLZ_TDE_SCOT) ||
        walk(5, 4, 256, 64, LLZ_TDE_PHAT) || walk(2, 2, 512, 512, LLZ_TDE_CC) || walk(7, 37, 1024, 256, LLZ_TDE_SCOT) ||
        walk(2, 1, 2048, 1024, LLZ_TDE_PHAT) || walk(3, 2, 4096, 1024, LLZ_TDE_PHAT))
        return 1;
    int t[4] = {0, 1, 1, 0};
#define INIT(ch, pr, tab, N, hop, win, L, wt, lo, hi, lam, dl) llz_tde_mc_init(ch, pr, tab, N, hop, win, L, wt, lo, hi, lam, dl)
    CHECK(INIT(0, 2, t, 256, 128, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("llz_tde_mc_init") && has("channels 0"));
    CHECK(INIT(2, 0, t, 256, 128, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("pairs 0"));
    CHECK(INIT(2, 2, NULL, 256, 128, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("llz_tde_mc_init"));
    CHECK(INIT(2, 2, t, 32, 16, HAMMING, 8, 1, 1, 15, 0.9f, 0.f) == BAD && has("fft_len 32"));
    CHECK(INIT(2, 2, t, 8192, 4096, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("fft_len 8192"));
    CHECK(INIT(2, 2, t, 256, 32, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("hop 32"));
    CHECK(INIT(1, 2, t, 256, 128, HAMMING, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("pair 0") && has("channel 1"));
    CHECK(INIT(2, 2, t, 256, 128, (win_t)9, 16, 1, 1, 127, 0.9f, 0.f) == BAD && has("unknown window 9"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 0, 1, 1, 127, 0.9f, 0.f) == BAD && has("max_lag 0"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 128, 1, 1, 127, 0.9f, 0.f) == BAD && has("max_lag 128"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 16, 3, 1, 127, 0.9f, 0.f) == BAD && has("weight 3"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 16, 1, 5, 4, 0.9f, 0.f) == BAD && has("k_lo 5"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 16, 1, 0, 129, 0.9f, 0.f) == BAD && has("k_hi 129"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 16, 1, 1, 127, 1.0f, 0.f) == BAD && has("lam 1"));
    CHECK(INIT(2, 2, t, 256, 128, HAMMING, 16, 1, 1, 127, 0.9f, -1.f) == BAD && has("delta -1"));
    float one[4] = {1, 0, 0, 0};
    const unsigned long bad[2] = {0, BAD};
    for (int i = 0; i < 2; i++) {
        CHECK(llz_tde_mc_process(bad[i], one, 4, one, NULL, 4) == LLZ_ERR_ARG && has("llz_tde_mc_process") && has("bad handle"));
        CHECK(llz_tde_mc_frames(bad[i]) == LLZ_ERR_ARG && has("llz_tde_mc_frames") && has("bad handle"));
        CHECK(llz_tde_mc_frames_for(bad[i], 4) == LLZ_ERR_ARG && has("llz_tde_mc_frames_for") && has("bad handle"));
        CHECK(llz_tde_mc_read(bad[i], 0, one) == LLZ_ERR_ARG && has("llz_tde_mc_read") && has("bad handle"));
        CHECK(llz_tde_mc_set_forget(bad[i], 0.5f) == LLZ_ERR_ARG && has("llz_tde_mc_set_forget"));
        CHECK(llz_tde_mc_reset(bad[i]) == LLZ_ERR_ARG && has("llz_tde_mc_reset"));
        CHECK(llz_tde_mc_set_stream(bad[i], NULL) == LLZ_ERR_ARG && has("llz_tde_mc_set_stream"));
        llz_tde_mc_uninit(bad[i]);
    }
    /* a handle of another kind fails the tag check */
    unsigned long other = llz_lpc_init(4);
    CHECK(other != BAD);
    CHECK(llz_tde_mc_process(other, one, 4, one, NULL, 4) == LLZ_ERR_ARG && has("llz_tde_mc_process") && has("bad handle"));
    llz_tde_mc_uninit(other);
    llz_lpc_uninit(other);
    printf("TDE_SANITIZE_OK\n");
    return 0;
}
