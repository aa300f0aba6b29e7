/* The Welch cross-spectra's host layer (llz_spectral_host.c) under AddressSanitizer + UBSan with the device shim stubbed out
 * (the stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without
 * computing): init at every size and hop, updates that start, continue and end runs with host buffers of exactly the documented
 * sizes (a staging copy one element too long is a heap overflow), the frame count and the plan after each, every read-out into
 * exact buffers, reset, set_stream, a handle whose partials exceed the scratch cap (several slab walks), every refusal with its
 * message, uninit. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_lpc.h"
#include "llz_spectral.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static int has(const char *needle) { return strstr(llz_hip_last_error(), needle) != NULL; }

static long frames_after(long hops, int N, int hop)
{
    const long lead = N / hop - 1;
    return hops > lead ? hops - lead : 0;
}

static int feed(unsigned long h, int channels, int hop, long hops_in_call)
{
    const size_t n = (size_t)hops_in_call * hop;
    float *x = malloc(sizeof(float) * channels * n);
    if (!x) return -100;
    for (size_t j = 0; j < channels * n; j++) x[j] = (float)(j % 17) - 8.0f;
    const long got = llz_csd_mc_update(h, x, (long)n);
    free(x);
    return (int)got;
}

static int walk(int channels, int pairs, int N, int hop)
{
    int *table = malloc(sizeof(int) * 2 * pairs);
    CHECK(table);
    for (int p = 0; p < 2 * pairs; p++) table[p] = (p * 7 + p / 2) % channels;
    unsigned long h = llz_csd_mc_init(channels, pairs, table, N, hop, (win_t)(N / 64 % 3));
    free(table);                                                    /* the handle keeps its own copy */
    CHECK(h != BAD && h != 0);
    const int bins = N / 2 + 1;
    float *out = malloc(sizeof(float) * 2 * pairs * bins);
    double *raw = malloc(sizeof(double) * 4 * pairs * bins);
    CHECK(out && raw);
    CHECK(llz_csd_mc_frames(h) == 0);
    CHECK(llz_csd_mc_read(h, LLZ_SPEC_PXX, out) == LLZ_ERR_ARG && has("llz_csd_mc_read") && has("no frame yet"));
    CHECK(llz_csd_mc_read_raw(h, raw) == LLZ_ERR_ARG && has("llz_csd_mc_read_raw") && has("no frame yet"));
    /* one hop at a time up to the first frames, then a call that ends mid-run, one that continues and ends the run and starts
     * the next, one that spans whole runs */
    const long calls[] = {1, 1, 1, 1, 20, 15, 2 * LLZ_CSD_RUN + 5, 1};
    long hops = 0;
    for (unsigned i = 0; i < sizeof(calls) / sizeof(calls[0]); i++) {
        int plan[4];
        CHECK(llz_csd_mc_plan(h, calls[i] * hop, plan) == LLZ_OK);
        const long lo = frames_after(hops, N, hop), hi = frames_after(hops + calls[i], N, hop);
        const long runs = hi > lo ? (hi - 1) / LLZ_CSD_RUN - lo / LLZ_CSD_RUN + 1 : 0;
        CHECK((plan[0] == 0 || plan[0] == 1) && plan[1] == LLZ_CSD_RUN && plan[2] == runs && plan[3] == (runs ? 1 : 0));
        hops += calls[i];
        CHECK(feed(h, channels, hop, calls[i]) == hi);
        CHECK(llz_csd_mc_frames(h) == hi);
        if (hi > 0) {
            for (int what = LLZ_SPEC_PXX; what <= LLZ_SPEC_TF; what++) CHECK(llz_csd_mc_read(h, what, out) == LLZ_OK);
            CHECK(llz_csd_mc_read_raw(h, raw) == LLZ_OK);
        }
        if (i == 5) CHECK(llz_csd_mc_set_stream(h, NULL) == LLZ_OK);
    }
    /* refusals on a live handle */
    float one[8] = {0};
    CHECK(llz_csd_mc_update(h, one, hop + 1) == LLZ_ERR_ARG && has("llz_csd_mc_update") && has("multiple of hop"));
    CHECK(llz_csd_mc_update(h, one, 0) == LLZ_ERR_ARG && has("llz_csd_mc_update"));
    CHECK(llz_csd_mc_update(h, NULL, hop) == LLZ_ERR_ARG && has("llz_csd_mc_update") && has("NULL"));
    CHECK(llz_csd_mc_read(h, 5, out) == LLZ_ERR_ARG && has("llz_csd_mc_read") && has("what 5"));
    CHECK(llz_csd_mc_read(h, LLZ_SPEC_TF, NULL) == LLZ_ERR_ARG && has("NULL"));
    CHECK(llz_csd_mc_plan(h, hop, NULL) == LLZ_ERR_ARG && has("llz_csd_mc_plan"));
    CHECK(llz_csd_mc_plan(h, hop / 2, (int[4]){0}) == LLZ_ERR_ARG && has("llz_csd_mc_plan"));
    CHECK(llz_csd_mc_reset(h) == LLZ_OK && llz_csd_mc_frames(h) == 0);
    CHECK(llz_csd_mc_read(h, LLZ_SPEC_CSD, out) == LLZ_ERR_ARG && has("no frame yet"));
    CHECK(feed(h, channels, hop, N / hop) == 1);
    CHECK(llz_csd_mc_read(h, LLZ_SPEC_COHERENCE, out) == LLZ_OK);
    free(out); free(raw);
    llz_csd_mc_uninit(h);
    printf("csd channels=%d pairs=%d fft_len=%d hop=%d ok\n", channels, pairs, N, hop);
    return 0;
}

/* partials beyond the scratch cap (256 MiB): 2100 pairs of 2049 bins are 65.7 MiB a run, three runs a walk */
static int slabs(void)
{
    const int pairs = 2100, N = 4096;
    int *table = calloc(2 * (size_t)pairs, sizeof(int));
    CHECK(table);
    unsigned long h = llz_csd_mc_init(1, pairs, table, N, N, HAMMING);
    free(table);
    CHECK(h != BAD);
    int plan[4];
    CHECK(llz_csd_mc_plan(h, (long)N * (6 * LLZ_CSD_RUN + 7), plan) == LLZ_OK);
    CHECK(plan[2] == 3 && plan[3] == 3);                            /* seven runs: 3 + 3 + 1 */
    CHECK(feed(h, 1, N, 5) == 5);                                   /* one walk that ends mid-run */
    CHECK(llz_csd_mc_plan(h, (long)N * (3 * LLZ_CSD_RUN), plan) == LLZ_OK && plan[2] == 3 && plan[3] == 2);
    CHECK(feed(h, 1, N, 3 * LLZ_CSD_RUN) == 3 * LLZ_CSD_RUN + 5);   /* continues the run, two walks, ends mid-run again */
    double *raw = malloc(sizeof(double) * 4 * (size_t)pairs * (N / 2 + 1));
    CHECK(raw && llz_csd_mc_read_raw(h, raw) == LLZ_OK);
    free(raw);
    llz_csd_mc_uninit(h);
    printf("csd slabs ok\n");
    return 0;
}

int main(void)
{
    if (walk(1, 1, 64, 64) || walk(2, 3, 64, 16) || walk(3, 5, 128, 64) || walk(5, 4, 256, 64) || walk(2, 2, 512, 512) ||
        walk(7, 9, 1024, 256) || walk(2, 1, 2048, 1024) || walk(3, 2, 4096, 1024) || slabs())
        return 1;
    int t[4] = {0, 1, 1, 0};
    CHECK(llz_csd_mc_init(0, 2, t, 256, 128, HAMMING) == BAD && has("llz_csd_mc_init") && has("channels 0"));
    CHECK(llz_csd_mc_init(2, 0, t, 256, 128, HAMMING) == BAD && has("pairs 0"));
    CHECK(llz_csd_mc_init(2, 2, NULL, 256, 128, HAMMING) == BAD && has("llz_csd_mc_init"));
    CHECK(llz_csd_mc_init(2, 2, t, 32, 16, HAMMING) == BAD && has("fft_len 32"));
    CHECK(llz_csd_mc_init(2, 2, t, 8192, 4096, HAMMING) == BAD && has("fft_len 8192"));
    CHECK(llz_csd_mc_init(2, 2, t, 384, 96, HAMMING) == BAD && has("fft_len 384"));
    CHECK(llz_csd_mc_init(2, 2, t, 256, 32, HAMMING) == BAD && has("hop 32"));
    CHECK(llz_csd_mc_init(2, 2, t, 256, 0, HAMMING) == BAD && has("hop 0"));
    CHECK(llz_csd_mc_init(1, 2, t, 256, 128, HAMMING) == BAD && has("pair 0") && has("channel 1"));
    t[3] = -1;
    CHECK(llz_csd_mc_init(2, 2, t, 256, 128, HAMMING) == BAD && has("pair 1") && has("channel -1"));
    t[3] = 0;
    CHECK(llz_csd_mc_init(2, 2, t, 256, 128, (win_t)9) == BAD && has("unknown window 9"));
    float one[4] = {1, 0, 0, 0};
    double oned[4] = {0};
    int plan[4];
    const unsigned long bad[2] = {0, BAD};
    for (int i = 0; i < 2; i++) {
        CHECK(llz_csd_mc_update(bad[i], one, 4) == LLZ_ERR_ARG && has("llz_csd_mc_update") && has("bad handle"));
        CHECK(llz_csd_mc_frames(bad[i]) == LLZ_ERR_ARG && has("llz_csd_mc_frames") && has("bad handle"));
        CHECK(llz_csd_mc_read(bad[i], 0, one) == LLZ_ERR_ARG && has("llz_csd_mc_read") && has("bad handle"));
        CHECK(llz_csd_mc_read_raw(bad[i], oned) == LLZ_ERR_ARG && has("llz_csd_mc_read_raw") && has("bad handle"));
        CHECK(llz_csd_mc_reset(bad[i]) == LLZ_ERR_ARG && has("llz_csd_mc_reset"));
        CHECK(llz_csd_mc_plan(bad[i], 4, plan) == LLZ_ERR_ARG && has("llz_csd_mc_plan"));
        CHECK(llz_csd_mc_set_stream(bad[i], NULL) == LLZ_ERR_ARG && has("llz_csd_mc_set_stream"));
        llz_csd_mc_uninit(bad[i]);
    }
    /* a handle of another kind fails the tag check */
    unsigned long other = llz_lpc_init(4);
    CHECK(other != BAD);
    CHECK(llz_csd_mc_update(other, one, 4) == LLZ_ERR_ARG && has("bad handle"));
    llz_csd_mc_uninit(other);
    llz_lpc_uninit(other);
    printf("CSD_SANITIZE_OK\n");
    return 0;
}
