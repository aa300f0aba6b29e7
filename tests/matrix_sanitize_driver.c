/* The matrix convolver's host layer (llz_fir_matrix_host.c) under AddressSanitizer + UBSan with the device shim stubbed out (the
 * stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK without computing),
 * at (block, taps, inputs x outputs) = (64, 1, 2 x 2), (64, 65, 3 x 2), (512, 513, 2 x 3), (128, 131073, 1 x 2): init with both
 * tap types, calls that wrap the ring, set_taps of sub-matrices (the row chunks of the spectra upload and the slices of the
 * connection table), the connected-path count of plan, host-buffer staging, flush (in several passes where the scratch is
 * smaller than the flush), reset, and every refusal with its message. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)
#define SAYS(s) (strstr(llz_hip_last_error(), s) != NULL)

static unsigned g_seed = 13579u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23) + 1.5f;       /* never zero */
}

static int drive(int B, int T, int I, int O)
{
    enum { K = 2 };
    const int frame = K * B, keep = T - 1, P = (T + B - 1) / B;
    const size_t paths = (size_t)I * (size_t)O, span = (size_t)(keep > frame ? keep : frame);
    float *taps = malloc(sizeof(float) * paths * (size_t)T);
    double *taps64 = malloc(sizeof(double) * paths * (size_t)T);
    float *zeros = calloc(paths * (size_t)T, sizeof(float));
    float *x = calloc((size_t)I * (size_t)frame, sizeof(float)), *y = calloc((size_t)O * span + 1, sizeof(float));
    int plan[6] = {0, 0, 0, 0, 0, 0};
    CHECK(taps && taps64 && zeros && x && y);
    for (size_t i = 0; i < paths * (size_t)T; i++) taps64[i] = taps[i] = rnd();
    unsigned long h = llz_fir_matrix_mc_init(I, O, B, frame, taps, T);
    CHECK(h != BAD);
    CHECK(llz_fir_matrix_mc_flt_len(h) == T);
    CHECK(llz_fir_filter_mc_algo(h) < 0 && llz_fir_bank_mc_algo(h) < 0 && llz_fir_stream_mc_flt_len(h) < 0);   /* its own kind */
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[0] == 2 * B && plan[1] == P && plan[2] == P + K - 1 && plan[3] == K);
    CHECK(plan[4] >= 1 && plan[4] <= I && plan[5] == (int)paths);
    CHECK(llz_fir_matrix_mc_plan(h, NULL) < 0 && SAYS("llz_fir_matrix_mc_plan"));
    for (int c = 0; c < 2 * (P + K) && c < 40; c += K) CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);     /* the head wraps */
    CHECK(llz_fir_matrix_mc(h, x, y, frame - B) < 0 && SAYS("frame_len"));
    CHECK(llz_fir_matrix_mc(h, x, y, B + 1) < 0);
    CHECK(llz_fir_matrix_mc(h, x, x, frame) < 0 && SAYS("in-place"));
    CHECK(llz_fir_matrix_mc(h, NULL, y, frame) < 0 && llz_fir_matrix_mc(h, x, NULL, frame) < 0 && SAYS("llz_fir_matrix_mc"));
    /* the connection table: the last path, then a sub-matrix, then everything, off and on again */
    CHECK(llz_fir_matrix_mc_set_taps(h, O - 1, 1, I - 1, 1, zeros) == 0);
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == (int)paths - 1);
    CHECK(llz_fir_matrix_mc_set_taps(h, O - 1, 1, I - 1, 1, taps) == 0);
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == (int)paths);
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, O, 0, 1, zeros) == 0);          /* a column: a slice of one entry per output row */
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == (int)paths - O);
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, O, 0, I, zeros) == 0);
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == 0);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);                     /* nothing connected: still a call */
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, O, 0, I, taps) == 0);
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == (int)paths);
    /* ranges outside the matrix */
    CHECK(llz_fir_matrix_mc_set_taps(h, O, 1, 0, 1, taps) < 0 && SAYS("llz_fir_matrix_mc_set_taps") && SAYS("outputs"));
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, O + 1, 0, 1, taps) < 0 && SAYS("outputs"));
    CHECK(llz_fir_matrix_mc_set_taps(h, -1, 1, 0, 1, taps) < 0 && llz_fir_matrix_mc_set_taps(h, 0, 0, 0, 1, taps) < 0);
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, I, 1, taps) < 0 && SAYS("inputs"));
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, I - 1, 2, taps) < 0 && SAYS("inputs"));
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, -1, 1, taps) < 0 && llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 0, taps) < 0);
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 1, NULL) < 0 && SAYS("NULL taps"));
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == (int)paths);   /* a refusal changes nothing */
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    CHECK(llz_fir_matrix_mc_flush(h, y) == keep);
    CHECK(keep ? llz_fir_matrix_mc_flush(h, NULL) < 0 : llz_fir_matrix_mc_flush(h, NULL) == 0);   /* one tap: nothing to emit */
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);             /* reused after the flush */
    CHECK(llz_fir_matrix_mc_reset(h) == 0);
    CHECK(llz_fir_matrix_mc_set_stream(h, NULL) == 0);
    llz_fir_matrix_mc_uninit(h);
    /* double taps, one block per call */
    h = llz_fir_matrix_mc_init_f64taps(I, O, B, B, taps64, T);
    CHECK(h != BAD);
    CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[2] == P && plan[3] == 1 && plan[5] == (int)paths);
    CHECK(llz_fir_matrix_mc(h, x, y, B) == B);
    CHECK(llz_fir_matrix_mc_flush(h, y) == keep);
    llz_fir_matrix_mc_uninit(h);
    printf("matrix handle block=%d T=%d %dx%d ok\n", B, T, I, O);
    free(taps); free(taps64); free(zeros); free(x); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][4] = {{64, 1, 2, 2}, {64, 65, 3, 2}, {512, 513, 2, 3}, {128, 131073, 1, 2}};
    for (int i = 0; i < 4; i++)
        if (drive(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3])) return 1;
    {   /* a flush longer than the 64 MiB of partial spectra hold: 16 -> 8 at block 4096 runs in 16 groups, 4 MiB of partials a
         * block, so the 20 blocks behind 81921 taps go in passes of 16 and 4; then an output row of more paths than one staging
         * chunk of spectra (8 MiB: 7 paths at 131073 taps) */
        const int Tl = 131073, Tm = 81921;
        float *taps = calloc((size_t)16 * 8 * Tm, sizeof(float)), *y = calloc((size_t)8 * (size_t)(Tl - 1), sizeof(float));
        int plan[6];
        CHECK(taps && y);
        unsigned long h = llz_fir_matrix_mc_init(16, 8, 4096, 4096, taps, Tm);
        CHECK(h != BAD);
        CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[4] == 16 && plan[5] == 0);
        CHECK(llz_fir_matrix_mc_flush(h, y) == Tm - 1);
        llz_fir_matrix_mc_uninit(h);
        free(taps);
        taps = calloc((size_t)9 * 2 * Tl, sizeof(float));
        CHECK(taps);
        taps[5] = 1.0f;                                             /* path (0, 0) alone is connected */
        h = llz_fir_matrix_mc_init(9, 2, 4096, 4096, taps, Tl);
        CHECK(h != BAD);
        CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == 1 && plan[4] == 9);
        CHECK(llz_fir_matrix_mc_set_taps(h, 1, 1, 1, 8, taps) == 0);
        CHECK(llz_fir_matrix_mc_plan(h, plan) == 0 && plan[5] == 2);
        CHECK(llz_fir_matrix_mc_flush(h, y) == Tl - 1);
        llz_fir_matrix_mc_uninit(h);
        free(y);
        /* refusals: each names the init and its range */
        CHECK(llz_fir_matrix_mc_init(0, 2, 64, 64, taps, 63) == BAD && SAYS("llz_fir_matrix_mc_init") && SAYS("inputs") && SAYS("1..4096"));
        CHECK(llz_fir_matrix_mc_init(4097, 2, 64, 64, taps, 63) == BAD && SAYS("inputs"));
        CHECK(llz_fir_matrix_mc_init(2, 0, 64, 64, taps, 63) == BAD && SAYS("outputs") && SAYS("1..4096"));
        CHECK(llz_fir_matrix_mc_init(2, 4097, 64, 64, taps, 63) == BAD && SAYS("outputs"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 96, 96, taps, 63) == BAD && SAYS("64..4096"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 100, taps, 63) == BAD && SAYS("frame_len"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 0, taps, 63) == BAD && SAYS("frame_len"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 64 * 65536, taps, 63) == BAD && SAYS("1..65535"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 64, taps, Tl + 1) == BAD && SAYS("1..131073"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 64, taps, 0) == BAD && SAYS("flt_len"));
        CHECK(llz_fir_matrix_mc_init(2, 2, 64, 64, NULL, 63) == BAD && SAYS("no taps"));
        CHECK(llz_fir_matrix_mc_init_f64taps(2, 2, 64, 64, NULL, 63) == BAD && SAYS("llz_fir_matrix_mc_init_f64taps"));
        /* handles of the other forms are not matrix handles, and bad handles are refused */
        h = llz_fir_stream_mc_init(2, 64, 64, taps, 1, 130);
        CHECK(h != BAD);
        CHECK(llz_fir_matrix_mc_plan(h, plan) < 0 && llz_fir_matrix_mc_reset(h) < 0 && llz_fir_matrix_mc_flt_len(h) < 0);
        CHECK(llz_fir_matrix_mc_flush(h, (float *)plan) < 0 && llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 1, taps) < 0);
        CHECK(llz_fir_matrix_mc(h, taps, (float *)plan, 64) < 0 && llz_fir_matrix_mc_set_stream(h, NULL) < 0);
        llz_fir_matrix_mc_uninit(h);                                /* not its handle: left alone */
        CHECK(llz_fir_stream_mc_flt_len(h) == 130);
        llz_fir_stream_mc_uninit(h);
        CHECK(llz_fir_matrix_mc_plan(0, plan) < 0 && llz_fir_matrix_mc_plan(BAD, plan) < 0);
        CHECK(llz_fir_matrix_mc_reset(0) < 0 && SAYS("llz_fir_matrix_mc_reset"));
        llz_fir_matrix_mc_uninit(0);
        llz_fir_matrix_mc_uninit(BAD);
        free(taps);
    }
    printf("MATRIX_SANITIZE_OK\n");
    return 0;
}
