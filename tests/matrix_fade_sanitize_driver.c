/* The matrix convolver's crossfade (llz_fir_xfade_matrix_mc, llz_fir_matrix_host.c) under AddressSanitizer + UBSan with the device
 * shim stubbed out (the stub of tests/test_host_sanitizers.py: device memory is calloc of the exact size, copies are memcpy,
 * kernels return LLZ_OK without computing), at (block, taps, inputs x outputs) = (64, 1, 2 x 2), (64, 65, 3 x 2), (512, 513, 2 x
 * 3), (128, 131073, 1 x 2): the second spectra buffer, the second scratch and the three tables, a fade across several calls with
 * k = 1 and k = 3, a fade whose end falls inside a call, paths joining and replacing paths of a pending fade, the adoption by
 * copies of runs and by swap, the connection table following the new taps (a path fading out, a path fading in), every refusal
 * with its message, set_taps refused mid-fade, reset and flush mid-fade, the flush of a pending fade, a second fade after the
 * first, uninit with a fade pending and in flight.  llz_fir_xfade_matrix_mc_left and plan()[5] are checked after every step. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)
#define XF llz_fir_xfade_matrix_mc
#define SAYS(s) (strstr(llz_hip_last_error(), "llz_fir_xfade_matrix_mc") && strstr(llz_hip_last_error(), s))
/* the blocks left and the connected paths */
#define STATE(h, left, conn) do { int pl_[6]; CHECK(llz_fir_xfade_matrix_mc_left(h) == (left)); \
                                  CHECK(llz_fir_matrix_mc_plan(h, pl_) == 0 && pl_[5] == (conn)); } while (0)

static unsigned g_seed = 24680u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23) + 1.5f;       /* never zero */
}

static int drive(int B, int T, int I, int O, int k)
{
    const int frame = k * B, keep = T - 1, paths = I * O;
    const size_t span = (size_t)(keep > frame ? keep : frame);
    float *taps = malloc(sizeof(float) * (size_t)paths * (size_t)T);
    float *zeros = calloc((size_t)paths * (size_t)T, sizeof(float));
    float *x = calloc((size_t)I * (size_t)frame, sizeof(float)), *y = calloc((size_t)O * span + 1, sizeof(float));
    CHECK(taps && zeros && x && y);
    for (size_t i = 0; i < (size_t)paths * (size_t)T; i++) taps[i] = rnd();
    unsigned long h = llz_fir_matrix_mc_init(I, O, B, frame, taps, T);
    CHECK(h != BAD);
    STATE(h, 0, paths);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    /* the refusals, each with its own message; none of them starts a fade or allocates for one */
    CHECK(XF(0, 0, 1, 0, 1, taps, 4) < 0 && SAYS("bad handle"));
    CHECK(XF(BAD, 0, 1, 0, 1, taps, 4) < 0 && SAYS("bad handle"));
    CHECK(XF(h, 0, 1, 0, 1, NULL, 4) < 0 && SAYS("no taps"));
    CHECK(XF(h, O, 1, 0, 1, taps, 4) < 0 && SAYS("outputs [") && SAYS("outside the handle's"));
    CHECK(XF(h, 0, O + 1, 0, 1, taps, 4) < 0 && SAYS("outputs ["));
    CHECK(XF(h, -1, 1, 0, 1, taps, 4) < 0 && SAYS("outputs [") && XF(h, 0, 0, 0, 1, taps, 4) < 0 && SAYS("outputs ["));
    CHECK(XF(h, 0, 1, I, 1, taps, 4) < 0 && SAYS("inputs [") && SAYS("outside the handle's"));
    CHECK(XF(h, 0, 1, I - 1, 2, taps, 4) < 0 && SAYS("inputs ["));
    CHECK(XF(h, 0, 1, -1, 1, taps, 4) < 0 && SAYS("inputs [") && XF(h, 0, 1, 0, 0, taps, 4) < 0 && SAYS("inputs ["));
    CHECK(XF(h, 0, 1, 0, 1, taps, 0) < 0 && SAYS("1..4096"));
    CHECK(XF(h, 0, 1, 0, 1, taps, 4097) < 0 && SAYS("1..4096"));
    CHECK(llz_fir_xfade_matrix_mc_left(0) < 0 && llz_fir_xfade_matrix_mc_left(BAD) < 0);
    STATE(h, 0, paths);
    /* the last column of every output, then the lone path (O - 1, 0) fading OUT to zero taps (with one input: a path of that
     * column, replaced), join one pending fade of 7 blocks */
    CHECK(XF(h, 0, O, I - 1, 1, taps, 7) == 0);
    STATE(h, 7, paths);
    CHECK(XF(h, O - 1, 1, 0, 1, zeros, 7) == 0);
    CHECK(XF(h, 0, 1, I - 1, 1, taps + T, 7) == 0);                 /* replaces a path of the pending fade */
    STATE(h, 7, paths);                                             /* the union: the path fading out still feeds the old sum */
    CHECK(XF(h, 0, 1, 0, 1, taps, 6) < 0 && SAYS("in flight") && SAYS("same fade_blocks"));
    STATE(h, 7, paths);
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 1, taps) < 0 && strstr(llz_hip_last_error(), "llz_fir_matrix_mc_set_taps") &&
          strstr(llz_hip_last_error(), "7 of its 7 blocks left"));
    /* across calls; with k = 3 the end (block 7) falls inside the third call */
    for (int done = k; done < 7; done += k) {
        CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
        STATE(h, 7 - done, paths);
        CHECK(XF(h, 0, 1, 0, 1, taps, 7) < 0 && SAYS("in flight") && !SAYS("same fade_blocks"));
        CHECK(llz_fir_matrix_mc_set_taps(h, 0, O, 0, I, taps) < 0 && strstr(llz_hip_last_error(), "in flight"));
    }
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);              /* the fade's last blocks: the runs of faded paths copied */
    STATE(h, 0, paths - 1);                                         /* faded out: unconnected */
    CHECK(llz_fir_matrix_mc_set_taps(h, O - 1, 1, 0, 1, taps) == 0); /* accepted again */
    STATE(h, 0, paths);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    /* a second fade, of every path: adopted by swapping the buffers; it ends inside its first call when k = 3 */
    CHECK(XF(h, 0, O, 0, I, taps, 2) == 0);
    STATE(h, 2, paths);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    STATE(h, k >= 2 ? 0 : 1, paths);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    STATE(h, 0, paths);
    /* a path fading IN from zero taps; reset mid-fade adopts at once */
    CHECK(llz_fir_matrix_mc_set_taps(h, 0, 1, 0, 1, zeros) == 0);
    STATE(h, 0, paths - 1);
    CHECK(XF(h, 0, 1, 0, 1, taps, 4000) == 0);
    STATE(h, 4000, paths);                                          /* the union */
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    STATE(h, 4000 - k, paths);
    CHECK(llz_fir_matrix_mc_reset(h) == 0);
    STATE(h, 0, paths);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    /* flush mid-fade: the ramp goes on through the zero blocks, then the handle is reset with the new taps: column 0 gone */
    CHECK(XF(h, 0, O, 0, 1, zeros, 4096) == 0);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    STATE(h, 4096 - k, paths);
    CHECK(llz_fir_matrix_mc_flush(h, y) == keep);
    STATE(h, 0, paths - O);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    /* flush of a PENDING fade of one block: the flush's blocks past it are new-taps blocks */
    CHECK(XF(h, 0, 1, 0, 1, taps, 1) == 0);
    STATE(h, 1, paths - O + 1);
    CHECK(llz_fir_matrix_mc_flush(h, y) == keep);
    STATE(h, 0, paths - O + 1);
    /* uninit with a fade in flight */
    CHECK(XF(h, 0, O, 0, I, taps, 9) == 0);
    CHECK(llz_fir_matrix_mc(h, x, y, frame) == frame);
    STATE(h, 9 - k, paths);
    llz_fir_matrix_mc_uninit(h);
    /* uninit with a fade pending; and a handle that never fades frees nothing it has not got */
    h = llz_fir_matrix_mc_init(I, O, B, frame, taps, T);
    CHECK(h != BAD);
    CHECK(XF(h, O - 1, 1, I - 1, 1, zeros, 3) == 0);
    STATE(h, 3, paths);
    llz_fir_matrix_mc_uninit(h);
    h = llz_fir_matrix_mc_init(I, O, B, frame, taps, T);
    CHECK(h != BAD);
    STATE(h, 0, paths);
    llz_fir_matrix_mc_uninit(h);
    free(taps); free(zeros); free(x); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][4] = {{64, 1, 2, 2}, {64, 65, 3, 2}, {512, 513, 2, 3}, {128, 131073, 1, 2}};
    for (int i = 0; i < 4; i++) {
        if (drive(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], 1)) return 1;
        if (drive(shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3], 3)) return 1;
        printf("matrix fade block=%d T=%d %dx%d : k = 1 and k = 3 done\n", shapes[i][0], shapes[i][1], shapes[i][2], shapes[i][3]);
    }
    {   /* a flush in passes while a fade runs: 16 -> 8 at block 4096, 81921 taps, the 20 blocks in passes of 16 and 4 */
        const int Tm = 81921;
        float *taps = calloc((size_t)16 * 8 * Tm, sizeof(float)), *y = calloc((size_t)8 * (size_t)(Tm - 1), sizeof(float));
        float *x = calloc((size_t)16 * 4096, sizeof(float));
        CHECK(taps && y && x);
        for (int q = 0; q < 16 * 8; q++) taps[(size_t)q * Tm] = 1.0f;
        unsigned long h = llz_fir_matrix_mc_init(16, 8, 4096, 4096, taps, Tm);
        CHECK(h != BAD);
        CHECK(XF(h, 0, 8, 15, 1, taps, 24) == 0);
        CHECK(llz_fir_matrix_mc(h, x, y, 4096) == 4096);
        STATE(h, 23, 128);
        CHECK(llz_fir_matrix_mc_flush(h, y) == Tm - 1);
        STATE(h, 0, 128);
        llz_fir_matrix_mc_uninit(h);
        free(taps); free(y); free(x);
    }
    printf("MATRIX_FADE_SANITIZE_OK\n");
    return 0;
}
