/* The stream convolver's crossfade (llz_fir_xfade_stream_mc, llz_fir_stream_host.c) under AddressSanitizer + UBSan with the device
 * shim stubbed out (the stub of tests/test_host_sanitizers.py: device memory is calloc of the exact size, copies are memcpy,
 * kernels return LLZ_OK without computing), at (block, taps) = (64, 1), (64, 65), (512, 513), (128, 131073): the second spectra
 * buffer and the row table, a fade across several calls with k = 1 and k = 3, a fade whose end falls inside a call, rows
 * added to a pending fade, the adoption by row copies and by swap, every refusal with its message, set_taps refused mid-fade,
 * reset and flush mid-fade, a second fade after the first, uninit with a fade in flight.  llz_fir_xfade_stream_mc_left is
 * checked after every step. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_fir.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)
#define LEFT(h, n) CHECK(llz_fir_xfade_stream_mc_left(h) == (n))
#define SAYS(s) (strstr(llz_hip_last_error(), "llz_fir_xfade_stream_mc") && strstr(llz_hip_last_error(), s))

static unsigned g_seed = 13579u;
static float rnd(void)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int)(g_seed >> 8) - (1 << 23)) / (float)(1 << 23);
}

/* a bank of CH rows in calls of k blocks */
static int drive_bank(int B, int T, int k)
{
    enum { CH = 5 };
    const int frame = k * B, keep = T - 1, span = keep > frame ? keep : frame;
    float *taps = malloc(sizeof(float) * CH * (size_t)T);
    float *x = calloc((size_t)CH * (size_t)frame, sizeof(float)), *y = calloc((size_t)CH * (size_t)span + 1, sizeof(float));
    CHECK(taps && x && y);
    for (size_t i = 0; i < CH * (size_t)T; i++) taps[i] = rnd();
    unsigned long h = llz_fir_stream_mc_init(CH, B, frame, taps, CH, T);
    CHECK(h != BAD);
    LEFT(h, 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, 0);
    /* the refusals, each with its own message; none of them starts a fade */
    CHECK(llz_fir_xfade_stream_mc(0, 0, 1, taps, 4) < 0 && SAYS("bad handle"));
    CHECK(llz_fir_xfade_stream_mc(BAD, 0, 1, taps, 4) < 0 && SAYS("bad handle"));
    CHECK(llz_fir_xfade_stream_mc(h, 0, 1, NULL, 4) < 0 && SAYS("no taps"));
    CHECK(llz_fir_xfade_stream_mc(h, 4, 2, taps, 4) < 0 && SAYS("outside the handle's"));
    CHECK(llz_fir_xfade_stream_mc(h, -1, 1, taps, 4) < 0 && SAYS("outside the handle's"));
    CHECK(llz_fir_xfade_stream_mc(h, 0, 0, taps, 4) < 0 && SAYS("outside the handle's"));
    CHECK(llz_fir_xfade_stream_mc(h, 0, 1, taps, 0) < 0 && SAYS("1..4096"));
    CHECK(llz_fir_xfade_stream_mc(h, 0, 1, taps, 4097) < 0 && SAYS("1..4096"));
    CHECK(llz_fir_xfade_stream_mc_left(0) < 0 && llz_fir_xfade_stream_mc_left(BAD) < 0);
    LEFT(h, 0);
    /* rows 1 and 4 join one pending fade of 7 blocks: rows that are not neighbours */
    CHECK(llz_fir_xfade_stream_mc(h, 1, 1, taps, 7) == 0);
    LEFT(h, 7);
    CHECK(llz_fir_xfade_stream_mc(h, 4, 1, taps, 7) == 0);          /* the last row of the table */
    CHECK(llz_fir_xfade_stream_mc(h, 1, 1, taps + T, 7) == 0);      /* replaces a row of the pending fade */
    LEFT(h, 7);
    CHECK(llz_fir_xfade_stream_mc(h, 2, 1, taps, 6) < 0 && SAYS("in flight") && SAYS("same fade_blocks"));
    LEFT(h, 7);
    CHECK(llz_fir_stream_mc_set_taps(h, 0, 1, taps) < 0 && strstr(llz_hip_last_error(), "llz_fir_stream_mc_set_taps") &&
          strstr(llz_hip_last_error(), "7 of its 7 blocks left"));
    /* across calls; with k = 3 the end (block 7) falls inside the third call */
    for (int done = k; done < 7; done += k) {
        CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
        LEFT(h, 7 - done);
        CHECK(llz_fir_xfade_stream_mc(h, 2, 1, taps, 7) < 0 && SAYS("in flight"));
        CHECK(llz_fir_stream_mc_set_taps(h, 0, CH, taps) < 0 && strstr(llz_hip_last_error(), "in flight"));
    }
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);              /* the fade's last blocks: rows 1 and 4 copied into the table */
    LEFT(h, 0);
    CHECK(llz_fir_stream_mc_set_taps(h, 0, CH, taps) == 0);          /* accepted again */
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    /* a second fade, of every row: adopted by swapping the buffers; it ends inside its first call when k = 3 */
    CHECK(llz_fir_xfade_stream_mc(h, 0, CH, taps, 2) == 0);
    LEFT(h, 2);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, k >= 2 ? 0 : 1);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, 0);
    /* reset mid-fade adopts at once */
    CHECK(llz_fir_xfade_stream_mc(h, 2, 3, taps, 4000) == 0);       /* rows 2 .. 4 of the swapped buffers */
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, 4000 - k);
    CHECK(llz_fir_stream_mc_reset(h) == 0);
    LEFT(h, 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    /* flush mid-fade: the ramp goes on through the zero blocks, then the handle is reset with the new taps */
    CHECK(llz_fir_xfade_stream_mc(h, 0, 2, taps, 4096) == 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, 4096 - k);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    LEFT(h, 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    /* flush of a PENDING fade of one block: the flush's blocks past it are new-taps blocks */
    CHECK(llz_fir_xfade_stream_mc(h, 3, 1, taps, 1) == 0);
    LEFT(h, 1);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    LEFT(h, 0);
    /* uninit with a fade in flight */
    CHECK(llz_fir_xfade_stream_mc(h, 0, CH, taps, 9) == 0);
    CHECK(llz_fir_stream_mc(h, x, y, frame) == frame);
    LEFT(h, 9 - k);
    llz_fir_stream_mc_uninit(h);
    free(taps); free(x); free(y);
    return 0;
}

/* one tap set for all channels: one row, the fade always swaps */
static int drive_shared(int B, int T)
{
    enum { CH = 3 };
    const int keep = T - 1, span = keep > B ? keep : B;
    float *taps = malloc(sizeof(float) * 2 * (size_t)T);
    float *x = calloc((size_t)CH * (size_t)B, sizeof(float)), *y = calloc((size_t)CH * (size_t)span + 1, sizeof(float));
    CHECK(taps && x && y);
    for (size_t i = 0; i < 2 * (size_t)T; i++) taps[i] = rnd();
    unsigned long h = llz_fir_stream_mc_init(CH, B, B, taps, 1, T);
    CHECK(h != BAD);
    CHECK(llz_fir_xfade_stream_mc(h, 1, 1, taps, 3) < 0 && SAYS("only first 0, count 1"));
    CHECK(llz_fir_xfade_stream_mc(h, 0, CH, taps, 3) < 0 && SAYS("outside the handle's"));
    LEFT(h, 0);
    CHECK(llz_fir_xfade_stream_mc(h, 0, 1, taps + T, 3) == 0);
    for (int j = 1; j <= 3; j++) {
        LEFT(h, 4 - j);
        CHECK(llz_fir_stream_mc(h, x, y, B) == B);
    }
    LEFT(h, 0);
    CHECK(llz_fir_xfade_stream_mc(h, 0, 1, taps, 2) == 0);           /* back again, through the swapped buffers */
    CHECK(llz_fir_stream_mc(h, x, y, B) == B);
    LEFT(h, 1);
    CHECK(llz_fir_stream_mc_flush(h, y) == keep);
    LEFT(h, 0);
    llz_fir_stream_mc_uninit(h);
    h = llz_fir_stream_mc_init(CH, B, B, taps, 1, T);                 /* a handle that never fades frees nothing it has not got */
    CHECK(h != BAD);
    LEFT(h, 0);
    llz_fir_stream_mc_uninit(h);
    free(taps); free(x); free(y);
    return 0;
}

int main(void)
{
    const int shapes[4][2] = {{64, 1}, {64, 65}, {512, 513}, {128, 131073}};
    for (int i = 0; i < 4; i++) {
        if (drive_bank(shapes[i][0], shapes[i][1], 1)) return 1;
        if (drive_bank(shapes[i][0], shapes[i][1], 3)) return 1;
        if (drive_shared(shapes[i][0], shapes[i][1])) return 1;
        printf("fade block=%d T=%d : k = 1, k = 3 and the shared handle done\n", shapes[i][0], shapes[i][1]);
    }
    printf("FADE_SANITIZE_OK\n");
    return 0;
}
