/* The host layer of the DFT of any length and the zoom transform (llz_dft_host.c) under AddressSanitizer + UBSan with the device
 * shim stubbed out (the stub of tests/test_host_sanitizers.py: device memory is malloc, copies are memcpy, kernels return LLZ_OK
 * without computing): init at lengths on both sides of the form threshold and of the large transforms, both table orders,
 * set_window, plan, every entry point on host buffers of exactly the documented sizes (a staging copy one element too long is a
 * heap overflow) with overlapping input rows and gaps between output rows that must come back as they were, configure to the
 * composed form and back with the window kept, a composed call that walks two slabs under the scratch cap, every refusal with its message and the handle alive behind it, uninit. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_lpc.h"
#include "llz_dft.h"

#define BAD ((unsigned long)-1)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "driver: %s failed at line %d (%s)\n", #c, __LINE__, llz_hip_last_error()); return 1; } } while (0)

static int has(const char *needle) { return strstr(llz_hip_last_error(), needle) != NULL; }

typedef int (*dft_fn)(unsigned long, const float *, long, float *, long, int);

/* one call on exact host buffers: in_el / out_el floats per element, rows in_pitch / out_pitch apart; the gaps keep their fill */
static int call(dft_fn fn, unsigned long h, int in_len, int in_el, long in_pitch, int out_len, int out_el, long out_pitch, int count)
{
    const size_t in_n = (size_t)in_el * ((size_t)(count - 1) * in_pitch + in_len);
    const size_t out_n = (size_t)out_el * ((size_t)(count - 1) * out_pitch + out_len);
    float *in = malloc(sizeof(float) * in_n), *out = malloc(sizeof(float) * out_n);
    if (!in || !out) return -100;
    for (size_t j = 0; j < in_n; j++) in[j] = (float)(j % 13) - 6.0f;
    for (size_t j = 0; j < out_n; j++) out[j] = 77.0f;
    int rc = fn(h, in, in_pitch, out, out_pitch, count);
    for (int r = 0; r + 1 < count && rc == LLZ_OK; r++)
        for (size_t j = (size_t)out_el * out_len; j < (size_t)out_el * out_pitch; j++)
            if (out[(size_t)out_el * r * out_pitch + j] != 77.0f) rc = -200;
    free(in); free(out);
    return rc;
}

static int walk_dft(int n, int expect_form, int expect_m)
{
    unsigned long h = llz_dft_mc_init(n);
    CHECK(h != BAD && h != 0);
    const int half = n / 2 + 1;
    int plan[5] = {-1, -1, -1, -1, -1};
    CHECK(llz_dft_mc_plan(h, 37, plan) == LLZ_OK && plan[0] == expect_form && plan[1] == expect_m && plan[4] == 1);
    float *w = malloc(sizeof(float) * n);
    CHECK(w);
    for (int i = 0; i < n; i++) w[i] = 0.5f + (float)(i % 7) / 16.0f;
    CHECK(llz_dft_mc_set_window(h, w) == LLZ_OK && llz_dft_mc_set_stream(h, NULL) == LLZ_OK);
    free(w);                                                        /* folded into the tables: not kept */
    const int counts[3] = {1, 5, 37};
    for (int c = 0; c < 3; c++) {
        const int count = counts[c];
        CHECK(call(llz_dft_mc_forward, h, n, 2, n, n, 2, n, count) == LLZ_OK);
        CHECK(call(llz_dft_mc_forward, h, n, 2, 1, n, 2, n + 3, count) == LLZ_OK);
        CHECK(call(llz_dft_mc_inverse, h, n, 2, n + 1, n, 2, n + 1, count) == LLZ_OK);
        CHECK(call(llz_dft_mc_real_forward, h, n, 1, n / 4 + 1, half, 2, half + 2, count) == LLZ_OK);
        CHECK(call(llz_dft_mc_real_inverse, h, half, 2, half, n, 1, n + 5, count) == LLZ_OK);
    }
    CHECK(llz_dft_mc_set_window(h, NULL) == LLZ_OK);
    /* refusals: the handle lives on */
    float one[8] = {0}, out[8] = {0};
    CHECK(llz_dft_mc_forward(h, one, n, out, n - 1, 1) == LLZ_ERR_ARG && has("llz_dft_mc_forward") && has("out_pitch"));
    CHECK(llz_dft_mc_real_forward(h, one, n, out, half - 1, 1) == LLZ_ERR_ARG && has("llz_dft_mc_real_forward") && has("out_pitch"));
    CHECK(llz_dft_mc_real_inverse(h, one, half, out, n - 1, 1) == LLZ_ERR_ARG && has("llz_dft_mc_real_inverse"));
    CHECK(llz_dft_mc_inverse(h, one, n, out, n, 0) == LLZ_ERR_ARG && has("llz_dft_mc_inverse") && has("count 0"));
    CHECK(llz_dft_mc_forward(h, one, 0, out, n, 1) == LLZ_ERR_ARG && has("in_pitch 0"));
    CHECK(llz_dft_mc_forward(h, NULL, n, out, n, 1) == LLZ_ERR_ARG && has("in NULL"));
    CHECK(llz_dft_mc_forward(h, one, n, NULL, n, 1) == LLZ_ERR_ARG && has("out NULL"));
    CHECK(llz_czt_mc_forward(h, one, n, out, n, 1) == LLZ_ERR_ARG && has("llz_czt_mc_forward") && has("DFT handle"));
    CHECK(llz_czt_mc_real_forward(h, one, n, out, n, 1) == LLZ_ERR_ARG && has("llz_czt_mc_real_forward"));
    CHECK(llz_dft_mc_plan(h, 0, plan) == LLZ_ERR_ARG && has("llz_dft_mc_plan"));
    CHECK(llz_dft_mc_plan(h, 1, NULL) == LLZ_ERR_ARG);
    CHECK(call(llz_dft_mc_forward, h, n, 2, n, n, 2, n, 2) == LLZ_OK);
    llz_dft_mc_uninit(h);
    printf("dft n=%d form=%d m=%d ok\n", n, expect_form, expect_m);
    return 0;
}

static int walk_czt(int n, int k, double f0, double df, int expect_m)
{
    unsigned long h = llz_czt_mc_init(n, k, f0, df);
    CHECK(h != BAD && h != 0);
    int plan[5];
    CHECK(llz_dft_mc_plan(h, 3, plan) == LLZ_OK && plan[0] == LLZ_DFT_FUSED && plan[1] == expect_m);
    float *w = malloc(sizeof(float) * n);
    CHECK(w);
    for (int i = 0; i < n; i++) w[i] = 1.0f / (float)(i + 1);
    CHECK(llz_dft_mc_set_window(h, w) == LLZ_OK);
    free(w);
    CHECK(call(llz_czt_mc_forward, h, n, 2, n, k, 2, k, 3) == LLZ_OK);
    CHECK(call(llz_czt_mc_forward, h, n, 2, 1, k, 2, k + 1, 37) == LLZ_OK);
    CHECK(call(llz_czt_mc_real_forward, h, n, 1, n + 2, k, 2, k + 4, 5) == LLZ_OK);
    float one[8] = {0}, out[8] = {0};
    CHECK(llz_dft_mc_forward(h, one, n, out, n, 1) == LLZ_ERR_ARG && has("llz_dft_mc_forward") && has("zoom handle"));
    CHECK(llz_dft_mc_inverse(h, one, n, out, n, 1) == LLZ_ERR_ARG && has("llz_dft_mc_inverse"));
    CHECK(llz_dft_mc_real_forward(h, one, n, out, n, 1) == LLZ_ERR_ARG && llz_dft_mc_real_inverse(h, one, n, out, n, 1) == LLZ_ERR_ARG);
    CHECK(llz_czt_mc_forward(h, one, n, out, k - 1, 1) == LLZ_ERR_ARG && has("out_pitch"));
    CHECK(call(llz_czt_mc_forward, h, n, 2, n, k, 2, k, 1) == LLZ_OK);
    llz_dft_mc_uninit(h);
    printf("czt n=%d k=%d m=%d ok\n", n, k, expect_m);
    return 0;
}

int main(void)
{
    if (walk_dft(2, LLZ_DFT_FUSED, 8) || walk_dft(3, LLZ_DFT_FUSED, 8) || walk_dft(480, LLZ_DFT_FUSED, 1024) ||
        walk_dft(2047, LLZ_DFT_FUSED, 4096) || walk_dft(2048, LLZ_DFT_FUSED, 4096) || walk_dft(2049, LLZ_DFT_COMPOSED, 8192) ||
        walk_dft(4800, LLZ_DFT_COMPOSED, 16384))
        return 1;
    if (walk_czt(1000, 64, 0.1, 1e-4, 2048) || walk_czt(2048, 2049, 0.0, 1.0 / 4096, 4096) || walk_czt(1, 1, 0.3, -0.1, 8) ||
        walk_czt(300, 3797, -1e9 + 0.25, 0.37 / 3797, 4096))
        return 1;
    /* a composed call that walks two slabs: 8192 points are 64 KiB of scratch a row, 32 rows under a cap of 2 MiB */
    {
        const int n = 2049, count = 37;
        unsigned long h = llz_dft_mc_init(n);
        CHECK(h != BAD);
        int plan[5];
        CHECK(llz_dft_mc_plan(h, count, plan) == LLZ_OK && plan[0] == LLZ_DFT_COMPOSED && plan[2] == 0 && plan[3] == 0 && plan[4] == 1);
        CHECK(llz_dft_mc_configure(h, 0, 2) == LLZ_OK);
        CHECK(llz_dft_mc_plan(h, count, plan) == LLZ_OK && plan[0] == LLZ_DFT_COMPOSED && plan[1] == 8192 && plan[4] == 2);
        CHECK(llz_dft_mc_plan(h, 32, plan) == LLZ_OK && plan[4] == 1);
        CHECK(call(llz_dft_mc_real_inverse, h, n / 2 + 1, 2, 1, n, 1, n + 1, count) == LLZ_OK);
        CHECK(call(llz_dft_mc_forward, h, n, 2, n, n, 2, n + 1, count) == LLZ_OK);
        CHECK(llz_dft_mc_configure(h, 0, 0) == LLZ_OK && llz_dft_mc_plan(h, count, plan) == LLZ_OK && plan[4] == count);
        CHECK(call(llz_dft_mc_forward, h, n, 2, n, n, 2, n, count) == LLZ_OK);
        CHECK(llz_dft_mc_configure(h, 0, -1) == LLZ_OK && llz_dft_mc_plan(h, count, plan) == LLZ_OK && plan[4] == 1);
        llz_dft_mc_uninit(h);
        printf("dft two slabs ok\n");
    }
    /* the composed form forced on handles the fused kernel would serve, and back; refusals leave the form where it was */
    {
        unsigned long hs[2] = {llz_dft_mc_init(480), llz_czt_mc_init(1000, 64, 0.1, 1e-4)};
        for (int i = 0; i < 2; i++) {
            const int n = i ? 1000 : 480, k = i ? 64 : 480;
            dft_fn fn = i ? llz_czt_mc_forward : llz_dft_mc_forward;
            int plan[5];
            CHECK(hs[i] != BAD);
            CHECK(llz_dft_mc_configure(hs[i], 1, 1) == LLZ_OK && llz_dft_mc_plan(hs[i], 37, plan) == LLZ_OK);
            CHECK(plan[0] == LLZ_DFT_COMPOSED && plan[2] == 0 && plan[3] == 0 && plan[4] == 1);
            CHECK(call(fn, hs[i], n, 2, n, k, 2, k + 1, 37) == LLZ_OK);
            CHECK(llz_dft_mc_configure(hs[i], 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_configure") && has("composed 2"));
            CHECK(llz_dft_mc_configure(hs[i], -1, 1) == LLZ_ERR_ARG && llz_dft_mc_configure(hs[i], 1, 65537) == LLZ_ERR_ARG);
            CHECK(llz_dft_mc_plan(hs[i], 37, plan) == LLZ_OK && plan[0] == LLZ_DFT_COMPOSED);
            CHECK(llz_dft_mc_configure(hs[i], 0, -1) == LLZ_OK && llz_dft_mc_plan(hs[i], 37, plan) == LLZ_OK && plan[0] == LLZ_DFT_FUSED);
            CHECK(call(fn, hs[i], n, 2, n, k, 2, k, 37) == LLZ_OK);
            llz_dft_mc_uninit(hs[i]);
        }
        printf("dft configure ok\n");
    }
    CHECK(llz_dft_mc_init(1) == BAD && has("llz_dft_mc_init") && has("n 1 "));
    CHECK(llz_dft_mc_init(0) == BAD && llz_dft_mc_init(-5) == BAD && has("n -5"));
    CHECK(llz_dft_mc_init(1048577) == BAD && has("n 1048577") && has("2..1048576"));
    CHECK(llz_czt_mc_init(0, 4, 0.0, 0.1) == BAD && has("llz_czt_mc_init") && has("n 0"));
    CHECK(llz_czt_mc_init(4, 0, 0.0, 0.1) == BAD && has("k 0"));
    CHECK(llz_czt_mc_init(2048, 2050, 0.0, 0.1) == BAD && has("n + k - 1 <= 4096"));
    CHECK(llz_czt_mc_init(2147483647, 2147483647, 0.0, 0.1) == BAD && has("llz_czt_mc_init"));
    CHECK(llz_czt_mc_init(8, 8, 0.0, 0.5000001) == BAD && has("df 0.5"));
    CHECK(llz_czt_mc_init(8, 8, 0.0, -0.75) == BAD && has("df -0.75"));
    CHECK(llz_czt_mc_init(8, 8, (double)INFINITY, 0.1) == BAD && has("f0 inf"));
    CHECK(llz_czt_mc_init(8, 8, 0.0, (double)NAN) == BAD && has("df"));
    float one[4] = {1, 0, 0, 0};
    int plan[5];
    const unsigned long bad[2] = {0, BAD};
    for (int i = 0; i < 2; i++) {
        CHECK(llz_dft_mc_forward(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_forward") && has("bad handle"));
        CHECK(llz_dft_mc_inverse(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_inverse") && has("bad handle"));
        CHECK(llz_dft_mc_real_forward(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_real_forward"));
        CHECK(llz_dft_mc_real_inverse(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_real_inverse"));
        CHECK(llz_czt_mc_forward(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_czt_mc_forward") && has("bad handle"));
        CHECK(llz_czt_mc_real_forward(bad[i], one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_czt_mc_real_forward"));
        CHECK(llz_dft_mc_set_window(bad[i], one) == LLZ_ERR_ARG && has("llz_dft_mc_set_window"));
        CHECK(llz_dft_mc_set_stream(bad[i], NULL) == LLZ_ERR_ARG && has("llz_dft_mc_set_stream"));
        CHECK(llz_dft_mc_configure(bad[i], 1, 4) == LLZ_ERR_ARG && has("llz_dft_mc_configure") && has("bad handle"));
        CHECK(llz_dft_mc_plan(bad[i], 1, plan) == LLZ_ERR_ARG && has("llz_dft_mc_plan") && has("bad handle"));
        llz_dft_mc_uninit(bad[i]);
    }
    /* a handle of another kind fails the tag check */
    unsigned long other = llz_lpc_init(4);
    CHECK(other != BAD);
    CHECK(llz_dft_mc_forward(other, one, 2, one, 2, 1) == LLZ_ERR_ARG && has("llz_dft_mc_forward") && has("bad handle"));
    llz_dft_mc_uninit(other);
    llz_lpc_uninit(other);
    printf("DFT_SANITIZE_OK\n");
    return 0;
}
