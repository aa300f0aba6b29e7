/* kalman_bands_matrix_sanitize_driver.c -- the host layer of llz_kalman_bands_matrix_mc
 * (csrc/host/llz_kalman_bands_matrix_host.c) over the generated stub of the device shim, built with -fsanitize=address,undefined
 * by tests/test_kalman_bands_matrix_host.py and never loaded into Python.  It runs the script named by argv[1], one command per
 * line,
 *     init <inputs> <outputs> <bins> <taps>
 *     call <frames> <with_y>
 *     fail <frames>               a call whose launch the shim refuses: a negative return, nothing moves
 *     taps                        set_taps of a pattern on a sub-matrix, get_taps of all: the pattern comes back in its place
 *     variance                    the same for set_variance / get_variance, with negative, NaN and infinite values refused and
 *                                 nothing changed; get_noise
 *     adapt                       set_adapt on an output range
 *     reset <clear>
 * and prints, behind every command, the frame counter, the launches since the init and which of the two history buffers the
 * last launch read; the test compares the lines with its own count.
 *
 * The one shim entry that is NOT the generated stub is this file's llzs_mkalman_bands_f32: it does the kernel's history step in
 * plain C -- hout = the last taps - 1 frames of (hin, x) -- and checks what the kernel relies on: hout is another buffer than
 * hin, both are the same two buffers throughout, and hin holds exactly the last taps - 1 frames the script fed since the last
 * reset (zeros before them), whatever empty and failed calls and resets came in between.  x carries a pattern of the frame's
 * number since the reset, so a stale, swapped or half-cleared history shows as a wrong value.
 *
 * Every caller buffer is host memory of exactly the size the header states, so a staging copy of another length is an error the
 * sanitizer reports.  Each output has one element more than the call may touch, holding a canary. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_shim.h"
#include "llz_kalman_bands_matrix.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)
#define INIT(i, o, b, k) llz_kalman_bands_matrix_mc_init(i, o, b, k, 0.999f, 0.9f, 1.f, 1e-3f)

static long long g_since_reset;         /* frames the script fed since the last reset: the call in flight starts there */
static int g_launches, g_read = -1, g_fail_next, g_bad;
static const float *g_buf[2];           /* the two history buffers (re), in the order they were first read and written */

static float pattern(int i, long long m, int k, int im)
{
    const float v = (float)((m * 7 + i * 3 + k) % 101) + 1.f;
    return im ? -v - 0.5f : v;
}

int llzs_mkalman_bands_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere, float *eim,
                           float *yre, float *yim, float *wre, float *wim, const float *hin_re, const float *hin_im,
                           float *hout_re, float *hout_im, float *var, float *noise, const int *adapt, const float *consts,
                           int inputs, int outputs, int bins, int taps, int frames, void *stream)
{
    (void)dre; (void)dim; (void)ere; (void)eim; (void)yre; (void)yim; (void)wre; (void)wim; (void)var; (void)noise; (void)adapt;
    (void)outputs; (void)stream;
    if (g_fail_next) {
        g_fail_next = 0;
        llzs_set_error("mkalman_bands_f32: refused on request");
        return LLZ_ERR_ARG;
    }
    if (consts[0] != 0.999f * 0.999f || consts[1] != 1.f - consts[0] || consts[2] != 0.9f || consts[3] != 1.f - 0.9f || consts[4] != 1e-3f) {
        g_bad++;
        printf("BAD: the constants are not the float32 values of the header\n");
    }
    if (hin_re == hout_re || hin_im == hout_im || hin_re == hin_im || hout_re == hout_im) { g_bad++; printf("BAD: history in place\n"); }
    if (!g_buf[0]) { g_buf[0] = hin_re; g_buf[1] = hout_re; }
    if (!((hin_re == g_buf[0] && hout_re == g_buf[1]) || (hin_re == g_buf[1] && hout_re == g_buf[0]))) { g_bad++; printf("BAD: a third history buffer\n"); }
    g_read = hin_re == g_buf[0] ? 0 : 1;
    g_launches++;
    const int H = taps > 1 ? taps - 1 : 1;
    for (int i = 0; i < inputs; i++)
        for (int q = 0; q + 1 < taps; q++)
            for (int k = 0; k < bins; k++) {
                const size_t at = ((size_t)i * (size_t)H + (size_t)q) * (size_t)bins + (size_t)k;
                const long long m = g_since_reset - 1 - q;                /* hin row q holds x_i[-1 - q] of this call */
                const float want_re = m >= 0 ? pattern(i, m, k, 0) : 0.f, want_im = m >= 0 ? pattern(i, m, k, 1) : 0.f;
                if (hin_re[at] != want_re || hin_im[at] != want_im) {
                    if (!g_bad++) printf("BAD: launch %d reads history (%d, %d, %d) = %g %+gi, the script's is %g %+gi\n", g_launches, i,
                                         q, k, (double)hin_re[at], (double)hin_im[at], (double)want_re, (double)want_im);
                }
                const int src = frames - 1 - q;                           /* hout row q: x_i[frames - 1 - q], or what hin still holds */
                const size_t xat = ((size_t)i * (size_t)frames + (size_t)(src >= 0 ? src : 0)) * (size_t)bins + (size_t)k;
                hout_re[at] = src >= 0 ? xre[xat] : hin_re[at - (size_t)frames * (size_t)bins];
                hout_im[at] = src >= 0 ? xim[xat] : hin_im[at - (size_t)frames * (size_t)bins];
            }
    return LLZ_OK;
}

static int counter(unsigned long h, const char *what, long long expect)
{
    long long n = -1;
    if (llz_kalman_bands_matrix_mc_frames(h, &n) != LLZ_OK || n != expect) return 1;
    printf("%s frames %lld launches %d read %d\n", what, n, g_launches, g_read);
    return 0;
}

static int refusals(unsigned long h, int inputs, int outputs, int bins)
{
    int plan[5], flag[1] = { 1 };
    long long n;
    float one[4] = { 0 };
    if (llz_kalman_bands_matrix_mc_plan(h, NULL) >= 0 || llz_kalman_bands_matrix_mc_plan(0, plan) >= 0) FAIL("plan refusals");
    if (llz_kalman_bands_matrix_mc_plan(h, plan) != LLZ_OK) FAIL("plan");
    if (llz_kalman_bands_matrix_mc(h, one, one, one, one, one, one, NULL, NULL, -1) >= 0) FAIL("negative frames");
    if (bins > 1 && llz_kalman_bands_matrix_mc(h, one, one, one, one, one, one, NULL, NULL, 2147483647 / bins + 1) >= 0) FAIL("frames x bins");
    if (llz_kalman_bands_matrix_mc(h, NULL, one, one, one, one, one, NULL, NULL, 1) >= 0 ||
        llz_kalman_bands_matrix_mc(h, one, one, one, NULL, one, one, NULL, NULL, 1) >= 0 ||
        llz_kalman_bands_matrix_mc(h, one, one, one, one, one, NULL, NULL, NULL, 1) >= 0) FAIL("NULL buffers");
    if (llz_kalman_bands_matrix_mc(h, one, one, one, one, one, one, one, NULL, 1) >= 0 ||
        llz_kalman_bands_matrix_mc(h, one, one, one, one, one, one, NULL, one, 0) >= 0) FAIL("half a y");
    if (llz_kalman_bands_matrix_mc(h, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != 0) FAIL("a call of no frames");
    if (llz_kalman_bands_matrix_mc_set_adapt(h, -1, 1, flag) >= 0 || llz_kalman_bands_matrix_mc_set_adapt(h, 0, outputs + 1, flag) >= 0 ||
        llz_kalman_bands_matrix_mc_set_adapt(h, outputs, 1, flag) >= 0 || llz_kalman_bands_matrix_mc_set_adapt(h, 0, 0, flag) >= 0 ||
        llz_kalman_bands_matrix_mc_set_adapt(h, 0, 1, NULL) >= 0) FAIL("set_adapt ranges");
    if (llz_kalman_bands_matrix_mc_set_taps(h, 0, outputs + 1, 0, 1, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, 0, inputs + 1, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, inputs, 1, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, -1, 1, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, 0, 0, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_taps(h, 0, 1, 0, 1, one, NULL) >= 0 ||
        llz_kalman_bands_matrix_mc_get_taps(h, outputs, 1, 0, 1, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_get_taps(h, 0, 1, inputs - 1, 2, one, one) >= 0 ||
        llz_kalman_bands_matrix_mc_get_taps(h, 0, 1, 0, 1, NULL, one) >= 0) FAIL("taps ranges");
    if (llz_kalman_bands_matrix_mc_set_variance(h, 0, outputs + 1, 0, 1, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_variance(h, 0, 1, inputs, 1, one) >= 0 ||
        llz_kalman_bands_matrix_mc_set_variance(h, 0, 1, 0, 1, NULL) >= 0 ||
        llz_kalman_bands_matrix_mc_get_variance(h, outputs, 1, 0, 1, one) >= 0 ||
        llz_kalman_bands_matrix_mc_get_variance(h, 0, 1, inputs - 1, 2, one) >= 0 ||
        llz_kalman_bands_matrix_mc_get_variance(h, 0, 1, 0, 1, NULL) >= 0 ||
        llz_kalman_bands_matrix_mc_get_noise(h, -1, 1, one) >= 0 || llz_kalman_bands_matrix_mc_get_noise(h, 0, outputs + 1, one) >= 0 ||
        llz_kalman_bands_matrix_mc_get_noise(h, 0, 1, NULL) >= 0) FAIL("variance and noise ranges");
    if (llz_kalman_bands_matrix_mc_set_stream(h, NULL) != LLZ_OK || llz_kalman_bands_matrix_mc_set_stream(0, NULL) >= 0) FAIL("set_stream");
    if (llz_kalman_bands_matrix_mc_frames(h, NULL) >= 0 || llz_kalman_bands_matrix_mc_frames(0, &n) >= 0 ||
        llz_kalman_bands_matrix_mc_reset(0, 1) >= 0 || llz_kalman_bands_matrix_mc_reset(LLZ_BAD_HANDLE, 0) >= 0) FAIL("bad handles");
    return 0;
}

/* one call of `frames` frames on exact-size host buffers; fail: the shim refuses the launch */
static int one_call(unsigned long h, int I, int O, int B, int frames, int with_y, int fail)
{
    const size_t nx = (size_t)I * (size_t)frames * (size_t)B, n = (size_t)O * (size_t)frames * (size_t)B;
    float *in[4], *out[4];
    for (int k = 0; k < 4; k++) {
        const size_t len = k < 2 ? nx : n;
        in[k] = (float *)malloc(sizeof(float) * len + 1);             /* exact-size inputs: a copy that reads past them is reported */
        out[k] = (float *)malloc(sizeof(float) * (n + 1));            /* one element more than the call may touch */
        if (!in[k] || !out[k]) return 1;
        for (size_t i = 0; i < len; i++) in[k][i] = (float)((i + (size_t)k) % 97) - 48.f;
        for (size_t i = 0; i <= n; i++) out[k][i] = CANARY;
    }
    for (int i = 0; i < I; i++)
        for (int m = 0; m < frames; m++)
            for (int k = 0; k < B; k++) {
                const size_t at = ((size_t)i * (size_t)frames + (size_t)m) * (size_t)B + (size_t)k;
                in[0][at] = pattern(i, g_since_reset + m, k, 0);
                in[1][at] = pattern(i, g_since_reset + m, k, 1);
            }
    g_fail_next = fail;
    const int ret = llz_kalman_bands_matrix_mc(h, in[0], in[1], in[2], in[3], out[0], out[1], with_y ? out[2] : NULL,
                                               with_y ? out[3] : NULL, frames);
    g_fail_next = 0;
    if (fail ? ret >= 0 : ret != frames) FAIL("a call of %d frames returned %d", frames, ret);
    if (!fail) g_since_reset += frames;
    for (int k = 0; k < 4; k++) {
        if (out[k][n] != CANARY) FAIL("the element behind output %d was written", k);
        if (k >= 2 && !with_y)
            for (size_t i = 0; i < n; i++)
                if (out[k][i] != CANARY) FAIL("a y buffer that was not passed was written");
        free(in[k]); free(out[k]);
    }
    return 0;
}

/* set on a sub-matrix and get of all and of the sub-matrix; var: the variances (with the refusals) and get_noise, else the taps */
static int round_trip(unsigned long h, int I, int O, int B, int K, int var)
{
    const int of = O > 1 ? 1 : 0, oc = O > 2 ? O - 2 : 1, inf = I > 1 ? 1 : 0, ic = I > 2 ? I - 2 : 1;
    const size_t path = (size_t)K * (size_t)B, sub = (size_t)oc * (size_t)ic * path, all = (size_t)O * (size_t)I * path;
    const size_t nn = (size_t)O * (size_t)B;
    float *wre = (float *)malloc(sizeof(float) * sub), *wim = (float *)malloc(sizeof(float) * sub);
    float *gre = (float *)malloc(sizeof(float) * (all + 1)), *gim = (float *)malloc(sizeof(float) * (all + 1));
    float *psi = (float *)malloc(sizeof(float) * (nn + 1));
    if (!wre || !wim || !gre || !gim || !psi) return 1;
    for (size_t i = 0; i < sub; i++) { wre[i] = (float)(i % 31) + 1.f; wim[i] = -(float)(i % 29) - 1.f; }
    gre[all] = gim[all] = psi[nn] = CANARY;
    if (var) {
        if (llz_kalman_bands_matrix_mc_set_variance(h, of, oc, inf, ic, wre) != LLZ_OK) FAIL("set_variance");
        if (llz_kalman_bands_matrix_mc_set_variance(h, of, oc, inf, ic, wim) >= 0) FAIL("negative variances were taken");
        const float bad[3] = { NAN, INFINITY, -0.5f };
        for (int b = 0; b < 3; b++) {
            const float keep = wre[sub - 1];
            wre[sub - 1] = bad[b];
            if (llz_kalman_bands_matrix_mc_set_variance(h, of, oc, inf, ic, wre) >= 0) FAIL("a variance of %g was taken", (double)bad[b]);
            wre[sub - 1] = keep;
        }
        if (llz_kalman_bands_matrix_mc_get_variance(h, of, oc, inf, ic, gre) != LLZ_OK || memcmp(gre, wre, sizeof(float) * sub))
            FAIL("a refused set_variance changed something");
        wre[sub - 1] = 0.f;
        if (llz_kalman_bands_matrix_mc_set_variance(h, of, oc, inf, ic, wre) != LLZ_OK) FAIL("a variance of 0 was refused");
        if (llz_kalman_bands_matrix_mc_get_variance(h, 0, O, 0, I, gre) != LLZ_OK) FAIL("get_variance");
        if (llz_kalman_bands_matrix_mc_get_noise(h, 0, O, psi) != LLZ_OK || llz_kalman_bands_matrix_mc_get_noise(h, O - 1, 1, psi) != LLZ_OK)
            FAIL("get_noise");
    } else {
        if (llz_kalman_bands_matrix_mc_set_taps(h, of, oc, inf, ic, wre, wim) != LLZ_OK) FAIL("set_taps");
        if (llz_kalman_bands_matrix_mc_get_taps(h, 0, O, 0, I, gre, gim) != LLZ_OK) FAIL("get_taps");
    }
    for (int o = 0; o < oc; o++)
        for (int i = 0; i < ic; i++) {
            const size_t in_all = ((size_t)(of + o) * (size_t)I + (size_t)(inf + i)) * path, in_sub = ((size_t)o * (size_t)ic + (size_t)i) * path;
            if (memcmp(gre + in_all, wre + in_sub, sizeof(float) * path) || (!var && memcmp(gim + in_all, wim + in_sub, sizeof(float) * path)))
                FAIL("a get does not return the set at path (%d, %d)", of + o, inf + i);
        }
    if (gre[all] != CANARY || gim[all] != CANARY || psi[nn] != CANARY) FAIL("a get wrote behind its buffer");
    gre[sub] = gim[sub] = CANARY;                                         /* the sub-matrix alone, into a buffer of its size */
    if (var ? llz_kalman_bands_matrix_mc_get_variance(h, of, oc, inf, ic, gre) != LLZ_OK
            : llz_kalman_bands_matrix_mc_get_taps(h, of, oc, inf, ic, gre, gim) != LLZ_OK) FAIL("a get of the sub-matrix");
    if (memcmp(gre, wre, sizeof(float) * sub) || (!var && memcmp(gim, wim, sizeof(float) * sub)) || gre[sub] != CANARY || gim[sub] != CANARY)
        FAIL("a get of the sub-matrix differs");
    if (var ? llz_kalman_bands_matrix_mc_get_variance(h, O - 1, 1, I - 1, 1, gre) != LLZ_OK
            : llz_kalman_bands_matrix_mc_get_taps(h, O - 1, 1, I - 1, 1, gre, gim) != LLZ_OK) FAIL("a get of the last path");
    free(wre); free(wim); free(gre); free(gim); free(psi);
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int I = 0, O = 0, B = 0, K = 0;
    if (INIT(0, 2, 33, 8) != LLZ_BAD_HANDLE || INIT(9, 2, 33, 1) != LLZ_BAD_HANDLE || INIT(2, 0, 33, 8) != LLZ_BAD_HANDLE ||
        INIT(2, 4097, 33, 8) != LLZ_BAD_HANDLE || INIT(2, 2, 4098, 8) != LLZ_BAD_HANDLE || INIT(1, 2, 33, 33) != LLZ_BAD_HANDLE ||
        INIT(5, 2, 33, 7) != LLZ_BAD_HANDLE || INIT(2, 2, 33, 0) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_matrix_mc_init(2, 2, 33, 8, 0.f, 0.9f, 1.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_matrix_mc_init(2, 2, 33, 8, 0.999f, 1.f, 1.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_matrix_mc_init(2, 2, 33, 8, 0.999f, 0.9f, 0.f, 1e-3f) != LLZ_BAD_HANDLE ||
        llz_kalman_bands_matrix_mc_init(2, 2, 33, 8, 0.999f, 0.9f, 1.f, 0.f) != LLZ_BAD_HANDLE)
        FAIL("an init that must be refused gave a handle");
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, d, frames, with_y, clear;
        if (sscanf(line, "init %d %d %d %d", &a, &b, &c, &d) == 4) {
            if (h != LLZ_BAD_HANDLE) llz_kalman_bands_matrix_mc_uninit(h);
            h = INIT(a, b, c, d);
            if (h == LLZ_BAD_HANDLE) FAIL("init");
            I = a; O = b; B = c; K = d;
            g_since_reset = 0; g_launches = 0; g_read = -1; g_buf[0] = g_buf[1] = NULL;
            if (refusals(h, I, O, B)) return 1;
            if (counter(h, "init", 0)) FAIL("frames");
        } else if (sscanf(line, "call %d %d", &frames, &with_y) == 2) {
            if (one_call(h, I, O, B, frames, with_y, 0)) return 1;
            if (counter(h, "call", g_since_reset)) FAIL("frames");
        } else if (sscanf(line, "fail %d", &frames) == 1) {
            if (one_call(h, I, O, B, frames, 1, 1)) return 1;
            if (counter(h, "fail", g_since_reset)) FAIL("frames");
        } else if (strncmp(line, "taps", 4) == 0 || strncmp(line, "variance", 8) == 0) {
            if (round_trip(h, I, O, B, K, line[0] == 'v')) return 1;
            if (counter(h, line[0] == 'v' ? "variance" : "taps", g_since_reset)) FAIL("frames");
        } else if (strncmp(line, "adapt", 5) == 0) {
            int *on = (int *)malloc(sizeof(int) * (size_t)O);
            if (!on) return 1;
            for (int i = 0; i < O; i++) on[i] = i % 2 ? 0 : 7;
            if (llz_kalman_bands_matrix_mc_set_adapt(h, 0, O, on) != LLZ_OK || llz_kalman_bands_matrix_mc_set_adapt(h, O - 1, 1, on) != LLZ_OK)
                FAIL("set_adapt");
            free(on);
            if (counter(h, "adapt", g_since_reset)) FAIL("frames");
        } else if (sscanf(line, "reset %d", &clear) == 1) {
            if (llz_kalman_bands_matrix_mc_reset(h, clear) != LLZ_OK) FAIL("reset");
            g_since_reset = 0;
            if (counter(h, "reset", 0)) FAIL("frames");
        }
    }
    fclose(fp);
    llz_kalman_bands_matrix_mc_uninit(h);
    llz_kalman_bands_matrix_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    if (g_bad) { printf("FAIL: %d history faults\n", g_bad); return 1; }
    printf("KALMAN_BANDS_MATRIX_SANITIZE_OK\n");
    return 0;
}
