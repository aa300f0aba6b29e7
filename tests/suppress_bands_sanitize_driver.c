/* suppress_bands_sanitize_driver.c -- the host layer of llz_suppress_bands_mc (csrc/host/llz_suppress_bands_host.c) over the
 * generated stub of the device shim, built with -fsanitize=address,undefined by tests/test_suppress_bands_host.py and never loaded
 * into Python.  It runs the script named by argv[1], one command per line,
 *     init <channels> <bins> <window>
 *     call <frames> <with_y> <with_g>
 *     floor                       set_floor on a channel range, with values outside [0, 1] and a NaN refused
 *     leak                        set_leak likewise, with a negative, an infinite and a NaN value refused
 *     enable                      set_enable on a channel range
 *     state                       get_state of every value, of all channels and of the last one; which = -1 and 7 refused
 *     reset
 * and prints the frame counter behind every command; the test compares it with its own count.  Every caller buffer is host
 * memory of exactly the size the header states, so a staging copy of another length is an error the sanitizer reports.  Each
 * output has one element more than the call may touch, holding a canary. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llz_hip.h"
#include "llz_suppress_bands.h"

#define CANARY 12345.0f
#define FAIL(...) do { printf("FAIL line %d: ", __LINE__); printf(__VA_ARGS__); printf(" (%s)\n", llz_hip_last_error()); return 1; } while (0)

static unsigned long init_with(int channels, int bins, int window)
{
    llz_suppress_cfg cfg;
    llz_suppress_bands_mc_default_cfg(&cfg);
    cfg.window = window;
    return llz_suppress_bands_mc_init(channels, bins, &cfg);
}

static int counter(unsigned long h, const char *what)
{
    long long n = -1;
    if (llz_suppress_bands_mc_frames(h, &n) != LLZ_OK) return 1;
    printf("%s frames %lld\n", what, n);
    return 0;
}

static int bad_cfgs(void)
{
    llz_suppress_cfg d, c;
    llz_suppress_bands_mc_default_cfg(NULL);
    llz_suppress_bands_mc_default_cfg(&d);
    if (d.window != 128 || d.as != 0.8f || d.aq != 0.2f || d.ad != 0.95f || d.t0 != 2.f || d.t1 != 5.f || d.beta != 0.98f ||
        d.rho != 0.6f || d.delta != 1e-6f) FAIL("defaults");
    if (init_with(0, 33, 16) != LLZ_BAD_HANDLE || init_with(65536, 33, 16) != LLZ_BAD_HANDLE || init_with(2, 0, 16) != LLZ_BAD_HANDLE ||
        init_with(2, 4098, 16) != LLZ_BAD_HANDLE || init_with(2, 33, 1) != LLZ_BAD_HANDLE || init_with(2, 33, 65536) != LLZ_BAD_HANDLE)
        FAIL("a shape that must be refused gave a handle");
#define BAD(field, value) do { c = d; c.field = (value); if (llz_suppress_bands_mc_init(2, 33, &c) != LLZ_BAD_HANDLE) FAIL(#field " = " #value); } while (0)
    BAD(as, 1.f); BAD(as, -0.1f); BAD(as, NAN); BAD(aq, 1.f); BAD(aq, NAN); BAD(ad, 1.5f); BAD(ad, -1.f); BAD(beta, 1.f);
    BAD(beta, NAN); BAD(rho, 1.f); BAD(rho, -0.5f); BAD(t0, 0.f); BAD(t0, 5.f); BAD(t0, NAN); BAD(t1, 2.f); BAD(t1, INFINITY);
    BAD(t1, NAN); BAD(delta, 0.f); BAD(delta, -1.f); BAD(delta, INFINITY); BAD(delta, NAN);
#undef BAD
    return 0;
}

static int refusals(unsigned long h, int channels, int bins)
{
    int plan[4], flag[1] = { 1 };
    long long n;
    float one[4] = { 0 };
    if (llz_suppress_bands_mc_plan(h, NULL) >= 0 || llz_suppress_bands_mc_plan(0, plan) >= 0) FAIL("plan refusals");
    if (llz_suppress_bands_mc_plan(h, plan) != LLZ_OK) FAIL("plan");
    if (llz_suppress_bands_mc(h, one, one, NULL, NULL, one, one, NULL, -1) >= 0) FAIL("negative frames");
    if (bins > 1 && llz_suppress_bands_mc(h, one, one, NULL, NULL, one, one, NULL, 2147483647 / bins + 1) >= 0) FAIL("frames x bins");
    if (llz_suppress_bands_mc(h, NULL, one, NULL, NULL, one, one, NULL, 1) >= 0 ||
        llz_suppress_bands_mc(h, one, NULL, NULL, NULL, one, one, one, 1) >= 0 ||
        llz_suppress_bands_mc(h, one, one, NULL, NULL, NULL, one, NULL, 1) >= 0 ||
        llz_suppress_bands_mc(h, one, one, one, one, one, NULL, NULL, 1) >= 0) FAIL("NULL buffers");
    if (llz_suppress_bands_mc(h, one, one, one, NULL, one, one, NULL, 1) >= 0 ||
        llz_suppress_bands_mc(h, one, one, NULL, one, one, one, NULL, 0) >= 0) FAIL("half a y");
    if (llz_suppress_bands_mc(h, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != 0) FAIL("a call of no frames");
    if (llz_suppress_bands_mc_set_enable(h, -1, 1, flag) >= 0 || llz_suppress_bands_mc_set_enable(h, 0, channels + 1, flag) >= 0 ||
        llz_suppress_bands_mc_set_enable(h, channels, 1, flag) >= 0 || llz_suppress_bands_mc_set_enable(h, 0, 0, flag) >= 0 ||
        llz_suppress_bands_mc_set_enable(h, 0, 1, NULL) >= 0) FAIL("set_enable ranges");
    if (llz_suppress_bands_mc_set_floor(h, 0, channels + 1, one) >= 0 || llz_suppress_bands_mc_set_floor(h, 0, 1, NULL) >= 0 ||
        llz_suppress_bands_mc_set_leak(h, channels, 1, one) >= 0 || llz_suppress_bands_mc_set_leak(h, 0, 1, NULL) >= 0 ||
        llz_suppress_bands_mc_set_leak(h, -1, 1, one) >= 0) FAIL("floor and leak ranges");
    if (llz_suppress_bands_mc_get_state(h, LLZ_SUPPRESS_N, 0, channels + 1, one) >= 0 ||
        llz_suppress_bands_mc_get_state(h, LLZ_SUPPRESS_N, 0, 1, NULL) >= 0 || llz_suppress_bands_mc_get_state(h, -1, 0, 1, one) >= 0 ||
        llz_suppress_bands_mc_get_state(h, LLZ_SUPPRESS_STATES, 0, 1, one) >= 0) FAIL("get_state refusals");
    if (llz_suppress_bands_mc_set_stream(h, NULL) != LLZ_OK || llz_suppress_bands_mc_set_stream(0, NULL) >= 0) FAIL("set_stream");
    if (llz_suppress_bands_mc_frames(h, NULL) >= 0 || llz_suppress_bands_mc_frames(0, &n) >= 0 || llz_suppress_bands_mc_reset(0) >= 0 ||
        llz_suppress_bands_mc_reset(LLZ_BAD_HANDLE) >= 0) FAIL("bad handles");
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : NULL;
    if (!fp) { printf("no script\n"); return 1; }
    char line[256];
    unsigned long h = LLZ_BAD_HANDLE;
    int C = 0, B = 0;
    if (bad_cfgs()) return 1;
    while (fgets(line, sizeof line, fp)) {
        int a, b, c, frames, with_y, with_g;
        if (sscanf(line, "init %d %d %d", &a, &b, &c) == 3) {
            if (h != LLZ_BAD_HANDLE) llz_suppress_bands_mc_uninit(h);
            h = c ? init_with(a, b, c) : llz_suppress_bands_mc_init(a, b, NULL);           /* window 0: a NULL cfg, the defaults */
            if (h == LLZ_BAD_HANDLE) FAIL("init");
            C = a; B = b;
            if (refusals(h, C, B)) return 1;
            if (counter(h, "init")) FAIL("frames");
        } else if (sscanf(line, "call %d %d %d", &frames, &with_y, &with_g) == 3) {
            const size_t n = (size_t)C * (size_t)frames * (size_t)B;
            float *in[4], *out[3];
            for (int k = 0; k < 4; k++) {
                in[k] = (float *)malloc(sizeof(float) * n + 1);           /* exact-size inputs: a copy that reads past them is reported */
                if (!in[k]) return 1;
                for (size_t i = 0; i < n; i++) in[k][i] = (float)((i + (size_t)k) % 97) - 48.f;
            }
            for (int k = 0; k < 3; k++) {
                out[k] = (float *)malloc(sizeof(float) * (n + 1));        /* one element more than the call may touch */
                if (!out[k]) return 1;
                for (size_t i = 0; i <= n; i++) out[k][i] = CANARY;
            }
            const int ret = llz_suppress_bands_mc(h, in[0], in[1], with_y ? in[2] : NULL, with_y ? in[3] : NULL, out[0], out[1],
                                                  with_g ? out[2] : NULL, frames);
            if (ret != frames) FAIL("a call of %d frames returned %d", frames, ret);
            for (int k = 0; k < 3; k++) {
                if (out[k][n] != CANARY) FAIL("the element behind output %d was written", k);
                if (k == 2 && !with_g)
                    for (size_t i = 0; i < n; i++)
                        if (out[k][i] != CANARY) FAIL("a g buffer that was not passed was written");
                free(out[k]);
            }
            for (int k = 0; k < 4; k++) free(in[k]);
            int plan[4] = { 0 };
            if (llz_suppress_bands_mc_plan(h, plan) != LLZ_OK) FAIL("plan behind a call");
            if (counter(h, "call")) FAIL("frames");
        } else if (strncmp(line, "floor", 5) == 0 || strncmp(line, "leak", 4) == 0) {
            const int leak = line[0] == 'l', first = C > 1 ? 1 : 0, count = C > 2 ? C - 2 : 1;
            float *v = (float *)malloc(sizeof(float) * (size_t)count);
            if (!v) return 1;
            int (*set)(unsigned long, int, int, const float *) = leak ? llz_suppress_bands_mc_set_leak : llz_suppress_bands_mc_set_floor;
            for (int i = 0; i < count; i++) v[i] = leak ? 0.01f * (float)(i % 5) : 0.25f * (float)(i % 5);
            if (set(h, first, count, v) != LLZ_OK) FAIL("a good %s was refused", leak ? "leakage" : "floor");
            v[count - 1] = NAN;
            if (set(h, first, count, v) >= 0) FAIL("a NaN was taken");
            v[count - 1] = -1e-30f;
            if (set(h, first, count, v) >= 0) FAIL("a negative value was taken");
            v[count - 1] = leak ? INFINITY : 1.0000001f;
            if (set(h, first, count, v) >= 0) FAIL("a value beyond the range was taken");
            v[count - 1] = leak ? 3e38f : 1.f;
            if (set(h, first, count, v) != LLZ_OK) FAIL("the largest value was refused");
            v[count - 1] = 0.f;
            if (set(h, C - 1, 1, v + count - 1) != LLZ_OK) FAIL("a value of 0 on the last channel was refused");
            free(v);
            if (counter(h, leak ? "leak" : "floor")) FAIL("frames");
        } else if (strncmp(line, "enable", 6) == 0) {
            int *on = (int *)malloc(sizeof(int) * (size_t)C);
            if (!on) return 1;
            for (int i = 0; i < C; i++) on[i] = i % 2 ? 0 : 7;
            if (llz_suppress_bands_mc_set_enable(h, 0, C, on) != LLZ_OK || llz_suppress_bands_mc_set_enable(h, C - 1, 1, on) != LLZ_OK)
                FAIL("set_enable");
            free(on);
            if (counter(h, "enable")) FAIL("frames");
        } else if (strncmp(line, "state", 5) == 0) {
            const size_t all = (size_t)C * (size_t)B;
            float *s = (float *)malloc(sizeof(float) * (all + 1));
            if (!s) return 1;
            s[all] = CANARY;
            for (int which = 0; which < LLZ_SUPPRESS_STATES; which++)
                if (llz_suppress_bands_mc_get_state(h, which, 0, C, s) != LLZ_OK || llz_suppress_bands_mc_get_state(h, which, C - 1, 1, s) != LLZ_OK)
                    FAIL("get_state %d", which);
            if (s[all] != CANARY) FAIL("a get wrote behind its buffer");
            free(s);
            if (counter(h, "state")) FAIL("frames");
        } else if (strncmp(line, "reset", 5) == 0) {
            if (llz_suppress_bands_mc_reset(h) != LLZ_OK) FAIL("reset");
            if (counter(h, "reset")) FAIL("frames");
        }
    }
    fclose(fp);
    llz_suppress_bands_mc_uninit(h);
    llz_suppress_bands_mc_uninit(h == LLZ_BAD_HANDLE ? 0 : LLZ_BAD_HANDLE);
    printf("SUPPRESS_BANDS_SANITIZE_OK\n");
    return 0;
}
