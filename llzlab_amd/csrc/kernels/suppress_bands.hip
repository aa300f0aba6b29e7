// suppress_bands.hip -- llz_suppress_bands_mc (include/llz_suppress_bands.h): the noise and residual-echo postfilter, a real gain
// for every (channel, bin, frame) of a batch of band signals, float32, one launch per call whatever its frames.
//
//   k_bands_suppress<HAS_Y, HAS_G>   k_bands_kalman's plan (kalman_bands.hip) without taps, so of bands_steps.hpp it takes the
//                      launch arithmetic alone: a lane owns one (channel, bin), lane g = c bins + k; a workgroup is one wave.
//                      The lane loads its seven state values and its channel's floor, leakage and flag, walks the call's frames
//                      with the next SUPPRESS_DEPTH frames requested while one is worked on, and stores the state back behind
//                      the last frame.  HAS_Y: the echo estimate is read; HAS_G: the gain is stored.
// The frame number n = count + m decides between the start-up and the running form and when the minimum's windows swap.  It is the
// same for every lane, so the host passes it folded into [0, 2 W) -- n below W as it is, anything else as W + n % W -- and the
// kernel counts it on in a scalar register: both decisions are scalar branches and no frame pays for a modulo.
//
// The recursion, all in float32 with every fused multiply-add written out (contraction is off); the header has it line by line:
//   pe = fma(e_im, e_im, e_re e_re);  S, Smin, Stmp, q -> step;  N = fma(step, pe - N, N);  R = max(eta py, rho R)
//   Q = (N + delta) + R;  rq = 1 / Q;  prio = fma(beta, Z rq, omb max(pe rq - 1, 0));  G = clamp(prio / (1 + prio), gmin, 1)
//   o = G e;  Z = |o|^2
// Two correctly rounded reciprocals per frame behind the start-up, three in the running form; every decision is a select.
#include "bands_steps.hpp"

namespace {

#ifndef SUPPRESS_DEPTH
#define SUPPRESS_DEPTH 1                // frames in flight ahead of the one worked on: 2 gains nothing, 4 loses
#endif

struct suppress_consts {                // formed once by the host layer, in float32
    float omas, omaq, omad, omb, kt, aq, beta, rho, delta, t1;
    unsigned W;
};

template <bool HAS_Y, bool HAS_G>
__global__ void __launch_bounds__(BANDS_THREADS)
k_bands_suppress(const float *__restrict__ ere, const float *__restrict__ eim, const float *__restrict__ yre,
                 const float *__restrict__ yim, float *__restrict__ ore, float *__restrict__ oim, float *__restrict__ gout,
                 float *__restrict__ state, const float *__restrict__ floors, const float *__restrict__ leaks,
                 const int *__restrict__ enable, suppress_consts sc, int lanes, int bins, int frames, unsigned n0)
{
#pragma clang fp contract(off)
    constexpr int D = SUPPRESS_DEPTH;
    const int g = (int)blockIdx.x * BANDS_THREADS + (int)threadIdx.x;
    if (g >= lanes) return;
    const int c = g / bins, k = g - c * bins;
    const bool on = enable[c] != 0;
    const float gmin = floors[c], eta = leaks[c];
    float *const st = state + g;                                          // value s of this lane: st[s lanes]
    float S = st[0], Smin = st[(size_t)lanes], Stmp = st[2 * (size_t)lanes], q = st[3 * (size_t)lanes];
    float N = st[4 * (size_t)lanes], R = st[5 * (size_t)lanes], Z = st[6 * (size_t)lanes];
    const size_t row = ((size_t)c * frames) * bins + k;                   // frame m of this lane: row + m bins
    float ner[D], nei[D], nyr[D], nyi[D];
#pragma unroll
    for (int j = 0; j < D; j++) {
        ner[j] = nei[j] = nyr[j] = nyi[j] = 0.f;
        if (j < frames) {
            ner[j] = ere[row + (size_t)j * bins];
            nei[j] = eim[row + (size_t)j * bins];
            if (HAS_Y) {
                nyr[j] = yre[row + (size_t)j * bins];
                nyi[j] = yim[row + (size_t)j * bins];
            }
        }
    }
    // frame 0 has arrived before the loop is entered: a wait for it at the loop's head would, from the second round on, wait
    // for the stores of the frames before as well (k_bands_kalman's remark)
    asm volatile("" : : "v"(ner[0]), "v"(nei[0]), "v"(nyr[0]), "v"(nyi[0]));
    unsigned n = __builtin_amdgcn_readfirstlane(n0);                      // in [0, 2 W): below W the start-up, else W + phase
    for (int m0 = 0; m0 < frames; m0 += D) {
#pragma unroll
        for (int j = 0; j < D; j++) {
            const int m = m0 + j;
            if (m >= frames) break;
            const size_t o = row + (size_t)m * bins;
            const float er = ner[j], ei = nei[j], yr = nyr[j], yi = nyi[j];
            if (m + D < frames) {                                         // frame m + D flies while frames m .. are worked on
                const size_t p = o + (size_t)D * bins;
                ner[j] = ere[p];
                nei[j] = eim[p];
                if (HAS_Y) {
                    nyr[j] = yre[p];
                    nyi[j] = yim[p];
                }
            }
            float orr = er, oi = ei, G = 1.f;                             // a disabled channel: e's bits, a gain of 1, no step
            if (on) {
                const float pe = __builtin_fmaf(ei, ei, er * er);
                const float py = HAS_Y ? __builtin_fmaf(yi, yi, yr * yr) : 0.f;
                float step;
                if (n < sc.W) {                                           // start-up: running means, no minimum
                    const float cn = 1.f / (float)(n + 1u);
                    const float sa = cn > sc.omas ? cn : sc.omas;
                    S = __builtin_fmaf(sa, pe - S, S);
                    Smin = Stmp = S;
                    step = cn > sc.omad ? cn : sc.omad;
                } else {
                    S = __builtin_fmaf(sc.omas, pe - S, S);
                    if (n == sc.W) {                                      // n % W == 0: the windows swap
                        Smin = S < Stmp ? S : Stmp;
                        Stmp = S;
                    } else {
                        Smin = S < Smin ? S : Smin;
                        Stmp = S < Stmp ? S : Stmp;
                    }
                    const float rm = 1.f / (Smin + sc.delta);
                    float J = (__builtin_fmaf(sc.t1, Smin, -S) * rm) * sc.kt;
                    J = J < 0.f ? 0.f : J;
                    J = J > 1.f ? 1.f : J;
                    q = __builtin_fmaf(sc.aq, q, sc.omaq * J);
                    step = sc.omad * q;
                }
                N = __builtin_fmaf(step, pe - N, N);
                const float a = eta * py, b = sc.rho * R;
                R = a > b ? a : b;
                const float Q = (N + sc.delta) + R;
                const float rq = 1.f / Q;
                float ml = pe * rq - 1.f;
                ml = ml < 0.f ? 0.f : ml;
                const float prio = __builtin_fmaf(sc.beta, Z * rq, sc.omb * ml);
                const float rg = 1.f / (1.f + prio);
                G = prio * rg;
                G = G < gmin ? gmin : G;
                G = G > 1.f ? 1.f : G;
                orr = G * er;
                oi = G * ei;
                Z = __builtin_fmaf(oi, oi, orr * orr);
            }
            ore[o] = orr;
            oim[o] = oi;
            if (HAS_G) gout[o] = G;
            n = n + 1u == 2u * sc.W ? sc.W : n + 1u;
        }
    }
    st[0] = S;                                                            // (a disabled channel's come back with the bits they had)
    st[(size_t)lanes] = Smin;
    st[2 * (size_t)lanes] = Stmp;
    st[3 * (size_t)lanes] = q;
    st[4 * (size_t)lanes] = N;
    st[5 * (size_t)lanes] = R;
    st[6 * (size_t)lanes] = Z;
}

static int suppress_shape(const char *who, int channels, int bins)
{
    const bands_dim dims[] = { { "channels", channels, 65535 }, { "bins", bins, 4097 } };
    return bands_shape(who, dims, 2);
}

} // namespace

extern "C" int llzs_suppress_bands_f32(const float *ere, const float *eim, const float *yre, const float *yim, float *ore,
                                       float *oim, float *g, float *state, const float *floors, const float *leaks,
                                       const int *enable, const float *consts, int window, int channels, int bins, int frames,
                                       int n0, void *stream)
{
    const char *who = "suppress_bands_f32";
    if (!ere || !eim || !yre != !yim || !ore || !oim || !state || !floors || !leaks || !enable || !consts || frames < 1 ||
        (long)frames * bins > 2147483647L || window < 2 || window > 65535 || n0 < 0 || n0 >= 2 * window) {
        llzs_set_error("%s: bad arguments", who);
        return LLZ_ERR_ARG;
    }
    const int rc = suppress_shape(who, channels, bins);
    if (rc != LLZ_OK) return rc;
    const suppress_consts sc = { consts[0], consts[1], consts[2], consts[3], consts[4], consts[5], consts[6], consts[7],
                                 consts[8], consts[9], (unsigned)window };
    const int lanes = channels * bins;                                     // at most 65535 x 4097
    const dim3 grid(bands_grid(lanes)), block(BANDS_THREADS);
#define SUPPRESS_LAUNCH(Y, G)                                                                                             \
    hipLaunchKernelGGL((k_bands_suppress<Y, G>), grid, block, 0, as_stream(stream), ere, eim, yre, yim, ore, oim, g, state, \
                       floors, leaks, enable, sc, lanes, bins, frames, (unsigned)n0)
    if (yre && g) SUPPRESS_LAUNCH(true, true);
    else if (yre) SUPPRESS_LAUNCH(true, false);
    else if (g) SUPPRESS_LAUNCH(false, true);
    else SUPPRESS_LAUNCH(false, false);
#undef SUPPRESS_LAUNCH
    LLZ_LAUNCH_CHECK("k_bands_suppress");
    return LLZ_OK;
}

extern "C" int llzs_suppress_bands_plan(int channels, int bins, int with_y, int *out)
{
    const char *who = "suppress_bands_plan";
    int rc = bands_no_out(who, out);
    if (rc == LLZ_OK) rc = suppress_shape(who, channels, bins);
    if (rc == LLZ_OK) bands_plan_tail(out, with_y != 0, channels * bins);
    return rc;
}
