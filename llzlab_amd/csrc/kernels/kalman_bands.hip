// kalman_bands.hip -- llz_kalman_bands_mc (include/llz_kalman_bands.h): the diagonal state-space (Kalman) adaptive filter of K
// complex taps for every (channel, bin) of a batch of band signals, float32, one launch per call whatever its frames.
//
//   k_bands_kalman<KC, HAS_Y>   k_bands_nlms's plan (adapt_bands.hip) over bands_steps.hpp: a lane owns one (channel, bin), lane
//                      g = c bins + k; a workgroup is one wave.  The lane loads its K weights, K variances, its noise power and
//                      K - 1 history values, walks the call's frames with frame m + 1 requested while frame m is worked on, and
//                      stores the state back behind the last frame.
// Weights, history and variances are register arrays of KC = the tap ceiling of the instance (4, 8, 16, 32) entries, indexed by
// the AGE q alone with constant indices: 5 KC + 1 registers of state per lane, 161 at the ceiling of 32 -- which is why there is
// no instance of 64.  Taps q >= K do not exist (scalar guards, K is the launch's).
//
// The sums, all in float32 with every fused multiply-add written out (contraction is off), q ascending:
//   y_re = fma(-w_im[q], x_im[q], fma(w_re[q], x_re[q], y_re));   y_im = fma(w_im[q], x_re[q], fma(w_re[q], x_im[q], y_im))
//                                                                  from 0: k_bands_nlms's y, instruction for instruction
// and where the channel adapts
//   psi   = fma(lam, psi, oml * fma(e_im, e_im, e_re * e_re))
//   u[q]  = P[q] * fma(x_im[q], x_im[q], x_re[q] * x_re[q])        (formed twice, for s and for the update: the same bits)
//   s     = (psi + delta) + u[0] + u[1] + ...                      one addition per tap
//   r     = 1 / s                                                  the one correctly rounded quotient of a frame
//   k     = (e r) P[q]                                             two products per component
//   w_re[q] = fma(k_im, x_im[q], fma(k_re, x_re[q], w_re[q]));    w_im[q] = fma(-k_re, x_im[q], fma(k_im, x_re[q], w_im[q]))
//   c     = 1 - u[q] r;  c < 0: c = 0                              the clamp of the reciprocal form
//   P[q]  = fma(omA2, fma(w_im[q], w_im[q], w_re[q] * w_re[q]), (A2 c) P[q])
#include "bands_steps.hpp"

namespace {

struct kalman_consts {                  // formed once by the host layer, in float32
    float A2, omA2, lam, oml, delta;
};

template <int KC, bool HAS_Y>
__global__ void __launch_bounds__(BANDS_THREADS)
k_bands_kalman(const float *__restrict__ xre, const float *__restrict__ xim, const float *__restrict__ dre,
               const float *__restrict__ dim, float *__restrict__ ere, float *__restrict__ eim, float *__restrict__ yre,
               float *__restrict__ yim, float *__restrict__ wre, float *__restrict__ wim, float *__restrict__ hre,
               float *__restrict__ him, float *__restrict__ var, float *__restrict__ noise, const int *__restrict__ adapt,
               kalman_consts kc, int lanes, int bins, int K, int frames)
{
#pragma clang fp contract(off)
    constexpr int LIVE = bands_live<KC, 4, 1>::value;
    const int g0 = (int)blockIdx.x * BANDS_THREADS, g = g0 + (int)threadIdx.x;
    if (g >= lanes) return;
    const int c = g / bins, k = g - c * bins;
    const bool on = adapt[c] != 0;
    // the state's addresses: a scalar base (the wave's first lane, then q rows of bins floats) and one 32-bit offset per lane --
    // a wave spans at most 63 / bins + 2 channel rows, so the offset stays below (63 + 2 bins) K floats
    const int c0 = __builtin_amdgcn_readfirstlane(g0 / bins), k0 = __builtin_amdgcn_readfirstlane(g0 - (g0 / bins) * bins);
    const int H = K > 1 ? K - 1 : 1;
    const size_t wbase = (size_t)c0 * K * bins + k0, hbase = (size_t)c0 * H * bins + k0;
    const unsigned woff = 4u * (unsigned)((c - c0) * K * bins + (k - k0)), hoff = 4u * (unsigned)((c - c0) * H * bins + (k - k0));
    float wr[KC], wi[KC], xr[KC], xi[KC], P[KC];                          // xr[q] = x[m - q] behind frame m's shift
#pragma unroll
    for (int q = 0; q < KC; q++) wr[q] = wi[q] = xr[q] = xi[q] = P[q] = 0.f;
    BANDS_WALK(q, KC, K) {
        wr[q] = bands_ld(wre + wbase + (size_t)q * bins, woff);
        wi[q] = bands_ld(wim + wbase + (size_t)q * bins, woff);
        P[q] = bands_ld(var + wbase + (size_t)q * bins, woff);
        if (q + 1 < K) {                                                  // x[-1 - q]: shifted to age q + 1 by the first frame
            xr[q] = bands_ld(hre + hbase + (size_t)q * bins, hoff);
            xi[q] = bands_ld(him + hbase + (size_t)q * bins, hoff);
        }
    }
    float psi = noise[g];
    const size_t row = ((size_t)c * frames) * bins + k;                   // frame m of this lane: row + m bins
    float nxr = xre[row], nxi = xim[row], ndr = dre[row], ndi = dim[row];
    // frame 0 has arrived before the loop is entered: a wait for it at the loop's head would, from frame 1 on, wait for the
    // stores of the frame before as well
    asm volatile("" : : "v"(nxr), "v"(nxi), "v"(ndr), "v"(ndi));
    for (int m = 0; m < frames; m++) {
        const size_t o = row + (size_t)m * bins;
        const float cxr = nxr, cxi = nxi, cdr = ndr, cdi = ndi;
        if (m + 1 < frames) {                                             // frame m + 1 flies while frame m is worked on
            nxr = xre[o + bins];
            nxi = xim[o + bins];
            ndr = dre[o + bins];
            ndi = dim[o + bins];
        }
        bands_shift<1>(xr, xi);
        xr[0] = cxr;
        xi[0] = cxi;
        float ar = 0.f, ai = 0.f;
        BANDS_WALK(q, KC, K) {
            ar = __builtin_fmaf(wr[q], xr[q], ar);
            ar = __builtin_fmaf(-wi[q], xi[q], ar);
            ai = __builtin_fmaf(wr[q], xi[q], ai);
            ai = __builtin_fmaf(wi[q], xr[q], ai);
        }
        const float er = cdr - ar, ei = cdi - ai;
        ere[o] = er;
        eim[o] = ei;
        if (HAS_Y) {
            yre[o] = ar;
            yim[o] = ai;
        }
        if (on) {
            psi = __builtin_fmaf(kc.lam, psi, kc.oml * __builtin_fmaf(ei, ei, er * er));
            float s = psi + kc.delta;
            BANDS_WALK(q, KC, K) s = s + P[q] * __builtin_fmaf(xi[q], xi[q], xr[q] * xr[q]);
            const float r = 1.f / s;
            const float gr = er * r, gi = ei * r;
            BANDS_WALK(q, KC, K) {
                const float u = P[q] * __builtin_fmaf(xi[q], xi[q], xr[q] * xr[q]);
                const float kr = gr * P[q], ki = gi * P[q];
                wr[q] = __builtin_fmaf(kr, xr[q], wr[q]);
                wr[q] = __builtin_fmaf(ki, xi[q], wr[q]);
                wi[q] = __builtin_fmaf(ki, xr[q], wi[q]);
                wi[q] = __builtin_fmaf(-kr, xi[q], wi[q]);
                float cq = 1.f - u * r;
                cq = cq < 0.f ? 0.f : cq;
                P[q] = __builtin_fmaf(kc.omA2, __builtin_fmaf(wi[q], wi[q], wr[q] * wr[q]), (kc.A2 * cq) * P[q]);
            }
        }
    }
    BANDS_WALK(q, KC, K) {
        bands_st(wre + wbase + (size_t)q * bins, woff, wr[q]);           // (a frozen channel's come back with the bits they had)
        bands_st(wim + wbase + (size_t)q * bins, woff, wi[q]);
        bands_st(var + wbase + (size_t)q * bins, woff, P[q]);
        if (q + 1 < K) {                                                  // x[last - q] is the next call's x[-1 - q]
            bands_st(hre + hbase + (size_t)q * bins, hoff, xr[q]);
            bands_st(him + hbase + (size_t)q * bins, hoff, xi[q]);
        }
    }
    noise[g] = psi;
}
static const int KALMAN_LOWEST = 4, KALMAN_HIGHEST = 32;                  // the tap ceilings of the instances

static int kalman_shape(const char *who, int channels, int bins, int taps)
{
    const bands_dim dims[] = { { "channels", channels, 65535 }, { "bins", bins, 4097 }, { "taps", taps, KALMAN_HIGHEST } };
    return bands_shape(who, dims, 3);
}

} // namespace

extern "C" int llzs_kalman_bands_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                                     float *eim, float *yre, float *yim, float *wre, float *wim, float *hre, float *him,
                                     float *var, float *noise, const int *adapt, const float *consts, int channels, int bins,
                                     int taps, int frames, void *stream)
{
    const char *who = "kalman_bands_f32";
    if (!xre || !xim || !dre || !dim || !ere || !eim || !yre != !yim || !wre || !wim || !hre || !him || !var || !noise ||
        !adapt || !consts || frames < 1 || (long)frames * bins > 2147483647L) {
        llzs_set_error("%s: bad arguments", who);
        return LLZ_ERR_ARG;
    }
    const int rc = kalman_shape(who, channels, bins, taps);
    if (rc != LLZ_OK) return rc;
    const kalman_consts kc = { consts[0], consts[1], consts[2], consts[3], consts[4] };
    const int lanes = channels * bins;                                     // at most 65535 x 4097
    const dim3 grid(bands_grid(lanes)), block(BANDS_THREADS);
#define KALMAN_LAUNCH(KC)                                                                                                 \
    do {                                                                                                                  \
        if (yre)                                                                                                          \
            hipLaunchKernelGGL((k_bands_kalman<KC, true>), grid, block, 0, as_stream(stream), xre, xim, dre, dim, ere, eim,     \
                               yre, yim, wre, wim, hre, him, var, noise, adapt, kc, lanes, bins, taps, frames);           \
        else                                                                                                              \
            hipLaunchKernelGGL((k_bands_kalman<KC, false>), grid, block, 0, as_stream(stream), xre, xim, dre, dim, ere, eim,    \
                               yre, yim, wre, wim, hre, him, var, noise, adapt, kc, lanes, bins, taps, frames);           \
    } while (0)
    switch (bands_ceiling(taps, KALMAN_LOWEST, KALMAN_HIGHEST)) {
    case 4: KALMAN_LAUNCH(4); break;
    case 8: KALMAN_LAUNCH(8); break;
    case 16: KALMAN_LAUNCH(16); break;
    default: KALMAN_LAUNCH(32); break;
    }
#undef KALMAN_LAUNCH
    LLZ_LAUNCH_CHECK("k_bands_kalman");
    return LLZ_OK;
}

extern "C" int llzs_kalman_bands_plan(int channels, int bins, int taps, int *out)
{
    const char *who = "kalman_bands_plan";
    int rc = bands_no_out(who, out);
    if (rc == LLZ_OK) rc = kalman_shape(who, channels, bins, taps);
    if (rc == LLZ_OK) bands_plan_tail(out, bands_ceiling(taps, KALMAN_LOWEST, KALMAN_HIGHEST), channels * bins);
    return rc;
}
