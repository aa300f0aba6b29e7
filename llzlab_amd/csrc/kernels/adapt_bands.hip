// adapt_bands.hip -- llz_adapt_bands_mc (include/llz_adapt_bands.h): a normalised LMS filter of K complex taps for every
// (channel, bin) of a batch of band signals, float32, one launch per call whatever its frames.
//
//   k_bands_nlms<KC, HAS_Y>   a lane owns one (channel, bin): lane g = c bins + k, so a wave's loads and stores of a frame are
//                      contiguous and a wave straddles channel rows where bins is no multiple of 64.  The lane loads its K
//                      weights and K - 1 history values, walks the call's frames with frame m + 1 requested while frame m is
//                      worked on, and stores weights and history back behind the last frame.
// Weights and history are register arrays of KC = the tap ceiling of the instance (4, 8, 16, 32, 64) entries each, indexed by
// the AGE q alone: xr[q] = x[m - q].  Every loop over q is unrolled, so every index is a constant; between frames the history
// shifts by one register.  Taps q >= K do not exist: the guards below are scalar (K is the launch's), and an instance's lower
// half needs none, since K > KC / 2 selects it.  A recursion over frames: nothing here is parallel but the lanes.
//
// The sums, all in float32 with every fused multiply-add written out (contraction is off), q ascending from an accumulator of 0:
//   y_re = fma(-w_im[q], x_im[q], fma(w_re[q], x_re[q], y_re));   y_im = fma(w_im[q], x_re[q], fma(w_re[q], x_im[q], y_im))
//   p    = fma(x_im[q], x_im[q], fma(x_re[q], x_re[q], p))
//   g    = (mu e) / (p + delta), a product and a correctly rounded quotient per component
//   w_re[q] = fma(g_im, x_im[q], fma(g_re, x_re[q], w_re[q]));    w_im[q] = fma(-g_re, x_im[q], fma(g_im, x_re[q], w_im[q]))
#include "bands_steps.hpp"

namespace {

template <int KC, bool HAS_Y>
__global__ void __launch_bounds__(BANDS_THREADS)
k_bands_nlms(const float *__restrict__ xre, const float *__restrict__ xim, const float *__restrict__ dre,
             const float *__restrict__ dim, float *__restrict__ ere, float *__restrict__ eim, float *__restrict__ yre,
             float *__restrict__ yim, float *__restrict__ wre, float *__restrict__ wim, float *__restrict__ hre,
             float *__restrict__ him, const float *__restrict__ mu, float delta, int lanes, int bins, int K, int frames)
{
#pragma clang fp contract(off)
    constexpr int LIVE = bands_live<KC, 4, 1>::value;
    const int g0 = (int)blockIdx.x * BANDS_THREADS, g = g0 + (int)threadIdx.x;
    if (g >= lanes) return;
    const int c = g / bins, k = g - c * bins;
    const float step = mu[c];
    // the state's addresses: a scalar base (the wave's first lane, then q rows of bins floats) and one 32-bit offset per lane --
    // a wave spans at most 63 / bins + 2 channel rows, so the offset stays below (63 + 2 bins) K floats
    const int c0 = __builtin_amdgcn_readfirstlane(g0 / bins), k0 = __builtin_amdgcn_readfirstlane(g0 - (g0 / bins) * bins);
    const int H = K > 1 ? K - 1 : 1;
    const size_t wbase = (size_t)c0 * K * bins + k0, hbase = (size_t)c0 * H * bins + k0;
    const unsigned woff = 4u * (unsigned)((c - c0) * K * bins + (k - k0)), hoff = 4u * (unsigned)((c - c0) * H * bins + (k - k0));
    float wr[KC], wi[KC], xr[KC], xi[KC];                                 // xr[q] = x[m - q] behind frame m's shift
#pragma unroll
    for (int q = 0; q < KC; q++) wr[q] = wi[q] = xr[q] = xi[q] = 0.f;
    BANDS_WALK(q, KC, K) {
        wr[q] = bands_ld(wre + wbase + (size_t)q * bins, woff);
        wi[q] = bands_ld(wim + wbase + (size_t)q * bins, woff);
        if (q + 1 < K) {                                                  // x[-1 - q]: shifted to age q + 1 by the first frame
            xr[q] = bands_ld(hre + hbase + (size_t)q * bins, hoff);
            xi[q] = bands_ld(him + hbase + (size_t)q * bins, hoff);
        }
    }
    const size_t row = ((size_t)c * frames) * bins + k;                   // frame m of this lane: row + m bins
    float nxr = xre[row], nxi = xim[row], ndr = dre[row], ndi = dim[row];
    // frame 0 has arrived before the loop is entered: a wait for it at the loop's head would, from frame 1 on, wait for the
    // stores of the frame before as well.  (HAS_Y is a template parameter for the same reason: the loads of frame m + 1 lie a
    // known number of stores back.)
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
        float ar = 0.f, ai = 0.f, p = 0.f;                                // y and the power take their term of age q
        BANDS_WALK(q, KC, K) {
            ar = __builtin_fmaf(wr[q], xr[q], ar);
            ar = __builtin_fmaf(-wi[q], xi[q], ar);
            ai = __builtin_fmaf(wr[q], xi[q], ai);
            ai = __builtin_fmaf(wi[q], xr[q], ai);
            p = __builtin_fmaf(xr[q], xr[q], p);
            p = __builtin_fmaf(xi[q], xi[q], p);
        }
        const float er = cdr - ar, ei = cdi - ai;
        ere[o] = er;
        eim[o] = ei;
        if (HAS_Y) {
            yre[o] = ar;
            yim[o] = ai;
        }
        if (step != 0.f) {
            const float den = p + delta;
            const float gr = (step * er) / den, gi = (step * ei) / den;
            BANDS_WALK(q, KC, K) {
                wr[q] = __builtin_fmaf(gr, xr[q], wr[q]);
                wr[q] = __builtin_fmaf(gi, xi[q], wr[q]);
                wi[q] = __builtin_fmaf(gi, xr[q], wi[q]);
                wi[q] = __builtin_fmaf(-gr, xi[q], wi[q]);
            }
        }
    }
    BANDS_WALK(q, KC, K) {
        bands_st(wre + wbase + (size_t)q * bins, woff, wr[q]);
        bands_st(wim + wbase + (size_t)q * bins, woff, wi[q]);
        if (q + 1 < K) {                                                  // x[last - q] is the next call's x[-1 - q]
            bands_st(hre + hbase + (size_t)q * bins, hoff, xr[q]);
            bands_st(him + hbase + (size_t)q * bins, hoff, xi[q]);
        }
    }
}
static const int NLMS_LOWEST = 4, NLMS_HIGHEST = 64;                      // the tap ceilings of the instances

static int nlms_shape(const char *who, int channels, int bins, int taps)
{
    const bands_dim dims[] = { { "channels", channels, 65535 }, { "bins", bins, 4097 }, { "taps", taps, NLMS_HIGHEST } };
    return bands_shape(who, dims, 3);
}

} // namespace

extern "C" int llzs_bands_nlms_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                                   float *eim, float *yre, float *yim, float *wre, float *wim, float *hre, float *him,
                                   const float *mu, float delta, int channels, int bins, int taps, int frames, void *stream)
{
    const char *who = "bands_nlms_f32";
    if (!xre || !xim || !dre || !dim || !ere || !eim || !yre != !yim || !wre || !wim || !hre || !him || !mu || frames < 1 ||
        (long)frames * bins > 2147483647L) {
        llzs_set_error("%s: bad arguments", who);
        return LLZ_ERR_ARG;
    }
    const int rc = nlms_shape(who, channels, bins, taps);
    if (rc != LLZ_OK) return rc;
    const int lanes = channels * bins;                                     // at most 65535 x 4097
    const dim3 grid(bands_grid(lanes)), block(BANDS_THREADS);
#define BANDS_LAUNCH(KC)                                                                                                  \
    do {                                                                                                                  \
        if (yre)                                                                                                          \
            hipLaunchKernelGGL((k_bands_nlms<KC, true>), grid, block, 0, as_stream(stream), xre, xim, dre, dim, ere, eim, yre,  \
                               yim, wre, wim, hre, him, mu, delta, lanes, bins, taps, frames);                            \
        else                                                                                                              \
            hipLaunchKernelGGL((k_bands_nlms<KC, false>), grid, block, 0, as_stream(stream), xre, xim, dre, dim, ere, eim, yre, \
                               yim, wre, wim, hre, him, mu, delta, lanes, bins, taps, frames);                            \
    } while (0)
    switch (bands_ceiling(taps, NLMS_LOWEST, NLMS_HIGHEST)) {
    case 4: BANDS_LAUNCH(4); break;
    case 8: BANDS_LAUNCH(8); break;
    case 16: BANDS_LAUNCH(16); break;
    case 32: BANDS_LAUNCH(32); break;
    default: BANDS_LAUNCH(64); break;
    }
#undef BANDS_LAUNCH
    LLZ_LAUNCH_CHECK("k_bands_nlms");
    return LLZ_OK;
}

extern "C" int llzs_bands_nlms_plan(int channels, int bins, int taps, int *out)
{
    const char *who = "bands_nlms_plan";
    int rc = bands_no_out(who, out);
    if (rc == LLZ_OK) rc = nlms_shape(who, channels, bins, taps);
    if (rc == LLZ_OK) bands_plan_tail(out, bands_ceiling(taps, NLMS_LOWEST, NLMS_HIGHEST), channels * bins);
    return rc;
}
