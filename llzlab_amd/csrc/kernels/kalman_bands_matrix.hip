// kalman_bands_matrix.hip -- llz_kalman_bands_matrix_mc (include/llz_kalman_bands_matrix.h): the diagonal state-space (Kalman)
// adaptive filter of I references x K complex taps for every (output, bin) of a batch of band signals, float32, one launch per
// call whatever its frames.  It is to kalman_bands.hip (K4l) what adapt_bands_matrix.hip (K4k) is to adapt_bands.hip (K4j).
//
//   k_bands_matrix_kalman<I, JC, HAS_Y>   k_bands_matrix_nlms's plan over bands_steps.hpp: a lane owns one (output, bin), lane
//                      g = o bins + k; a workgroup is one wave.  The lane loads its J = I K weights, J variances, its noise power
//                      and the I (K - 1) history values of its bin, walks the call's frames with frame m + 1 (I values of x, one
//                      of d) requested while frame m is worked on, and stores its state back behind the last frame.
// Weights, regressor and variances are register arrays of JC = the entry ceiling of the instance (8, 16, 32) entries each:
// 5 JC + 1 registers of state per lane, 161 at the ceiling of 32 as in k_bands_kalman -- which is why there is no instance of 64
// -- and 4 I more for the frame in flight and the frame at hand.  Entry j = q I + i holds age q of input i, so the header's walk
// "q ascending, within a q i ascending" is j ascending with constant indices.  Entries j >= J do not exist (scalar guards, J is
// the launch's).
//
// The history is SHARED by the outputs and follows k_bands_matrix_nlms's rule: the kernel reads hin, the lanes of output 0 alone
// -- one lane per (input, age, bin), whether or not output 0 adapts -- write hout, another buffer; the host swaps the two behind
// a launch.  No element has two writers, and no workgroup can read what this launch wrote.
//
// The sums are k_bands_kalman's with j in the place of q, float32 with every fused multiply-add written out (contraction is off):
//   y_re = fma(-w_im[j], x_im[j], fma(w_re[j], x_re[j], y_re));   y_im = fma(w_im[j], x_re[j], fma(w_re[j], x_im[j], y_im))
// and where the output adapts
//   psi   = fma(lam, psi, oml * fma(e_im, e_im, e_re * e_re))
//   u[j]  = P[j] * fma(x_im[j], x_im[j], x_re[j] * x_re[j])        (formed twice, for s and for the update: the same bits)
//   s     = (psi + delta) + u[0] + u[1] + ...                      one addition per entry: the JOINT predicted error power
//   r     = 1 / s                                                  the one correctly rounded quotient of a frame
//   k     = (e r) P[j]
//   w_re[j] = fma(k_im, x_im[j], fma(k_re, x_re[j], w_re[j]));    w_im[j] = fma(-k_re, x_im[j], fma(k_im, x_re[j], w_im[j]))
//   c     = 1 - u[j] r;  c < 0: c = 0
//   P[j]  = fma(omA2, fma(w_im[j], w_im[j], w_re[j] * w_re[j]), (A2 c) P[j])
// With I = 1 this is k_bands_kalman value for value in the same order, and its bits; a frozen output's y and e are
// k_bands_matrix_nlms's at mu = 0.
#include "bands_steps.hpp"

namespace {

constexpr int MKAL_MAX_INPUTS = 8, MKAL_LOWEST = 8, MKAL_MAX_ENTRIES = 32;   // (the entry ceilings of the instances: 8, 16, 32)

struct mkal_consts {                    // formed once by the host layer, in float32
    float A2, omA2, lam, oml, delta;
};

template <int I, int JC, bool HAS_Y>
__global__ void __launch_bounds__(BANDS_THREADS)
k_bands_matrix_kalman(const float *__restrict__ xre, const float *__restrict__ xim, const float *__restrict__ dre,
                      const float *__restrict__ dim, float *__restrict__ ere, float *__restrict__ eim, float *__restrict__ yre,
                      float *__restrict__ yim, float *__restrict__ wre, float *__restrict__ wim, const float *__restrict__ hin_re,
                      const float *__restrict__ hin_im, float *__restrict__ hout_re, float *__restrict__ hout_im,
                      float *__restrict__ var, float *__restrict__ noise, const int *__restrict__ adapt, mkal_consts kc, int lanes,
                      int bins, int K, int frames)
{
#pragma clang fp contract(off)
    constexpr int LIVE = bands_live<JC, MKAL_LOWEST, I>::value;
    const int g0 = (int)blockIdx.x * BANDS_THREADS, g = g0 + (int)threadIdx.x;
    if (g >= lanes) return;
    const int o = g / bins, k = g - o * bins;
    const bool on = adapt[o] != 0;
    const int J = I * K, H = K > 1 ? K - 1 : 1;
    // the addresses of weights and variances: a scalar base (the wave's first lane, then the row of (input, age)) and one 32-bit
    // offset per lane -- a wave spans at most 63 / bins + 2 output rows, so the offset stays below (63 + 2 bins) J floats.  The
    // history and the references are the same for every output: a scalar row and the lane's bin.
    const int o0 = __builtin_amdgcn_readfirstlane(g0 / bins), k0 = __builtin_amdgcn_readfirstlane(g0 - (g0 / bins) * bins);
    const size_t wbase = (size_t)o0 * J * bins + k0;
    const unsigned woff = 4u * (unsigned)((o - o0) * J * bins + (k - k0)), koff = 4u * (unsigned)k;
    float wr[JC], wi[JC], xr[JC], xi[JC], P[JC];                          // xr[q I + i] = x_i[m - q] behind frame m's shift
#pragma unroll
    for (int j = 0; j < JC; j++) wr[j] = wi[j] = xr[j] = xi[j] = P[j] = 0.f;
    BANDS_WALK(j, JC, J) {
        const int q = j / I, i = j - q * I;
        const size_t wrow = ((size_t)i * K + q) * bins;                   // weights and variances [O][I][K][bins]
        wr[j] = bands_ld(wre + wbase + wrow, woff);
        wi[j] = bands_ld(wim + wbase + wrow, woff);
        P[j] = bands_ld(var + wbase + wrow, woff);
        if (j + I < J) {                                                  // x_i[-1 - q]: shifted to age q + 1 by the first frame
            const size_t hrow = ((size_t)i * H + q) * bins;               // history [I][H][bins]
            xr[j] = bands_ld(hin_re + hrow, koff);
            xi[j] = bands_ld(hin_im + hrow, koff);
        }
    }
    float psi = noise[g];
    const size_t fb = (size_t)frames * bins;                              // a row of x, d, e, y
    const size_t row = (size_t)o * fb + k;                                // frame m of this lane's d, e, y: row + m bins
    float nxr[I], nxi[I], ndr = dre[row], ndi = dim[row];
#pragma unroll
    for (int i = 0; i < I; i++) {
        nxr[i] = bands_ld(xre + (size_t)i * fb, koff);
        nxi[i] = bands_ld(xim + (size_t)i * fb, koff);
    }
    // frame 0 has arrived before the loop is entered: a wait for it at the loop's head would, from frame 1 on, wait for the
    // stores of the frame before as well
#pragma unroll
    for (int i = 0; i < I; i++) asm volatile("" : : "v"(nxr[i]), "v"(nxi[i]));
    asm volatile("" : : "v"(ndr), "v"(ndi));
    for (int m = 0; m < frames; m++) {
        const size_t at = row + (size_t)m * bins;
        float cxr[I], cxi[I];
#pragma unroll
        for (int i = 0; i < I; i++) {
            cxr[i] = nxr[i];
            cxi[i] = nxi[i];
        }
        const float cdr = ndr, cdi = ndi;
        if (m + 1 < frames) {                                             // frame m + 1 flies while frame m is worked on
            const size_t next = (size_t)(m + 1) * bins;
#pragma unroll
            for (int i = 0; i < I; i++) {
                nxr[i] = bands_ld(xre + (size_t)i * fb + next, koff);
                nxi[i] = bands_ld(xim + (size_t)i * fb + next, koff);
            }
            ndr = dre[at + bins];
            ndi = dim[at + bins];
        }
        bands_shift<I>(xr, xi);                                           // every input's history moves on by one age
#pragma unroll
        for (int i = 0; i < I; i++) {
            xr[i] = cxr[i];
            xi[i] = cxi[i];
        }
        float ar = 0.f, ai = 0.f;
        BANDS_WALK(j, JC, J) {
            ar = __builtin_fmaf(wr[j], xr[j], ar);
            ar = __builtin_fmaf(-wi[j], xi[j], ar);
            ai = __builtin_fmaf(wr[j], xi[j], ai);
            ai = __builtin_fmaf(wi[j], xr[j], ai);
        }
        const float er = cdr - ar, ei = cdi - ai;
        ere[at] = er;
        eim[at] = ei;
        if (HAS_Y) {
            yre[at] = ar;
            yim[at] = ai;
        }
        if (on) {
            psi = __builtin_fmaf(kc.lam, psi, kc.oml * __builtin_fmaf(ei, ei, er * er));
            float s = psi + kc.delta;
            BANDS_WALK(j, JC, J) s = s + P[j] * __builtin_fmaf(xi[j], xi[j], xr[j] * xr[j]);
            const float r = 1.f / s;
            const float gr = er * r, gi = ei * r;
            BANDS_WALK(j, JC, J) {
                const float u = P[j] * __builtin_fmaf(xi[j], xi[j], xr[j] * xr[j]);
                const float kr = gr * P[j], ki = gi * P[j];
                wr[j] = __builtin_fmaf(kr, xr[j], wr[j]);
                wr[j] = __builtin_fmaf(ki, xi[j], wr[j]);
                wi[j] = __builtin_fmaf(ki, xr[j], wi[j]);
                wi[j] = __builtin_fmaf(-kr, xi[j], wi[j]);
                float cj = 1.f - u * r;
                cj = cj < 0.f ? 0.f : cj;
                P[j] = __builtin_fmaf(kc.omA2, __builtin_fmaf(wi[j], wi[j], wr[j] * wr[j]), (kc.A2 * cj) * P[j]);
            }
        }
    }
    BANDS_WALK(j, JC, J) {
        const int q = j / I, i = j - q * I;
        const size_t wrow = ((size_t)i * K + q) * bins;
        bands_st(wre + wbase + wrow, woff, wr[j]);                        // (a frozen output's come back with the bits they had)
        bands_st(wim + wbase + wrow, woff, wi[j]);
        bands_st(var + wbase + wrow, woff, P[j]);
    }
    noise[g] = psi;
    if (o == 0) {                                                         // one writer per element of the other history buffer
        BANDS_WALK(j, JC, J) {
            if (j + I < J) {                                              // x_i[last - q] is the next call's x_i[-1 - q]
                const int q = j / I, i = j - q * I;
                const size_t hrow = ((size_t)i * H + q) * bins;
                bands_st(hout_re + hrow, koff, xr[j]);
                bands_st(hout_im + hrow, koff, xi[j]);
            }
        }
    }
}
static int mkal_ceiling(int entries) { return bands_ceiling(entries, MKAL_LOWEST, MKAL_MAX_ENTRIES); }

static int mkal_shape(const char *who, int inputs, int outputs, int bins, int taps)
{
    const bands_dim dims[] = { { "inputs", inputs, MKAL_MAX_INPUTS }, { "outputs", outputs, 4096 }, { "bins", bins, 4097 },
                               { "taps", taps, MKAL_MAX_ENTRIES } };
    return bands_shape(who, dims, 4, inputs < 1 || taps < 1 || inputs * taps <= MKAL_MAX_ENTRIES);
}

struct mkal_args {
    const float *xre, *xim, *dre, *dim;
    float *ere, *eim, *yre, *yim, *wre, *wim;
    const float *hin_re, *hin_im;
    float *hout_re, *hout_im, *var, *noise;
    const int *adapt;
    mkal_consts kc;
    int lanes, bins, taps, frames;
    hipStream_t stream;
};

template <int I, int JC, bool HAS_Y> static void mkal_launch_as(const mkal_args &a)
{
    const dim3 grid(bands_grid(a.lanes)), block(BANDS_THREADS);
    hipLaunchKernelGGL((k_bands_matrix_kalman<I, JC, HAS_Y>), grid, block, 0, a.stream, a.xre, a.xim, a.dre, a.dim, a.ere, a.eim,
                       a.yre, a.yim, a.wre, a.wim, a.hin_re, a.hin_im, a.hout_re, a.hout_im, a.var, a.noise, a.adapt, a.kc,
                       a.lanes, a.bins, a.taps, a.frames);
}

template <int I> static void mkal_launch(const mkal_args &a)
{
#define MKAL_CASE(JC)                                                                                                     \
    case JC:                                                                                                              \
        if (a.yre) mkal_launch_as<I, JC, true>(a);                                                                        \
        else mkal_launch_as<I, JC, false>(a);                                                                             \
        break
    switch (mkal_ceiling(I * a.taps)) {
        MKAL_CASE(8);
        MKAL_CASE(16);
    default:
        MKAL_CASE(32);
    }
#undef MKAL_CASE
}

} // namespace

extern "C" int llzs_mkalman_bands_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                                      float *eim, float *yre, float *yim, float *wre, float *wim, const float *hin_re,
                                      const float *hin_im, float *hout_re, float *hout_im, float *var, float *noise,
                                      const int *adapt, const float *consts, int inputs, int outputs, int bins, int taps,
                                      int frames, void *stream)
{
    const char *who = "mkalman_bands_f32";
    if (!xre || !xim || !dre || !dim || !ere || !eim || !yre != !yim || !wre || !wim || !hin_re || !hin_im || !hout_re ||
        !hout_im || !var || !noise || !adapt || !consts || frames < 1 || (long)frames * bins > 2147483647L) {
        llzs_set_error("%s: bad arguments", who);
        return LLZ_ERR_ARG;
    }
    if (hin_re == hout_re || hin_im == hout_im) {
        llzs_set_error("%s: the history may not be updated in place (every output reads it)", who);
        return LLZ_ERR_ARG;
    }
    const int rc = mkal_shape(who, inputs, outputs, bins, taps);
    if (rc != LLZ_OK) return rc;
    const mkal_args a = { xre, xim, dre, dim, ere, eim, yre, yim, wre, wim, hin_re, hin_im, hout_re, hout_im, var, noise, adapt,
                          { consts[0], consts[1], consts[2], consts[3], consts[4] },
                          outputs * bins /* at most 4096 x 4097 */, bins, taps, frames, as_stream(stream) };
    switch (inputs) {
    case 1: mkal_launch<1>(a); break;
    case 2: mkal_launch<2>(a); break;
    case 3: mkal_launch<3>(a); break;
    case 4: mkal_launch<4>(a); break;
    case 5: mkal_launch<5>(a); break;
    case 6: mkal_launch<6>(a); break;
    case 7: mkal_launch<7>(a); break;
    default: mkal_launch<8>(a); break;
    }
    LLZ_LAUNCH_CHECK("k_bands_matrix_kalman");
    return LLZ_OK;
}

extern "C" int llzs_mkalman_bands_plan(int inputs, int outputs, int bins, int taps, int *out)
{
    const char *who = "mkalman_bands_plan";
    int rc = bands_no_out(who, out);
    if (rc == LLZ_OK) rc = mkal_shape(who, inputs, outputs, bins, taps);
    if (rc == LLZ_OK) {
        out[0] = inputs;
        bands_plan_tail(out + 1, mkal_ceiling(inputs * taps), outputs * bins);
    }
    return rc;
}
