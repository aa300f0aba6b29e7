// adapt_bands_matrix.hip -- llz_adapt_bands_matrix_mc (include/llz_adapt_bands_matrix.h): a normalised LMS filter of I references
// x K complex taps for every (output, bin) of a batch of band signals, float32, one launch per call whatever its frames.
//
//   k_bands_matrix_nlms<I, JC, HAS_Y>   a lane owns one (output, bin): lane g = o bins + k, so a wave's loads and stores of a frame
//                      are contiguous and a wave straddles output rows where bins is no multiple of 64.  The lane loads its J = I K
//                      weights and the I (K - 1) history values of its bin, walks the call's frames with frame m + 1 (I values of x,
//                      one of d) requested while frame m is worked on, and stores its weights back behind the last frame.
// Weights and regressor are register arrays of JC = the entry ceiling of the instance (8, 16, 32, 64) entries each.  Entry
// j = q I + i holds age q of input i: xr[q I + i] = x_i[m - q], so the walk "q ascending, within a q i ascending" of the header is
// j ascending, every loop over j is unrolled and every index is a constant.  Between frames every input's history moves on by one
// age, a shift by I registers: hence I is a template parameter.  Entries j >= J do not exist: the guards below are scalar (J is
// the launch's), and an instance's lower half needs none, since J > JC / 2 selects it (JC = 8: J >= I).
//
// The history is SHARED by the outputs: the lanes of outputs 0 .. O - 1 all read x_i's history of bin k.  It is therefore never
// updated in place: the kernel reads hin and the lanes of output 0 alone -- one lane per (input, age, bin) -- write hout, another
// buffer; the host swaps the two behind a launch.  No element has two writers, and no workgroup can read what this launch wrote.
//
// The sums, all in float32 with every fused multiply-add written out (contraction is off), j ascending from an accumulator of 0,
// are those of adapt_bands.hip with the regressor in the place of the one reference's history:
//   y_re = fma(-w_im[j], x_im[j], fma(w_re[j], x_re[j], y_re));   y_im = fma(w_im[j], x_re[j], fma(w_re[j], x_im[j], y_im))
//   p    = fma(x_im[j], x_im[j], fma(x_re[j], x_re[j], p))        the JOINT power of all references
//   g    = (mu e) / (p + delta), a product and a correctly rounded quotient per component
//   w_re[j] = fma(g_im, x_im[j], fma(g_re, x_re[j], w_re[j]));    w_im[j] = fma(-g_re, x_im[j], fma(g_im, x_re[j], w_im[j]))
// With I = 1 this is k_bands_nlms instruction for instruction in every sum, and its bits.
#include "bands_steps.hpp"

namespace {

constexpr int BMX_MAX_INPUTS = 8, BMX_LOWEST = 8, BMX_MAX_ENTRIES = 64;   // (the entry ceilings of the instances: 8 .. 64)

template <int I, int JC, bool HAS_Y>
__global__ void __launch_bounds__(BANDS_THREADS)
k_bands_matrix_nlms(const float *__restrict__ xre, const float *__restrict__ xim, const float *__restrict__ dre,
                    const float *__restrict__ dim, float *__restrict__ ere, float *__restrict__ eim, float *__restrict__ yre,
                    float *__restrict__ yim, float *__restrict__ wre, float *__restrict__ wim, const float *__restrict__ hin_re,
                    const float *__restrict__ hin_im, float *__restrict__ hout_re, float *__restrict__ hout_im,
                    const float *__restrict__ mu, float delta, int lanes, int bins, int K, int frames)
{
#pragma clang fp contract(off)
    constexpr int LIVE = bands_live<JC, BMX_LOWEST, I>::value;
    const int g0 = (int)blockIdx.x * BANDS_THREADS, g = g0 + (int)threadIdx.x;
    if (g >= lanes) return;
    const int o = g / bins, k = g - o * bins;
    const float step = mu[o];
    const int J = I * K, H = K > 1 ? K - 1 : 1;
    // the weights' addresses: a scalar base (the wave's first lane, then the row of (input, age)) and one 32-bit offset per lane
    // -- a wave spans at most 63 / bins + 2 output rows, so the offset stays below (63 + 2 bins) J floats.  The history and the
    // references are the same for every output: a scalar row and the lane's bin.
    const int o0 = __builtin_amdgcn_readfirstlane(g0 / bins), k0 = __builtin_amdgcn_readfirstlane(g0 - (g0 / bins) * bins);
    const size_t wbase = (size_t)o0 * J * bins + k0;
    const unsigned woff = 4u * (unsigned)((o - o0) * J * bins + (k - k0)), koff = 4u * (unsigned)k;
    float wr[JC], wi[JC], xr[JC], xi[JC];                                 // xr[q I + i] = x_i[m - q] behind frame m's shift
#pragma unroll
    for (int j = 0; j < JC; j++) wr[j] = wi[j] = xr[j] = xi[j] = 0.f;
    BANDS_WALK(j, JC, J) {
        const int q = j / I, i = j - q * I;
        const size_t wrow = ((size_t)i * K + q) * bins;                   // weights [O][I][K][bins]
        wr[j] = bands_ld(wre + wbase + wrow, woff);
        wi[j] = bands_ld(wim + wbase + wrow, woff);
        if (j + I < J) {                                                  // x_i[-1 - q]: shifted to age q + 1 by the first frame
            const size_t hrow = ((size_t)i * H + q) * bins;               // history [I][H][bins]
            xr[j] = bands_ld(hin_re + hrow, koff);
            xi[j] = bands_ld(hin_im + hrow, koff);
        }
    }
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
        float ar = 0.f, ai = 0.f, p = 0.f;                                // y and the joint power take their term of entry j
        BANDS_WALK(j, JC, J) {
            ar = __builtin_fmaf(wr[j], xr[j], ar);
            ar = __builtin_fmaf(-wi[j], xi[j], ar);
            ai = __builtin_fmaf(wr[j], xi[j], ai);
            ai = __builtin_fmaf(wi[j], xr[j], ai);
            p = __builtin_fmaf(xr[j], xr[j], p);
            p = __builtin_fmaf(xi[j], xi[j], p);
        }
        const float er = cdr - ar, ei = cdi - ai;
        ere[at] = er;
        eim[at] = ei;
        if (HAS_Y) {
            yre[at] = ar;
            yim[at] = ai;
        }
        if (step != 0.f) {
            const float den = p + delta;
            const float gr = (step * er) / den, gi = (step * ei) / den;
            BANDS_WALK(j, JC, J) {
                wr[j] = __builtin_fmaf(gr, xr[j], wr[j]);
                wr[j] = __builtin_fmaf(gi, xi[j], wr[j]);
                wi[j] = __builtin_fmaf(gi, xr[j], wi[j]);
                wi[j] = __builtin_fmaf(-gr, xi[j], wi[j]);
            }
        }
    }
    BANDS_WALK(j, JC, J) {
        const int q = j / I, i = j - q * I;
        const size_t wrow = ((size_t)i * K + q) * bins;
        bands_st(wre + wbase + wrow, woff, wr[j]);
        bands_st(wim + wbase + wrow, woff, wi[j]);
    }
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
static int bmx_ceiling(int entries) { return bands_ceiling(entries, BMX_LOWEST, BMX_MAX_ENTRIES); }

static int bmx_shape(const char *who, int inputs, int outputs, int bins, int taps)
{
    const bands_dim dims[] = { { "inputs", inputs, BMX_MAX_INPUTS }, { "outputs", outputs, 4096 }, { "bins", bins, 4097 },
                               { "taps", taps, BMX_MAX_ENTRIES } };
    return bands_shape(who, dims, 4, inputs < 1 || taps < 1 || inputs * taps <= BMX_MAX_ENTRIES);
}

struct bmx_args {
    const float *xre, *xim, *dre, *dim;
    float *ere, *eim, *yre, *yim, *wre, *wim;
    const float *hin_re, *hin_im;
    float *hout_re, *hout_im;
    const float *mu;
    float delta;
    int lanes, bins, taps, frames;
    hipStream_t stream;
};

template <int I, int JC, bool HAS_Y> static void bmx_launch_as(const bmx_args &a)
{
    const dim3 grid(bands_grid(a.lanes)), block(BANDS_THREADS);
    hipLaunchKernelGGL((k_bands_matrix_nlms<I, JC, HAS_Y>), grid, block, 0, a.stream, a.xre, a.xim, a.dre, a.dim, a.ere, a.eim,
                       a.yre, a.yim, a.wre, a.wim, a.hin_re, a.hin_im, a.hout_re, a.hout_im, a.mu, a.delta, a.lanes, a.bins, a.taps,
                       a.frames);
}

template <int I> static void bmx_launch(const bmx_args &a)
{
#define BMX_CASE(JC)                                                                                                      \
    case JC:                                                                                                              \
        if (a.yre) bmx_launch_as<I, JC, true>(a);                                                                         \
        else bmx_launch_as<I, JC, false>(a);                                                                              \
        break
    switch (bmx_ceiling(I * a.taps)) {
        BMX_CASE(8);
        BMX_CASE(16);
        BMX_CASE(32);
    default:
        BMX_CASE(64);
    }
#undef BMX_CASE
}

} // namespace

extern "C" int llzs_matrix_bands_nlms_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                                          float *eim, float *yre, float *yim, float *wre, float *wim, const float *hin_re,
                                          const float *hin_im, float *hout_re, float *hout_im, const float *mu, float delta,
                                          int inputs, int outputs, int bins, int taps, int frames, void *stream)
{
    const char *who = "bands_matrix_nlms_f32";
    if (!xre || !xim || !dre || !dim || !ere || !eim || !yre != !yim || !wre || !wim || !hin_re || !hin_im || !hout_re ||
        !hout_im || !mu || frames < 1 || (long)frames * bins > 2147483647L) {
        llzs_set_error("%s: bad arguments", who);
        return LLZ_ERR_ARG;
    }
    if (hin_re == hout_re || hin_im == hout_im) {
        llzs_set_error("%s: the history may not be updated in place (every output reads it)", who);
        return LLZ_ERR_ARG;
    }
    const int rc = bmx_shape(who, inputs, outputs, bins, taps);
    if (rc != LLZ_OK) return rc;
    const bmx_args a = { xre, xim, dre, dim, ere, eim, yre, yim, wre, wim, hin_re, hin_im, hout_re, hout_im, mu, delta,
                         outputs * bins /* at most 4096 x 4097 */, bins, taps, frames, as_stream(stream) };
    switch (inputs) {
    case 1: bmx_launch<1>(a); break;
    case 2: bmx_launch<2>(a); break;
    case 3: bmx_launch<3>(a); break;
    case 4: bmx_launch<4>(a); break;
    case 5: bmx_launch<5>(a); break;
    case 6: bmx_launch<6>(a); break;
    case 7: bmx_launch<7>(a); break;
    default: bmx_launch<8>(a); break;
    }
    LLZ_LAUNCH_CHECK("k_bands_matrix_nlms");
    return LLZ_OK;
}

extern "C" int llzs_matrix_bands_nlms_plan(int inputs, int outputs, int bins, int taps, int *out)
{
    const char *who = "bands_matrix_nlms_plan";
    int rc = bands_no_out(who, out);
    if (rc == LLZ_OK) rc = bmx_shape(who, inputs, outputs, bins, taps);
    if (rc == LLZ_OK) {
        out[0] = inputs;
        bands_plan_tail(out + 1, bmx_ceiling(inputs * taps), outputs * bins);
    }
    return rc;
}
