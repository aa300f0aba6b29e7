// corr.hip -- auto / cross correlation kernels (reference libllzfilter/llz_corr.c:38-177).
//
//  k_corr_exact_f64    one lane per lag, the reference's running sum in its order (rounded multiply, rounded add):
//                      bit-identical to llz_autocorr / llz_crosscorr; also the three sums of llz_corr_cof.
//  k_autocorr_mc_f32   one wave per frame, 512-sample chunks in the wave's private LDS, register sliding window
//                      (64 FMAs per two ds_read_b128), partial sums in registers, one DPP reduction per frame.
//                      CROSS: the window is staged from a second row (llz_crosscorr_mc); the negative lags of a two-sided
//                      result are the same kernel with the rows swapped, storing downwards.
//  k_corr_cof_mc_f32   <a,b>, <a,a>, <b,b> of a frame pair in one pass (the chunks of the lag-0 register form), one quotient
//                      in double per frame.
//  k_xcf_pack / k_xcf_product / k_xcf_extract
//                      the pointwise steps of the FFT cross-correlation: z = x + i y zero-padded, conj(X) Y from Z[k] and
//                      conj(Z[F-k]), lags -p..p from the inverse transform.
//  k_acf_pack / k_acf_power / k_acf_extract
//                      the pointwise steps of the FFT form around the batched float32 FFT of fft.hip:
//                      zero-padded real -> complex, |X|^2 of the FIRST n bins (the reference's definition), 2*Re.
#include "common.hpp"
#include "acf_reg.hpp"

namespace {

__global__ void __launch_bounds__(64)
k_corr_exact_f64(const double *__restrict__ x, const double *__restrict__ y, int n, int p, double *__restrict__ r)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k > p) return;
    double acc = 0.0;
    for (int i = 0; i + k < n; i++) {
        const double prod = x[i] * y[i + k];
        acc = acc + prod;
    }
    r[k] = acc;
}

// Direct autocorrelation of many frames.  A WAVE owns a frame (frames are dealt round robin to the waves of a
// persistent grid) and walks it in chunks of 512 samples: the chunk plus p samples of look-ahead is staged in the wave's
// private LDS (coalesced dword loads, no workgroup barrier), lane l keeps x[8l .. 8l+7] in registers and slides a
// 15-sample window over the lags, 8 lags at a time: 64 FMAs per two ds_read_b128 -- the register-window scheme of
// fir_td.hip with the frame itself in the role of the taps.  Per-lane partial sums live in registers for the whole
// frame and are reduced across the wave once per frame with DPP adds.
constexpr int AC_WAVES = 4;
constexpr int AC_CHUNK = 512;                 // samples per wave and step: 8 per lane
constexpr int AC_MAXLAG = 256;                // p <= 255
constexpr int AC_LDS = (AC_CHUNK + AC_MAXLAG + 16) + ((AC_CHUNK + AC_MAXLAG + 16) >> 3) * 4;   // padded image

__device__ __forceinline__ int ac_phys(int p) { return p + ((p >> 3) << 2); }

// Where a launch stores: lag k of frame f goes to r[f * stride + base + sign * k] (one-sided: stride p + 1, base 0, sign 1; a
// two-sided row has 2 p + 1 entries with lag 0 at index p: base p, sign 1 for the positive and -1 for the negative lags).
struct ac_out {
    long stride;
    int base, sign;
};

// This launch does lags lag0 + wshift .. lag0 + wshift + 8 NG - 1 of sum_i x[i] * w[i + k], w = CROSS ? y : x.  The window is
// staged `wshift` samples further on (0 or 1; 1 only with CROSS): the negative side of a two-sided result starts at lag 1 (its
// lag 0 is the positive side's) while lag0 stays a multiple of 8, which the 16-byte window reads need.
template <int NG, bool CROSS>                   // lag groups of 8 kept in registers
__global__ void __launch_bounds__(64 * AC_WAVES)
k_autocorr_mc_f32(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ r, int frames, int n, int p,
                  int lag0, int wshift, ac_out o)
{
    __shared__ __attribute__((aligned(16))) float lds_ac[AC_WAVES][AC_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *xs = lds_ac[wave];
    const long waves_total = (long)gridDim.x * AC_WAVES;
    const int look = lag0 + 8 * NG;                            // look-ahead samples a chunk needs behind its end
    const int ws = CROSS ? wshift : 0;
    for (long f = (long)blockIdx.x * AC_WAVES + wave; f < frames; f += waves_total) {
        const float *row = x + (size_t)f * n;
        const float *wrow = CROSS ? y + (size_t)f * n : row;   // the row the window slides over
        float acc[8 * NG];
#pragma unroll
        for (int k = 0; k < 8 * NG; k++) acc[k] = 0.f;
        for (int c0 = 0; c0 < n; c0 += AC_CHUNK) {
            // stage w[c0 + wshift .. c0 + wshift + 512 + look): zeros behind the end of the frame make those products vanish
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the previous step's reads are done
            for (int i = lane; i < AC_CHUNK + look; i += 64) {
                const int idx = c0 + ws + i;
                xs[ac_phys(i)] = idx < n ? wrow[idx] : 0.f;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int p0 = lane * 8;
            float xl[8], wa[8], wb[8];
            auto load8 = [&](float (&w)[8], int q) {
                const float4 a = *reinterpret_cast<const float4 *>(&xs[ac_phys(q)]);
                const float4 b = *reinterpret_cast<const float4 *>(&xs[ac_phys(q + 4)]);
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
                w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            };
            if (CROSS) acf_fetch8<false>(row, nullptr, n, c0 + p0, xl);      // the lane's own samples: the x row
            else load8(xl, p0);
            load8(wa, p0 + lag0);
            // lag group g: lags 8g .. 8g+7 need w[p0 + 8g .. p0 + 8g + 14] = (wa | wb) with wb = the next 8 samples
#pragma unroll
            for (int g = 0; g < NG; g++) {
                load8(wb, p0 + lag0 + 8 * g + 8);
#pragma unroll
                for (int kk = 0; kk < 8; kk++)
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int slot = j + kk;                           // 0..14
                        acc[8 * g + kk] = __builtin_fmaf(xl[j], slot < 8 ? wa[slot] : wb[slot - 8], acc[8 * g + kk]);
                    }
#pragma unroll
                for (int j = 0; j < 8; j++) wa[j] = wb[j];
            }
        }
        int k;
        const float v = wave_sums(acc, lane, &k);
        const int lag = lag0 + ws + k;
        if (k < 8 * NG && lag <= p) r[(size_t)f * o.stride + o.base + o.sign * lag] = v;
    }
}

// Direct correlation for SHORT lag ranges (p <= 8 NL <= 32: the LPC orders) without LDS: the register form of one frame
// (acf_reg_frame in acf_reg.hpp: 8 samples per lane, the look-ahead through the wave shuffle, 8 (p + 1) FMAs per lane and
// chunk); the per-lane partial sums are reduced across the wave once per frame.  (The LDS form
// above -- staging, two waits and the window reads per 512 samples, nothing in flight meanwhile -- measured 0.93 ms for 2^18
// frames of 1024 at p = 16; this one is bound by the reduction and the FMAs.)  CROSS: sum_i x[i] * y[i + k]; K0 = 1: lags 1..p.
template <int NL, bool CROSS, int K0>
__global__ void __launch_bounds__(64 * AC_WAVES)
k_autocorr_reg_f32(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ r, int frames, int n, int p,
                   ac_out o)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves_total = (long)gridDim.x * AC_WAVES;
    for (long f = (long)blockIdx.x * AC_WAVES + wave; f < frames; f += waves_total) {
        float acc[8 * NL + 1 - K0];
        acf_reg_frame<NL, false, CROSS, K0>(x + (size_t)f * n, nullptr, n, lane, acc, CROSS ? y + (size_t)f * n : nullptr);
        int k;
        const float v = wave_sums(acc, lane, &k);
        if (K0 + k <= p) r[(size_t)f * o.stride + o.base + o.sign * (K0 + k)] = v;
    }
}

// The correlation coefficient of `frames` pairs of rows: one pass over a and b, three float32 sums per lane in the chunks of the
// lag-0 register form (8 samples per lane, 63 lanes, the next chunk requested first), one reduction per frame,
// and the quotient in double, so that exact sums give the reference's own value (llz_corr.c:61-78); 0 / 0 = NaN as there.
__global__ void __launch_bounds__(64 * AC_WAVES)
k_corr_cof_mc_f32(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ c, int frames, int n)
{
    constexpr int STEP = 8 * 63;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long waves_total = (long)gridDim.x * AC_WAVES;
    const bool active = lane < 63;
    for (long f = (long)blockIdx.x * AC_WAVES + wave; f < frames; f += waves_total) {
        const float *ra = a + (size_t)f * n, *rb = b + (size_t)f * n;
        float acc[3] = {0.f, 0.f, 0.f};                                  // <a,b>, <a,a>, <b,b>
        float ca[8], cb[8], na[8], nb[8];
        acf_fetch8<false>(ra, nullptr, n, 8 * lane, ca);
        acf_fetch8<false>(rb, nullptr, n, 8 * lane, cb);
        for (int c0 = 0; c0 < n; c0 += STEP) {
            const bool more = c0 + STEP < n;
            if (more) {
                acf_fetch8<false>(ra, nullptr, n, c0 + STEP + 8 * lane, na);
                acf_fetch8<false>(rb, nullptr, n, c0 + STEP + 8 * lane, nb);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float va = active ? ca[j] : 0.f, vb = active ? cb[j] : 0.f;
                acc[0] = __builtin_fmaf(va, vb, acc[0]);
                acc[1] = __builtin_fmaf(va, va, acc[1]);
                acc[2] = __builtin_fmaf(vb, vb, acc[2]);
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < 8; j++) { ca[j] = na[j]; cb[j] = nb[j]; }
            }
        }
        int k;
        const float v = wave_sums(acc, lane, &k);                        // sum s ends in the lane whose six bits, reversed, are s
        const float ab = __shfl(v, 0, 64), aa = __shfl(v, 32, 64), bb = __shfl(v, 16, 64);
        if (lane == 0) c[f] = (float)((double)ab / sqrt((double)aa * (double)bb));
    }
}

// zero-padded real frame -> interleaved complex of length F
__global__ void __launch_bounds__(256)
k_acf_pack(const float *__restrict__ x, float2 *__restrict__ z, int n, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;                  // flat index over frames x F
    if (e >= total) return;
    const long f = e / F;
    const int i = (int)(e - f * F);
    z[e] = make_float2(i < n ? x[f * n + i] : 0.f, 0.f);
}

// power spectrum of the first n bins, zero elsewhere (llz_corr.c:165-170)
__global__ void __launch_bounds__(256)
k_acf_power(float2 *__restrict__ z, int n, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % F);
    const float2 v = z[e];
    z[e] = make_float2(i < n ? __builtin_fmaf(v.x, v.x, v.y * v.y) : 0.f, 0.f);
}

__global__ void __launch_bounds__(256)
k_acf_extract(const float2 *__restrict__ z, float *__restrict__ r, int p, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;                  // flat index over frames x (p+1)
    if (e >= total) return;
    const long f = e / (p + 1);
    const int k = (int)(e - f * (p + 1));
    r[e] = z[f * F + k].x * 2.f;                                          // llz_corr.c:173
}

// FFT cross-correlation, step 1: z = x + i y, zero-padded to F points
__global__ void __launch_bounds__(256)
k_xcf_pack(const float *__restrict__ x, const float *__restrict__ y, float2 *__restrict__ z, int n, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;                  // flat index over frames x F
    if (e >= total) return;
    const long f = e / F;
    const int i = (int)(e - f * F);
    z[e] = i < n ? make_float2(x[f * n + i], y[f * n + i]) : make_float2(0.f, 0.f);
}

// step 2: x and y are real, so X[k] = (Z[k] + conj(Z[F-k])) / 2 and Y[k] = (Z[k] - conj(Z[F-k])) / 2i; the spectrum of
// r[k] = sum_i x[i] y[i+k] is conj(X) Y, Hermitian because r is real.  A thread owns the pair of bins (k, F - k), in place.
__global__ void __launch_bounds__(256)
k_xcf_product(float2 *__restrict__ z, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;                  // flat index over frames x (F/2 + 1)
    if (e >= total) return;
    const int half = F / 2 + 1;
    const long f = e / half;
    const int k = (int)(e - f * half), k2 = (F - k) & (F - 1);
    float2 *zf = z + f * F;
    const float2 a = zf[k], b = zf[k2];
    const float xr = 0.5f * (a.x + b.x), xi = 0.5f * (a.y - b.y);
    const float yr = 0.5f * (a.y + b.y), yi = 0.5f * (b.x - a.x);
    const float rr = __builtin_fmaf(xr, yr, xi * yi), ri = __builtin_fmaf(xr, yi, -(xi * yr));
    zf[k] = make_float2(rr, ri);
    if (k2 != k) zf[k2] = make_float2(rr, -ri);
}

// step 3, after the inverse transform: lag k >= 0 sits at bin k, lag -k at bin F - k
__global__ void __launch_bounds__(256)
k_xcf_extract(const float2 *__restrict__ z, float *__restrict__ r, int p, int two_sided, int F, long total)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;                  // flat index over frames x (p+1 or 2p+1)
    if (e >= total) return;
    const int width = two_sided ? 2 * p + 1 : p + 1;
    const long f = e / width;
    const int lag = (int)(e - f * width) - (two_sided ? p : 0);
    r[e] = z[f * F + (lag >= 0 ? lag : F + lag)].x;
}

} // namespace

extern "C" int llzs_corr_exact_f64(const double *x, const double *y, int n, int p, double *r, void *stream)
{
    if (!x || !y || !r || n < 1 || p < 0) {
        llzs_set_error("corr_exact_f64: bad arguments");
        return LLZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_corr_exact_f64, dim3((unsigned)(p / 64 + 1)), dim3(64), 0, as_stream(stream), x, y, n, p, r);
    LLZ_LAUNCH_CHECK("k_corr_exact_f64");
    return LLZ_OK;
}

// lags k0 .. p of sum_i x[f][i] * w[f][i + k] for every frame, stored where `o` says.  cross = 0: w is x itself (the one-row
// kernels); k0 = 1 (with cross): the negative side of a two-sided result.  The path choice is the autocorrelation's: the
// register form for p <= 32, the LDS window above it (or always, with acf_lds = 1), 64 lags per launch.
static int corr_mc_pass(const float *x, const float *w, float *r, int frames, int n, int p, int cross, int k0, ac_out o,
                        void *stream)
{
    long blocks = ((long)frames + AC_WAVES - 1) / AC_WAVES;
    if (blocks > 256L * 4) blocks = 256L * 4;                       // persistent: frames dealt round robin to the waves
    if (p <= 32 && llzs_tune(LLZS_TUNE_ACF_LDS) < 1) {              // short lag ranges: the register form
        const int nl = p <= 8 ? 1 : (p + 7) / 8;
#define LLZ_AC_REG(NLV, CROSSV, K0V)                                                                              \
    hipLaunchKernelGGL((k_autocorr_reg_f32<NLV, CROSSV, K0V>), dim3((unsigned)blocks), dim3(64 * AC_WAVES), 0,     \
                       as_stream(stream), x, w, r, frames, n, p, o)
#define LLZ_AC_REG_NL(CROSSV, K0V)                                                                                \
    do {                                                                                                          \
        if (nl == 1) LLZ_AC_REG(1, CROSSV, K0V);                                                                  \
        else if (nl == 2) LLZ_AC_REG(2, CROSSV, K0V);                                                             \
        else if (nl == 3) LLZ_AC_REG(3, CROSSV, K0V);                                                             \
        else LLZ_AC_REG(4, CROSSV, K0V);                                                                          \
    } while (0)
        if (!cross) LLZ_AC_REG_NL(false, 0);
        else if (k0 == 0) LLZ_AC_REG_NL(true, 0);
        else LLZ_AC_REG_NL(true, 1);
#undef LLZ_AC_REG_NL
#undef LLZ_AC_REG
        LLZ_LAUNCH_CHECK("k_autocorr_reg_f32");
        return LLZ_OK;
    }
    // lags are done 64 per launch (8 groups of 8 accumulators per lane); p > 63 re-reads the frames per block of lags
#define LLZ_AC_LAUNCH(NG, LAG0)                                                                                   \
    do {                                                                                                          \
        if (cross)                                                                                                \
            hipLaunchKernelGGL((k_autocorr_mc_f32<NG, true>), dim3((unsigned)blocks), dim3(64 * AC_WAVES), 0,      \
                               as_stream(stream), x, w, r, frames, n, p, LAG0, k0, o);                            \
        else                                                                                                      \
            hipLaunchKernelGGL((k_autocorr_mc_f32<NG, false>), dim3((unsigned)blocks), dim3(64 * AC_WAVES), 0,     \
                               as_stream(stream), x, w, r, frames, n, p, LAG0, 0, o);                             \
    } while (0)
    for (int lag0 = 0; lag0 + k0 <= p; lag0 += 64) {
        const int last = p - lag0 - k0;                             // lags of this launch: lag0 + k0 + (0 .. min(last, 63))
        const int ng = ((last < 63 ? last : 63) + 8) / 8;
        if (ng <= 1) LLZ_AC_LAUNCH(1, lag0);
        else if (ng <= 2) LLZ_AC_LAUNCH(2, lag0);
        else if (ng <= 3) LLZ_AC_LAUNCH(3, lag0);
        else if (ng <= 4) LLZ_AC_LAUNCH(4, lag0);
        else if (ng <= 5) LLZ_AC_LAUNCH(5, lag0);
        else LLZ_AC_LAUNCH(8, lag0);
    }
#undef LLZ_AC_LAUNCH
    LLZ_LAUNCH_CHECK("k_autocorr_mc_f32");
    return LLZ_OK;
}

extern "C" int llzs_autocorr_mc_f32(const float *x, float *r, int frames, int n, int p, void *stream)
{
    if (!x || !r || frames < 1 || n < 1 || p < 0 || p >= n || p > 255) {
        llzs_set_error("autocorr_mc_f32: bad arguments (frames=%d n=%d p=%d; p < n, p <= 255)", frames, n, p);
        return LLZ_ERR_ARG;
    }
    return corr_mc_pass(x, x, r, frames, n, p, 0, 0, ac_out{p + 1, 0, 1}, stream);
}

extern "C" int llzs_crosscorr_mc_f32(const float *x, const float *y, float *r, int frames, int n, int p, int two_sided,
                                     void *stream)
{
    if (!x || !y || !r || frames < 1 || n < 1 || p < 0 || p >= n || p > 255 || (two_sided != 0 && two_sided != 1)) {
        llzs_set_error("crosscorr_mc_f32: bad arguments (frames=%d n=%d p=%d two_sided=%d; p < n, p <= 255)", frames, n, p,
                       two_sided);
        return LLZ_ERR_ARG;
    }
    const int cross = x != y;                                       // the same row twice: the one-row kernels, the same bits
    if (!two_sided) return corr_mc_pass(x, y, r, frames, n, p, cross, 0, ac_out{p + 1, 0, 1}, stream);
    int rc = corr_mc_pass(x, y, r, frames, n, p, cross, 0, ac_out{2L * p + 1, p, 1}, stream);
    // r[-k] = sum_i y[i] * x[i + k]: the rows swapped, lags 1..p only (lag 0 is done), stored downwards from index p - 1
    if (rc == LLZ_OK && p > 0) rc = corr_mc_pass(y, x, r, frames, n, p, 1, 1, ac_out{2L * p + 1, p, -1}, stream);
    return rc;
}

extern "C" int llzs_corr_cof_mc_f32(const float *a, const float *b, float *c, int frames, int n, void *stream)
{
    if (!a || !b || !c || frames < 1 || n < 1) {
        llzs_set_error("corr_cof_mc_f32: bad arguments (frames=%d n=%d)", frames, n);
        return LLZ_ERR_ARG;
    }
    long blocks = ((long)frames + AC_WAVES - 1) / AC_WAVES;
    if (blocks > 256L * 4) blocks = 256L * 4;
    hipLaunchKernelGGL(k_corr_cof_mc_f32, dim3((unsigned)blocks), dim3(64 * AC_WAVES), 0, as_stream(stream), a, b, c, frames, n);
    LLZ_LAUNCH_CHECK("k_corr_cof_mc_f32");
    return LLZ_OK;
}

extern "C" int llzs_acf_pack(const float *x, float *z, int frames, int n, int F, void *stream)
{
    const long total = (long)frames * F;
    hipLaunchKernelGGL(k_acf_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x,
                       reinterpret_cast<float2 *>(z), n, F, total);
    LLZ_LAUNCH_CHECK("k_acf_pack");
    return LLZ_OK;
}

extern "C" int llzs_acf_power(float *z, int frames, int n, int F, void *stream)
{
    const long total = (long)frames * F;
    hipLaunchKernelGGL(k_acf_power, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<float2 *>(z), n, F, total);
    LLZ_LAUNCH_CHECK("k_acf_power");
    return LLZ_OK;
}

extern "C" int llzs_acf_extract(const float *z, float *r, int frames, int p, int F, void *stream)
{
    const long total = (long)frames * (p + 1);
    hipLaunchKernelGGL(k_acf_extract, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2 *>(z), r, p, F, total);
    LLZ_LAUNCH_CHECK("k_acf_extract");
    return LLZ_OK;
}

extern "C" int llzs_xcf_pack(const float *x, const float *y, float *z, int frames, int n, int F, void *stream)
{
    const long total = (long)frames * F;
    hipLaunchKernelGGL(k_xcf_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, y,
                       reinterpret_cast<float2 *>(z), n, F, total);
    LLZ_LAUNCH_CHECK("k_xcf_pack");
    return LLZ_OK;
}

extern "C" int llzs_xcf_product(float *z, int frames, int F, void *stream)
{
    const long total = (long)frames * (F / 2 + 1);
    hipLaunchKernelGGL(k_xcf_product, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<float2 *>(z), F, total);
    LLZ_LAUNCH_CHECK("k_xcf_product");
    return LLZ_OK;
}

extern "C" int llzs_xcf_extract(const float *z, float *r, int frames, int p, int two_sided, int F, void *stream)
{
    const long total = (long)frames * (two_sided ? 2 * p + 1 : p + 1);
    hipLaunchKernelGGL(k_xcf_extract, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2 *>(z), r, p, two_sided, F, total);
    LLZ_LAUNCH_CHECK("k_xcf_extract");
    return LLZ_OK;
}
