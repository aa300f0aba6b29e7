// dft.hip -- batched DFT of any length and zoom transform by Bluestein's chirp-z algorithm (include/llz_dft.h, host layer
// llz_dft_host.c), float32 on the staged passes of fft_core.hpp.  With the chirp c(m) (e^{-i pi m^2 / N} for the DFT) a row of
// N points becomes K outputs through two M-point transforms, M the power of two >= N + K - 1:
//   a = x . pre  (zeros up to M),  A = FFT_M(a),  B = A . V,  b = IFFT_M(B) unscaled,  X[k] = b[k] . post[k]
// pre, V = FFT_M(v) / M and post are the host's tables (built in double, rounded once): the window, the zoom's start frequency
// and the inverse's 1 / N are folded into them, so that forward, inverse and zoom are ONE kernel with other tables.
//
//   k_dft_fused_f32<MODE>   M <= 4096: a workgroup serves tpw rows (fft_make_plan), each in its own LDS image from load to
//                           store, one launch per call.  V is stored in image order (entry j = bin bitrev(j)): the forward
//                           passes leave A where the inverse passes expect B, so no reordering pass is needed (as tde.hip's
//                           weighted spectrum).  V is read from global memory, 8 M bytes shared by all rows.
//   k_dft_pack_f32<MODE>, k_dft_mul_f32, k_dft_extract_f32<REAL_OUT>
//                           the pointwise steps of the composed form around llzs_fft_f32 / llzs_fft_large_f32 on a device
//                           scratch of M complex values per row, V in natural order and unscaled (the library's inverse
//                           transform divides by M).
// MODE: DFT_CPX complex rows in and out, DFT_REAL real rows in, DFT_HERM bins 0 .. N/2 in (Hermitian extension, the imaginary
// parts of the real bins dropped) and real rows out.  The ragged last workgroup masks loads and stores, never a barrier.
#include "fft_core.hpp"

namespace {

enum { DFT_CPX = 0, DFT_REAL = 1, DFT_HERM = 2 };

struct dft_args {
    const float *in;                // [count] rows in_pitch elements apart (complex pairs; floats for DFT_REAL)
    float *out;                     // [count] rows out_pitch elements apart (complex pairs; floats for DFT_HERM)
    const float *pre, *v, *post;    // [N], [M], [K stored] complex
    long in_pitch, out_pitch;
    int count, N, K, M;             // K: outputs stored per row
};

__device__ __forceinline__ cpx<float> dft_mul(cpx<float> a, cpx<float> b)
{
    cpx<float> y;
    y.re = __builtin_fmaf(a.re, b.re, -(a.im * b.im));
    y.im = __builtin_fmaf(a.re, b.im, a.im * b.re);
    return y;
}

__device__ __forceinline__ cpx<float> dft_ld(const float *p, size_t i)
{
    const float2 t = *reinterpret_cast<const float2 *>(p + 2 * i);
    cpx<float> z;
    z.re = t.x;
    z.im = t.y;
    return z;
}

// a[m] of one row: the input sample m < N times pre[m]
template <int MODE>
__device__ __forceinline__ cpx<float> dft_take(const dft_args &a, size_t row, int m)
{
    cpx<float> x;
    if (MODE == DFT_REAL) {
        x.re = a.in[row * (size_t)a.in_pitch + m];
        x.im = 0.f;
    } else if (MODE == DFT_HERM) {
        const int half = a.N >> 1, b = m <= half ? m : a.N - m;
        x = dft_ld(a.in, row * (size_t)a.in_pitch + b);
        if (b == 0 || 2 * b == a.N) x.im = 0.f;
        else if (m > half) x.im = -x.im;
    } else {
        x = dft_ld(a.in, row * (size_t)a.in_pitch + m);
    }
    return dft_mul(x, dft_ld(a.pre, m));
}

template <int MODE>
__device__ __forceinline__ void dft_put(const dft_args &a, size_t row, int k, cpx<float> b)
{
    const cpx<float> y = dft_mul(b, dft_ld(a.post, k));
    if (MODE == DFT_HERM) a.out[row * (size_t)a.out_pitch + k] = y.re;
    else *reinterpret_cast<float2 *>(a.out + 2 * (row * (size_t)a.out_pitch + k)) = make_float2(y.re, y.im);
}

template <int MODE>
__global__ void __launch_bounds__(FFT_THREADS)
k_dft_fused_f32(dft_args a, const float *__restrict__ cs, int log2m, unsigned groups, int tpw)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    const int tid = threadIdx.x, M = a.M, tstride = fft_tstride(M), points = tpw << log2m;
    cpx<float> *tw = s + tpw * tstride;
    fft_load_twiddles(tw, cs, M, tid);
    const size_t row0 = (size_t)blockIdx.x * tpw;
    for (int i = tid; i < points; i += FFT_THREADS) {
        const int tr = i >> log2m, m = i & (M - 1);
        cpx<float> z;
        z.re = 0.f;
        z.im = 0.f;
        if (m < a.N && row0 + tr < (size_t)a.count) z = dft_take<MODE>(a, row0 + tr, m);
        s[tr * tstride + fft_phys(m)] = z;
    }
    __syncthreads();
    fft_run<arith_f32, false>(s, tpw, M, log2m, tstride, tw, groups, tid);
    for (int i = tid; i < points; i += FFT_THREADS) {                  // position j holds bin bitrev(j), and so does V
        const int tr = i >> log2m, j = i & (M - 1);
        cpx<float> *p = s + tr * tstride + fft_phys(j);
        *p = dft_mul(*p, dft_ld(a.v, j));
    }
    __syncthreads();
    fft_run<arith_f32, true>(s, tpw, M, log2m, tstride, tw, groups, tid);
    for (int i = tid; i < points; i += FFT_THREADS) {
        const int tr = i >> log2m, k = i & (M - 1);
        if (k < a.K && row0 + tr < (size_t)a.count) dft_put<MODE>(a, row0 + tr, k, s[tr * tstride + fft_phys(k)]);
    }
}

// ---- the composed form's pointwise steps: z = [count][M] complex ----
template <int MODE>
__global__ void __launch_bounds__(256) k_dft_pack_f32(dft_args a, float *__restrict__ z, int log2m)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, row = i >> log2m;
    const int m = (int)(i & (size_t)(a.M - 1));
    if (row >= (size_t)a.count) return;
    cpx<float> v;
    v.re = 0.f;
    v.im = 0.f;
    if (m < a.N) v = dft_take<MODE>(a, row, m);
    *reinterpret_cast<float2 *>(z + 2 * i) = make_float2(v.re, v.im);
}

__global__ void __launch_bounds__(256) k_dft_mul_f32(float *__restrict__ z, const float *__restrict__ v, size_t points, int M)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= points) return;
    const cpx<float> y = dft_mul(dft_ld(z, i), dft_ld(v, i & (size_t)(M - 1)));
    *reinterpret_cast<float2 *>(z + 2 * i) = make_float2(y.re, y.im);
}

template <int MODE>
__global__ void __launch_bounds__(256) k_dft_extract_f32(dft_args a, const float *__restrict__ z, int log2m)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, row = i >> log2m;
    const int k = (int)(i & (size_t)(a.M - 1));
    if (row < (size_t)a.count && k < a.K) dft_put<MODE>(a, row, k, dft_ld(z, i));
}

int dft_log2(int m)
{
    int k = 0;
    while ((1 << k) < m) k++;
    return (1 << k) == m ? k : -1;
}

// 0, or LLZ_ERR_ARG with a message: what every launcher here asks of its shape
int dft_refuse(const char *who, const void *p0, const void *p1, const void *p2, int count, int n, int k, int m, int max_log2m,
               long in_pitch, long out_pitch, int mode)
{
    const int log2m = dft_log2(m);
    if (p0 && p1 && p2 && count >= 1 && n >= 1 && k >= 1 && log2m >= 3 && log2m <= max_log2m && n <= m && k <= m && in_pitch >= 1 &&
        out_pitch >= k && mode >= DFT_CPX && mode <= DFT_HERM)
        return LLZ_OK;
    llzs_set_error("%s: bad arguments (count %d n %d k %d m %d pitches %ld, %ld mode %d)", who, count, n, k, m, in_pitch,
                   out_pitch, mode);
    return LLZ_ERR_ARG;
}

template <typename F>
void dft_pick_mode(int mode, F f)
{
    if (mode == DFT_REAL) f(std::integral_constant<int, DFT_REAL>{});
    else if (mode == DFT_HERM) f(std::integral_constant<int, DFT_HERM>{});
    else f(std::integral_constant<int, DFT_CPX>{});
}

} // namespace

extern "C" int llzs_dft_plan(int m, int count, int *out)
{
    if (dft_log2(m) < 3 || m > 4096 || count < 1 || !out) {
        llzs_set_error("llzs_dft_plan: m %d count %d (a power of two in 8..4096, count >= 1)", m, count);
        return LLZ_ERR_ARG;
    }
    const fft_plan pl = fft_make_plan<arith_f32>(m, count);
    out[0] = pl.tpw;
    out[1] = (int)pl.lds;
    return LLZ_OK;
}

extern "C" int llzs_dft_fused_f32(const float *in, float *out, const float *pre, const float *v, const float *post,
                                  const float *cs, int count, int n, int k, int m, long in_pitch, long out_pitch, int mode,
                                  void *stream)
{
    const int rc = dft_refuse("dft_fused_f32", in, out, pre && v && post ? cs : nullptr, count, n, k, m, 12, in_pitch, out_pitch, mode);
    if (rc != LLZ_OK) return rc;
    const int log2m = dft_log2(m);
    const dft_args a = {in, out, pre, v, post, in_pitch, out_pitch, count, n, k, m};
    const fft_plan pl = fft_make_plan<arith_f32>(m, count);
    dft_pick_mode(mode, [&](auto md) {
        hipLaunchKernelGGL((k_dft_fused_f32<md()>), dim3((unsigned)pl.blocks), dim3(FFT_THREADS), pl.lds, as_stream(stream), a, cs,
                           log2m, fft_groups(log2m), pl.tpw);
    });
    LLZ_LAUNCH_CHECK("k_dft_fused_f32");
    return LLZ_OK;
}

extern "C" int llzs_dft_pack_f32(const float *in, float *z, const float *pre, int count, int n, int m, long in_pitch, int mode,
                                 void *stream)
{
    const int rc = dft_refuse("dft_pack_f32", in, z, pre, count, n, 1, m, 21, in_pitch, 1, mode);
    if (rc != LLZ_OK) return rc;
    const int log2m = dft_log2(m);
    const dft_args a = {in, nullptr, pre, nullptr, nullptr, in_pitch, 0, count, n, 0, m};
    const size_t points = (size_t)count << log2m;
    dft_pick_mode(mode, [&](auto md) {
        hipLaunchKernelGGL((k_dft_pack_f32<md()>), dim3((unsigned)((points + 255) / 256)), dim3(256), 0, as_stream(stream), a, z,
                           log2m);
    });
    LLZ_LAUNCH_CHECK("k_dft_pack_f32");
    return LLZ_OK;
}

extern "C" int llzs_dft_mul_f32(float *z, const float *v, int count, int m, void *stream)
{
    const int rc = dft_refuse("dft_mul_f32", z, v, v, count, 1, 1, m, 21, 1, 1, DFT_CPX);
    if (rc != LLZ_OK) return rc;
    const size_t points = (size_t)count * (size_t)m;
    hipLaunchKernelGGL(k_dft_mul_f32, dim3((unsigned)((points + 255) / 256)), dim3(256), 0, as_stream(stream), z, v, points, m);
    LLZ_LAUNCH_CHECK("k_dft_mul_f32");
    return LLZ_OK;
}

extern "C" int llzs_dft_extract_f32(const float *z, float *out, const float *post, int count, int k, int m, long out_pitch,
                                    int mode, void *stream)
{
    const int rc = dft_refuse("dft_extract_f32", z, out, post, count, 1, k, m, 21, 1, out_pitch, mode);
    if (rc != LLZ_OK) return rc;
    const int log2m = dft_log2(m);
    const dft_args a = {nullptr, out, nullptr, nullptr, post, 0, out_pitch, count, 0, k, m};
    const size_t points = (size_t)count << log2m;
    dft_pick_mode(mode, [&](auto md) {
        hipLaunchKernelGGL((k_dft_extract_f32<md()>), dim3((unsigned)((points + 255) / 256)), dim3(256), 0, as_stream(stream), a, z,
                           log2m);
    });
    LLZ_LAUNCH_CHECK("k_dft_extract_f32");
    return LLZ_OK;
}
