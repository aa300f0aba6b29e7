// fft_square.hpp -- what the register-transform kernels of the FFT family share (fft.hip, acf_fft.hip, stft.hip): the E-point
// transform and the E x E core of the square sizes, the twiddle table of the 1024-point half-wave kernels, the overlap-add
// walk of the register synthesis kernels, and the cache of the twiddle tables derived on the device.
#pragma once
#include <array>
#include <map>
#include <mutex>
#include "fft_core.hpp"
#include "fft32.hpp"

namespace {

// Square sizes N = E*E beside 1024 (E = 16: N = 256, E = 64: N = 4096), float32: the same two-register-pass scheme as
// k_fft1024_f32 with a group of E lanes per transform (a quarter wave / a whole wave), E elements per lane.
// The E-point transform is the decimation-in-time form of fft32.hpp written for any E <= 64 (constants in 64ths of a
// turn); the inter-pass twiddles W_N^(k1*l) come from a [E][E] table laid out so that a group reads a contiguous row.
__device__ constexpr float kCos64[17] = {1.00000000000000000000f, 0.99518472667219692873f, 0.98078528040323043058f, 0.95694033573220882438f, 0.92387953251128673848f, 0.88192126434835504956f, 0.83146961230254523567f, 0.77301045336273699338f, 0.70710678118654757274f, 0.63439328416364548779f, 0.55557023301960228867f, 0.47139673682599780857f, 0.38268343236508983729f, 0.29028467725446233105f, 0.19509032201612833135f, 0.09801714032956077016f, 0.00000000000000006123f};

template <int E>
__device__ constexpr int brevE(int r)
{
    int o = 0;
    for (int b = 1, t = E >> 1; b < E; b <<= 1, t >>= 1)
        if (r & b) o |= t;
    return o;
}

// (a, b) -> (a + w b, a - w b), w = W_E^q (conjugated for the inverse), 0 <= q < E/2, Linzer-Feig form as in fft32.hpp
template <int E, bool INV>
__device__ __forceinline__ void bfly_ditE(cf &a, cf &b, int q)
{
    const int q64 = q * (64 / E);                               // sixty-fourths of a turn, 0..31
    const cf A = a, B = b;
    if (q64 == 0) {
        a = cadd(A, B); b = csub(A, B);
        return;
    }
    if (q64 == 16) {
        const cf wb = INV ? cf{-B.y, B.x} : cf{B.y, -B.x};
        a = cadd(A, wb); b = csub(A, wb);
        return;
    }
    const float c = q64 <= 16 ? kCos64[q64] : -kCos64[32 - q64];
    const float s0 = q64 <= 16 ? kCos64[16 - q64] : kCos64[q64 - 16];
    const float sn = INV ? s0 : -s0;
    float p, g, f;
    if (c >= s0 || -c >= s0) {
        const float t = sn / c;
        p = __builtin_fmaf(-t, B.y, B.x);
        g = __builtin_fmaf(t, B.x, B.y);
        f = c;
    } else {
        const float r = c / sn;
        p = __builtin_fmaf(r, B.x, -B.y);
        g = __builtin_fmaf(r, B.y, B.x);
        f = sn;
    }
    a = cf{__builtin_fmaf(f, p, A.x), __builtin_fmaf(f, g, A.y)};
    b = cf{__builtin_fmaf(-f, p, A.x), __builtin_fmaf(-f, g, A.y)};
}

// natural order in, v[r] = X[brevE(r)] out.  The decimation-in-time network works on w[i] = v[brevE(i)] and leaves
// w[j] = X[j]; with w aliased onto v through the index map both permutations cost nothing.
template <int E, bool INV>
__device__ __forceinline__ void fftE(cf (&v)[E])
{
#pragma unroll
    for (int half = 1; half <= E / 2; half <<= 1) {
        const int tstep = (E / 2) / half;
#pragma unroll
        for (int blk = 0; blk < E; blk += 2 * half) {
#pragma unroll
            for (int q = 0; q < half; q++)
                bfly_ditE<E, INV>(v[brevE<E>(blk + q)], v[brevE<E>(blk + q + half)], q * tstep);
        }
    }
}

// the E x E core shared by the square-size kernels: E-point transform, transpose inside the lane group, inter-pass twiddle
// W_(E*E)^(k1 * l) read as contiguous rows of the symmetric table, E-point transform.  In: v[j] = element lg + E j of the
// group's transform; out: v[q] = bin lg + E brevE(q).
template <int E, bool INV>
__device__ __forceinline__ void square_core(cf (&v)[E], float *buf, const float2 *__restrict__ tw2d, int lg)
{
    constexpr int PITCH = E + 1;
    fftE<E, INV>(v);
#pragma unroll
    for (int q = 0; q < E; q++) buf[brevE<E>(q) * PITCH + lg] = v[q].x;
    OLS_WAVE_SYNC();
#pragma unroll
    for (int cidx = 0; cidx < E; cidx++) v[cidx].x = buf[lg * PITCH + cidx];
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < E; q++) buf[brevE<E>(q) * PITCH + lg] = v[q].y;
    OLS_WAVE_SYNC();
#pragma unroll
    for (int cidx = 0; cidx < E; cidx++) v[cidx].y = buf[lg * PITCH + cidx];
    OLS_WAVE_SYNC();
#pragma unroll
    for (int l0 = 0; l0 < E; l0 += 8) {
#pragma unroll
        for (int l = l0; l < l0 + 8; l++) {
            const float2 w = tw2d[l * E + lg];
            v[l] = cmul<INV>(v[l], cf{w.x, w.y});
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    fftE<E, INV>(v);
}

// the [32][32] table of the 1024-point half-wave kernels (transpose_twiddle of fft32.hpp): s_tw[a][b] = W_1024^(a*b) =
// exp(-2 pi j a b / 1024) from the host-built cs (1024 cos, then 1024 sin); the caller places the barrier
__device__ __forceinline__ void load_tw1024(float2 *s_tw, const float *__restrict__ cs, int tid)
{
    for (int i = tid; i < 1024; i += 256) {
        const int m = ((i >> 5) * (i & 31)) & 1023;
        s_tw[i] = make_float2(cs[m], -cs[1024 + m]);
    }
}

// Overlap-add walk of the register synthesis kernels.  A workgroup owns output blocks [b0, b1) of one channel; block t
// (F samples) is the sum of the windowed inverse transforms of frames t-R+1 .. t (llz_asmodel.c:279-304), so it walks
// frames max(0, b0-R+1) .. b1-1 in groups of TPW, keeps the running overlap-add tail (N - F samples) in `carry` and drops
// the blocks in front of b0 (their sums are incomplete; the first run of a channel starts from the handle's tail instead).
// fill(c, g0, ng) writes the windowed frames g0 .. g0+ng-1 of channel c into seg[0 .. ng); the accumulation order per
// sample is the reference's, oldest frame first.
template <int TPW, int N, typename Fill>
__device__ __forceinline__ void stft_ola_walk(float (&seg)[TPW][N], float (&carry)[N], float *__restrict__ x,
                                              const float *__restrict__ ola_old, float *__restrict__ ola_new, int frames,
                                              int F, long x_pitch, int run_len, int runs, float magic, int tid, Fill fill)
{
    constexpr int MAXM = ((TPW - 1) * (N / 2) + N + 255) / 256;        // span of a group at the largest hop (N/2)
    const int c = blockIdx.x / runs, run = blockIdx.x - c * runs;
    const int b0 = run * run_len, b1 = min(frames, b0 + run_len);
    const int R = N / F, keep = N - F;
    const int fs = max(0, b0 - (R - 1));
    for (int q = tid; q < keep; q += 256) carry[q] = fs == 0 ? ola_old[(size_t)c * keep + q] : 0.f;
    for (int g0 = fs; g0 < b1; g0 += TPW) {
        const int ng = min(TPW, b1 - g0);
        __syncthreads();                                               // carry and seg of the previous group are consumed
        fill(c, g0, ng);
        __syncthreads();
        const int span = (ng - 1) * F + N;
        float acc[MAXM];
#pragma unroll
        for (int m = 0; m < MAXM; m++) {
            const int p = tid + m * 256;
            float a = 0.f;
            if (p < span) {
                a = p < keep ? carry[p] : 0.f;
                const int k_hi = min(ng - 1, p / F);                   // frames k with 0 <= p - kF < N
                const int k_lo = p < N ? 0 : (p - N) / F + 1;
                for (int k = k_lo; k <= k_hi; k++) a += seg[k][p - k * F];
            }
            acc[m] = a;
        }
        __syncthreads();                                               // every read of carry and seg is done
#pragma unroll
        for (int m = 0; m < MAXM; m++) {
            const int p = tid + m * 256;
            if (p < span) {
                if (p < ng * F) {
                    if (g0 + p / F >= b0) x[(size_t)c * x_pitch + (size_t)g0 * F + p] = magic * acc[m];
                } else {
                    carry[p - ng * F] = acc[m];
                }
            }
        }
    }
    __syncthreads();
    if (b1 == frames)
        for (int q = tid; q < keep; q += 256) ola_new[(size_t)c * keep + q] = carry[q];
}

// ---------------------------------------------------------------------------------------------------------------------
// Twiddle tables derived on the device from a handle's table cs (cos, then sin of 2 pi i / N, N = stride E^2: exactly the
// host-built values), [E][E] float2 each:
//   tw2d[k1][l] = W_N^(stride k1 l)   the inter-pass twiddles of square_core: W_(E^2)^(k1 l)
//   tw1[j][l]   = W_N^(l + E j)       the radix-2 step around two E x E transforms (stride 2 only; null: not wanted)
__global__ void k_fft_tables(float2 *__restrict__ tw2d, float2 *__restrict__ tw1, const float *__restrict__ cs, int E,
                             int stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x, H = E * E, N = stride * H;
    if (i >= H) return;
    const int m2 = (stride * (i / E) * (i % E)) & (N - 1);
    tw2d[i] = make_float2(cs[m2], -cs[N + m2]);
    if (!tw1) return;
    const int m1 = (i % E) + E * (i / E);
    tw1[i] = make_float2(cs[m1], -cs[N + m1]);
}

// One set per (kind, key, device), built on first use and kept for the process; the state is the including file's own, so
// a kind number means something inside one file only.  The lock is held from the lookup until freshly built tables are
// published, and they are published only once complete (other streams may use them at once), tw1 before the tw2d that
// marks the set as built: any number of host threads and any device index are fine.
static int fft_derived_tables(int kind, int key, int E, int stride, bool with_tw1, const float *cs, void *stream,
                              const char *what, const float2 **tw2d, const float2 **tw1)
{
    static std::mutex lock;
    static std::map<std::array<int, 3>, std::array<float2 *, 2>> sets;
    int dev = 0;
    LLZ_HIP_CHECK(hipGetDevice(&dev));
    const int H = E * E;
    std::lock_guard<std::mutex> guard(lock);
    std::array<float2 *, 2> &set = sets[{kind, key, dev}];
    if (!set[0]) {
        float2 *t = nullptr;
        LLZ_HIP_CHECK(hipMalloc(&t, sizeof(float2) * (size_t)H * (with_tw1 ? 2 : 1)));
        hipLaunchKernelGGL(k_fft_tables, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, as_stream(stream), t,
                           with_tw1 ? t + H : nullptr, cs, E, stride);
        LLZ_LAUNCH_CHECK(what);
        LLZ_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
        set[1] = with_tw1 ? t + H : nullptr;
        set[0] = t;
    }
    *tw2d = set[0];
    if (tw1) *tw1 = set[1];
    return LLZ_OK;
}

} // namespace
