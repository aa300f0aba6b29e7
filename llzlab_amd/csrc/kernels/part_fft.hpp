// part_fft.hpp -- the in-LDS radix-2 transform passes of the partitioned FIR forms: fir_part.hip (K4d / K4e: N = 1024 .. 8192 points,
// 256 threads) and fir_stream.hip (K4f: the B = 64 .. 4096-point complex transform of a real block pair, min(B, 256) threads).
// One workgroup of THREADS threads transforms N = 2^LOG2N complex points in place, two radix-2 stages per LDS round trip:
// decimation in frequency forward (natural order in, bit-reversed out), decimation in time back (bit-reversed in, natural
// out, unscaled).  tw[m] = W_N^m = exp(-2 pi j m / N), m < N / 2.  Both end on a __syncthreads().
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ float2 c_add(float2 a, float2 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 c_sub(float2 a, float2 b) { return {a.x - b.x, a.y - b.y}; }
// a * w (INV = false) or a * conj(w)
template <bool INV>
__device__ __forceinline__ float2 c_mul(float2 a, float2 w)
{
    if (INV) return {__builtin_fmaf(a.y, w.y, a.x * w.x), __builtin_fmaf(-a.x, w.y, a.y * w.x)};
    return {__builtin_fmaf(-a.y, w.y, a.x * w.x), __builtin_fmaf(a.x, w.y, a.y * w.x)};
}

// forward: N-point decimation in frequency in LDS, natural order in, l[i] = X[bitrev(i)] out.  tw[m] = W_N^m, m < N / 2.
template <int LOG2N, int THREADS>
__device__ __forceinline__ void part_fft_dif(float2 *l, const float2 *__restrict__ tw, int tid)
{
    constexpr int N = 1 << LOG2N;
    int S = N;
    for (; S >= 4; S >>= 2) {                   // spans S and S / 2 in one round trip
        const int Q = S >> 2, tstep = N / S;
        __syncthreads();
        for (int b = tid; b < N / 4; b += THREADS) {
            const int j = b & (Q - 1);
            const int base = (b - j) * 4 + j;
            const float2 x0 = l[base], x1 = l[base + Q], x2 = l[base + 2 * Q], x3 = l[base + 3 * Q];
            const float2 w1 = tw[2 * j * tstep];
            const float2 a0 = c_add(x0, x2), a1 = c_add(x1, x3);
            const float2 a2 = c_mul<false>(c_sub(x0, x2), tw[j * tstep]);
            const float2 a3 = c_mul<false>(c_sub(x1, x3), tw[(j + Q) * tstep]);
            l[base] = c_add(a0, a1);
            l[base + Q] = c_mul<false>(c_sub(a0, a1), w1);
            l[base + 2 * Q] = c_add(a2, a3);
            l[base + 3 * Q] = c_mul<false>(c_sub(a2, a3), w1);
        }
    }
    if (S == 2) {                               // odd log2 N: the last span alone, twiddle 1
        __syncthreads();
        for (int b = tid; b < N / 2; b += THREADS) {
            const float2 a = l[2 * b], c = l[2 * b + 1];
            l[2 * b] = c_add(a, c);
            l[2 * b + 1] = c_sub(a, c);
        }
    }
    __syncthreads();
}

// inverse (unscaled): decimation in time, l[i] = Y[bitrev(i)] in, natural order out: the forward's stages backwards
template <int LOG2N, int THREADS>
__device__ __forceinline__ void part_fft_dit_inv(float2 *l, const float2 *__restrict__ tw, int tid)
{
    constexpr int N = 1 << LOG2N;
    int S = 4;
    if (LOG2N & 1) {
        __syncthreads();
        for (int b = tid; b < N / 2; b += THREADS) {
            const float2 a = l[2 * b], c = l[2 * b + 1];
            l[2 * b] = c_add(a, c);
            l[2 * b + 1] = c_sub(a, c);
        }
        S = 8;
    }
    for (; S <= N; S <<= 2) {                   // spans S / 2 and S in one round trip
        const int Q = S >> 2, tstep = N / S;
        __syncthreads();
        for (int b = tid; b < N / 4; b += THREADS) {
            const int j = b & (Q - 1);
            const int base = (b - j) * 4 + j;
            const float2 x0 = l[base], x1 = l[base + Q], x2 = l[base + 2 * Q], x3 = l[base + 3 * Q];
            const float2 w1 = tw[2 * j * tstep];
            const float2 t1 = c_mul<true>(x1, w1), t3 = c_mul<true>(x3, w1);
            const float2 a0 = c_add(x0, t1), a1 = c_sub(x0, t1), a2 = c_add(x2, t3), a3 = c_sub(x2, t3);
            const float2 u2 = c_mul<true>(a2, tw[j * tstep]), u3 = c_mul<true>(a3, tw[(j + Q) * tstep]);
            l[base] = c_add(a0, u2);
            l[base + 2 * Q] = c_sub(a0, u2);
            l[base + Q] = c_add(a1, u3);
            l[base + 3 * Q] = c_sub(a1, u3);
        }
    }
    __syncthreads();
}

} // namespace
