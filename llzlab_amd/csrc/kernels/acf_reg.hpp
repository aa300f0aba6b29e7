// acf_reg.hpp -- the register form of the direct auto / cross correlation of one frame, shared by k_autocorr_reg_f32 (corr.hip) and
// the fused LPC kernel (lpc.hip), so that both give the same bits: the same chunks, the same per-lane FMA order and the same
// cross-lane reduction.
#pragma once
#include "common.hpp"

namespace {

// All K per-lane partial sums of a wave at once by recursive halving: in the step with distance d a lane keeps one accumulator of a
// pair and hands the other to lane ^ d, which keeps that one -- the number of live sums halves with every step (17 -> 9 -> 5 -> 3
// -> 2 -> 1 -> 1: 21 exchanges instead of 17 x 6).  Returns the total of sum number (six bits of the lane, reversed) -- for
// K <= 64 every sum ends in exactly one lane; *which says which.
template <int K>
__device__ __forceinline__ float wave_sums(float (&acc)[K], int lane, int *which)
{
    static_assert(K <= 64, "one sum per lane at most");
    int cnt = K;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const bool upper = (lane & d) != 0;
        const int half = (cnt + 1) / 2;
#pragma unroll
        for (int i = 0; i < (K + 1) / 2; i++) {
            if (i < half) {
                const float a = acc[2 * i], b = 2 * i + 1 < cnt ? acc[2 * i + 1] : 0.f;
                acc[i] = (upper ? b : a) + __shfl_xor(upper ? a : b, d, 64);
            }
        }
        cnt = half;
    }
    *which = (int)(__brev((unsigned)lane) >> 26);
    return acc[0];
}

typedef float ac_f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) ac_x4 { ac_f32x4 v; };     // a 16-byte load at any 4-byte address

// Eight consecutive samples row[i0 .. i0 + 7] of a frame of n samples, zeros behind its end (those products vanish).  WIN: the
// samples are multiplied by win[i] (one float32 rounding) as they are loaded.
template <bool WIN>
__device__ __forceinline__ void acf_fetch8(const float *row, const float *win, int n, int i0, float (&v)[8])
{
#pragma clang fp contract(off)
    if (i0 + 8 <= n) {
        const ac_f32x4 a = reinterpret_cast<const ac_x4 *>(row + i0)->v, b = reinterpret_cast<const ac_x4 *>(row + i0 + 4)->v;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        if (WIN) {
            const ac_f32x4 wa = reinterpret_cast<const ac_x4 *>(win + i0)->v, wb = reinterpret_cast<const ac_x4 *>(win + i0 + 4)->v;
            v[0] *= wa.x; v[1] *= wa.y; v[2] *= wa.z; v[3] *= wa.w;
            v[4] *= wb.x; v[5] *= wb.y; v[6] *= wb.z; v[7] *= wb.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            v[j] = i0 + j < n ? (WIN ? row[i0 + j] * win[i0 + j] : row[i0 + j]) : 0.f;
    }
}

// Per-lane partial sums of lags K0 .. 8 NL of one frame of n samples (`row`): lane l keeps x[8 l .. 8 l + 7] of a chunk in
// registers and gets the samples it slides over from lanes l + 1 .. l + NL through the wave shuffle, so a chunk is 8 (64 - NL)
// samples (the last NL lanes only look ahead: their own products are formed by the next chunk, where they are the first lanes);
// the next chunk's samples are requested before the current one is worked on.  One 16-byte-pair load and 8 (8 NL + 1) FMAs per
// lane and chunk.  WIN: the samples are multiplied by win[i] (one float32 rounding) as they are loaded, before any shuffle.
// CROSS: the samples slid over come from a second row, `wrow` (the cross-correlation sum_i row[i] * wrow[i + k]: two loads per
// lane and chunk); chunks, FMA order and accumulators are the same, so wrow == row gives the bits of the one-row form.
// acc[k] belongs to lag K0 + k (K0 = 1: the negative side of a two-sided cross-correlation, whose lag 0 the positive side has).
template <int NL, bool WIN, bool CROSS = false, int K0 = 0>
__device__ __forceinline__ void acf_reg_frame(const float *row, const float *win, int n, int lane,
                                              float (&acc)[8 * NL + 1 - K0], const float *wrow = nullptr)
{
    static_assert(!(WIN && CROSS) && (K0 == 0 || K0 == 1), "no windowed cross form");
    constexpr int NLAG = 8 * NL + 1 - K0, STEP = 8 * (64 - NL);
    const bool active = lane < 64 - NL;
#pragma unroll
    for (int k = 0; k < NLAG; k++) acc[k] = 0.f;
    float cur[8], nxt[8], wcur[8], wnxt[8];
    acf_fetch8<WIN>(row, win, n, 8 * lane, cur);
    if (CROSS) acf_fetch8<false>(wrow, nullptr, n, 8 * lane, wcur);
    for (int c0 = 0; c0 < n; c0 += STEP) {
        const bool more = c0 + STEP < n;
        if (more) {
            acf_fetch8<WIN>(row, win, n, c0 + STEP + 8 * lane, nxt);
            if (CROSS) acf_fetch8<false>(wrow, nullptr, n, c0 + STEP + 8 * lane, wnxt);
        }
        // s = the lane's samples of the row slid over followed by those of lanes l + 1 .. l + NL
        float s[8 * (NL + 1)];
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = CROSS ? wcur[j] : cur[j];
#pragma unroll
        for (int h = 1; h <= NL; h++)
#pragma unroll
            for (int j = 0; j < 8; j++) s[8 * h + j] = __shfl_down(s[8 * (h - 1) + j], 1, 64);
        float xa[8];
#pragma unroll
        for (int j = 0; j < 8; j++) xa[j] = active ? cur[j] : 0.f;
#pragma unroll
        for (int k = 0; k < NLAG; k++)
#pragma unroll
            for (int j = 0; j < 8; j++) acc[k] = __builtin_fmaf(xa[j], s[j + k + K0], acc[k]);
        if (more) {                                      // (a last chunk has fetched nothing to hand on)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                cur[j] = nxt[j];
                if (CROSS) wcur[j] = wnxt[j];
            }
        }
    }
}

} // namespace
