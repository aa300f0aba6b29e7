// fir_adapt.hip -- K4h: the partitioned frequency-domain NLMS adaptive filter (llz_adapt_mc, include/llz_adapt.h): K4f's filter
// (fir_stream.hip: the ring of packed half-spectra of the input, one workgroup per channel, the head by value) plus an error, a
// normalised gradient and a constrained weight update on the same ring.  Per channel and block j, N = 2 B, P partitions:
//   filter(j):  X_j into ring slot cur; Y = sum_{p < P} X_{j-p} W_p, p ascending; y_j = the last B samples of the inverse;
//               e_j = d_j - y_j; and where the channel's mu is not zero D = sum_p |X_{j-p}|^2 (in the same walk of the ring),
//               E = the spectrum of (0_B, e_j), G = mu E / (D + delta) into a [channels][B] scratch;
//   update(j):  for every p: dW = conj(X_{j-p}) G; its inverse transform; every sample t >= min(B, flt_len - p B) zeroed (the
//               gradient constraint: the second half, and in the last partition what lies beyond flt_len); the forward
//               transform; W_p += dW.
// Two launches per block, filter(0), update(0), filter(1), ... on one stream, which is the only ordering they need: update(j)
// reads the G and the ring slot filter(j) wrote, filter(j + 1) the W update(j) wrote.  The slot comes by value with each
// launch, so a launch captured into a graph would replay one slot: not supported, as for K4f.
//
// Choices, with their reasons:
//   * The layout is K4f's (stream_bins.hpp): position i holds bin bitrev(i), position 0 packs DC and Nyquist, the ring holds the
//     doubled split output X' = 2 X, W carries K4f's 1 / (2 N): W' = W / (2 N).  With these D' = sum |X'|^2 = 4 D and E' = 2 E,
//     so G' = mu E' / (D' + 4 delta) = G / 2 and conj(X') G' = conj(X) G; the transform pair of the constraint returns 2 N times
//     its input spectrum and W' wants 1 / (2 N) of it: the window multiplies the samples it keeps by 1 / (4 N^2).  Every one of
//     these factors is a power of two.  The two halves of packed bin 0 are two real bins in the product, the power and the
//     quotient.
//   * The filter kernel is K4f's walk with K4f's helpers, bin ownership and product order (bin_mac, p ascending): for given
//     weights y has the bits of llz_fir_stream_mc with those taps.  The power is summed beside the product from the values the
//     product loads, real and imaginary squares apart, added at the end.
//   * A channel whose mu is zero is frozen: its filter workgroup stops behind e (a workgroup-uniform branch), its update
//     workgroups return at once, so its W keeps its bits.  The host launches no update when every mu is zero.
//   * The update runs on a grid of (channel, group of partitions).  A partition's update depends on X_{j-p}, G and W_p alone,
//     so no two workgroups touch the same W_p: no atomics, no fences, and the grouping cannot change a bit.  A workgroup keeps G
//     in registers for its partitions; per partition it moves 3 B 8 bytes (X read, W read and written) and runs two B-point
//     transforms.  One partition per workgroup where the grid would otherwise not fill the device (fewer than 4096 (channel,
//     partition) pairs: 16 workgroups per CU), else 4, which takes the read of G from a quarter of a workgroup's traffic to a
//     thirteenth.  Timed at 1024 channels against 1, 2 and 8 (the adapt_ppw override): within 5 %, 4 the fastest at 25248 taps.
//   * Blocks 64 .. 2048: at 4096 a thread owns 16 bins, K4f is at 238 VGPRs there and this kernel carries the power sums on top.
//   * All index arithmetic over channels x slots x bins is size_t / long.
//   * The error tail behind the inverse transform, the update kernel (k_adapt_update<LOG2B, false>) and the launch preamble are
//     adapt_steps.hpp's, shared with fir_adapt_matrix.hip (K4i).  This file keeps the front: the ring walk with the power sums.
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"
#include "adapt_steps.hpp"

namespace {

struct adapt_filter_geom {
    int P, R, cur;              // partitions, ring slots, the slot this block's spectrum goes to
    int j, last;                // the block of the call; last != 0: the call's last block (the input block goes to prev)
    long pitch;                 // row pitch of x, d, e and y
    float delta4;               // 4 delta: the regularisation against the doubled spectra's power
};

// K4h filter: workgroup c -> channel c, block G.j of the call.  tw as K4f's.  W: [channels][P][B]; gs: [channels][B]
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adapt_filter(const float *__restrict__ x, const float *__restrict__ d, float *__restrict__ e, float *__restrict__ y,
               const float2 *__restrict__ W, const float2 *__restrict__ tw, float2 *ring, float *prev, float2 *__restrict__ gs,
               const float *__restrict__ mus, adapt_filter_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    constexpr int U = M >= 8 ? 1 : 8 / M;                   // partitions in flight
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, c = blockIdx.x;
    const float2 *spl = tw + B / 2;
    const size_t row = (size_t)c * (size_t)G.pitch + (size_t)G.j * B;
    const float *xrow = x + row, *drow = d + row;
    float *prow = prev + (size_t)c * B;
    float2 *rc = ring + (size_t)c * (size_t)G.R * B;
    const float2 *wc = W + (size_t)c * (size_t)G.P * B;
    const float mu = mus[c];

    int pos[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) pos[g] = (tid + g * T) * V;
    const bool first = tid == 0;                            // owner of position 0, the packed bin

    // (previous block, this block) as B complex values
    const float *older = G.j == 0 ? prow : xrow - B;
    for (int t = tid; t < B; t += T) {
        lf[t] = older[t];
        lf[B + t] = xrow[t];
    }
    part_fft_dif<LOG2B, T>(lds, tw, tid);
    float2 xb[M], acc[M], pw[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int i = pos[m / V] + m % V;
        const float2 a = lds[i];
        xb[m] = split_fwd(a, lds[mirror<LOG2B>(i)], spl[i]);
        if (m == 0 && first) xb[m] = split_fwd0(a);
    }
    // pw: the squares of the real and of the imaginary parts, summed apart
    auto power = [](float2 &q, float2 v) {
        q.x = __builtin_fmaf(v.x, v.x, q.x);
        q.y = __builtin_fmaf(v.y, v.y, q.y);
    };
    float2 *slot = rc + (size_t)G.cur * B;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        float2 h[V];
        store_bins<V>(slot + pos[g], &xb[g * V]);
        load_bins<V>(wc + pos[g], h);
#pragma unroll
        for (int v = 0; v < V; v++) {
            acc[g * V + v] = float2{0.f, 0.f};
            pw[g * V + v] = float2{0.f, 0.f};
            bin_mac(acc[g * V + v], xb[g * V + v], h[v], g == 0 && v == 0 && first);
            power(pw[g * V + v], xb[g * V + v]);
        }
    }
    int p = 1;
    // Y = sum_p X_{j-p} W_p, p ascending; slot of X_{j-p} = (cur - p) mod R
    auto step = [&](int pp) {
        int s = G.cur - pp;
        if (s < 0) s += G.R;
        const float2 *xs = rc + (size_t)s * B, *hs = wc + (size_t)pp * B;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            float2 xv[V], h[V];
            load_bins<V>(xs + pos[g], xv);
            load_bins<V>(hs + pos[g], h);
#pragma unroll
            for (int v = 0; v < V; v++) {
                bin_mac(acc[g * V + v], xv[v], h[v], g == 0 && v == 0 && first);
                power(pw[g * V + v], xv[v]);
            }
        }
    };
#pragma unroll 1
    for (; p + U <= G.P; p += U) {
#pragma unroll
        for (int u = 0; u < U; u++) step(p + u);
    }
#pragma unroll 1
    for (; p < G.P; p++) step(p);

    // inverse split through LDS
    __syncthreads();                                        // every mirror read of the forward split is done
#pragma unroll
    for (int g = 0; g < NG; g++) store_bins<V>(lds + pos[g], &acc[g * V]);
    __syncthreads();
    float2 zz[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int i = pos[m / V] + m % V;
        zz[m] = split_inv(acc[m], lds[mirror<LOG2B>(i)], spl[i]);
        if (m == 0 && first) zz[m] = split_inv0(acc[m]);
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; g++) store_bins<V>(lds + pos[g], &zz[g * V]);
    part_fft_dit_inv<LOG2B, T>(lds, tw, tid);
    // the denominators of the V positions from pos[g] on: D' + 4 delta, the halves of the packed bin each by its own
    auto den = [&](int g, float2 *dn) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int m = g * V + v;
            const bool packed0 = m == 0 && first;
            const float dsum = pw[m].x + pw[m].y;
            dn[v] = float2{(packed0 ? pw[m].x : dsum) + G.delta4, (packed0 ? pw[m].y : dsum) + G.delta4};
        }
    };
    // y, e = d - y, the call's last block handed over to prev, and where the channel adapts G = mu E / den
    adapt_error_tail<LOG2B>(lds, tw, tid, pos, drow, e, y, row, G.last ? prow : nullptr, xrow, mu, gs + (size_t)c * B, den);
}

} // namespace

// Block j of a call of nblk blocks: x, d, e, y are [channels][pitch] (y may be null), the block's samples at [j block, (j + 1)
// block); its spectrum goes to ring slot `slot`; w: [channels][P][block] packed spectra as llz_host_stream_spectra builds them;
// tw, ring, prev as llzs_fir_stream_f32's; g: [channels][block] complex, written for the channels whose mu is not zero.
extern "C" int llzs_fir_adapt_filter_f32(int block, int flt_len, const float *w, const float *tw, float *ring, float *prev,
                                         float *g, const float *mu, float delta, const float *x, const float *d, float *e,
                                         float *y, int channels, int nblk, int j, long pitch, int P, int R, int slot, void *stream)
{
    int log2b;
    const bool ok = adapt_log2(block, &log2b);
    if (!adapt_geom_ok(ok, block, flt_len, P, R, slot) || channels < 1 || channels > 65535 ||
        !(w && tw && ring && prev && g && mu && x && d && e) || nblk < 1 || j < 0 || j >= nblk || pitch < (long)nblk * block ||
        !(delta > 0.f)) {
        llzs_set_error("fir_adapt_filter_f32: bad arguments (block=%d flt_len=%d channels=%d nblk=%d j=%d P=%d R=%d slot=%d)", block,
                       flt_len, channels, nblk, j, P, R, slot);
        return LLZ_ERR_ARG;
    }
    const adapt_filter_geom G = {P, R, slot, j, j == nblk - 1, pitch, 4.f * delta};
    const float2 *W = reinterpret_cast<const float2 *>(w), *TW = reinterpret_cast<const float2 *>(tw);
    float2 *rg = reinterpret_cast<float2 *>(ring), *gs = reinterpret_cast<float2 *>(g);
    hipStream_t st = as_stream(stream);
#define FILTER(L)                                                                                                                \
    hipLaunchKernelGGL((k_adapt_filter<L>), dim3((unsigned)channels), dim3(stream_threads(L)), 0, st, x, d, e, y, W, TW, rg, prev,  \
                       gs, mu, G)
    ADAPT_DISPATCH(log2b, FILTER)
#undef FILTER
    LLZ_LAUNCH_CHECK("k_adapt_filter");
    return LLZ_OK;
}

// The weight update behind llzs_fir_adapt_filter_f32 of the same block and slot: W_p += the constrained conj(X_{j-p}) G for every
// p < P of every channel whose mu is not zero.
extern "C" int llzs_fir_adapt_update_f32(int block, int flt_len, float *w, const float *tw, const float *ring, const float *g,
                                         const float *mu, int channels, int P, int R, int slot, void *stream)
{
    int log2b;
    const bool ok = adapt_log2(block, &log2b);
    if (!adapt_geom_ok(ok, block, flt_len, P, R, slot) || channels < 1 || channels > 65535 || !(w && tw && ring && g && mu)) {
        llzs_set_error("fir_adapt_update_f32: bad arguments (block=%d flt_len=%d channels=%d P=%d R=%d slot=%d)", block, flt_len,
                       channels, P, R, slot);
        return LLZ_ERR_ARG;
    }
    const adapt_update_geom G = {1, P, R, slot, flt_len};
    const int ppw = adapt_ppw((long)channels * P), nq = (P + ppw - 1) / ppw;
    const dim3 grid((unsigned)channels, (unsigned)nq);
    float2 *W = reinterpret_cast<float2 *>(w);
    const float2 *TW = reinterpret_cast<const float2 *>(tw), *rg = reinterpret_cast<const float2 *>(ring);
    const float2 *gs = reinterpret_cast<const float2 *>(g);
    hipStream_t st = as_stream(stream);
#define UPDATE(L) hipLaunchKernelGGL((k_adapt_update<L, false>), grid, dim3(stream_threads(L)), 0, st, W, TW, rg, gs, mu, G, ppw, nq)
    ADAPT_DISPATCH(log2b, UPDATE)
#undef UPDATE
    LLZ_LAUNCH_CHECK("k_adapt_update");
    return LLZ_OK;
}
