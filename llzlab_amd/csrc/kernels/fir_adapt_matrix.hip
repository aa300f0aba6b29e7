// fir_adapt_matrix.hip -- K4i: the multi-reference frequency-domain NLMS adaptive filter (llz_adapt_matrix_mc,
// include/llz_adapt_matrix.h): I shared references, O desired signals, a weight set per path (o, i).  It is K4g's delay lines
// and product (fir_matrix.hip: a ring of packed half-spectra per INPUT, the sum over inputs in G groups) with K4h's error,
// normalised gradient and constrained update (fir_adapt.hip) on those rings.  Per call of k blocks:
//   llzs_fir_matrix_fwd_f32 (K4g, unchanged): the k spectra of every input into its ring;
//   power:  grid (block of the call, bin tile): den[j] = sum_i sum_p |X_{i,j-p}|^2 + delta, i ascending, p ascending within i,
//           one fma chain per bin for the squares of the real parts and one for the imaginary parts, added at the end; it
//           does not depend on W, so all k blocks go in one launch;
// and per block j, ordered by the stream:
//   llzs_fir_matrix_mac_f32 (K4g, unchanged) with one block and a connection table of ones: the G partial spectra of Y_o;
//   error:  grid (output): the partials added g ascending, the inverse split and transform (K4g's inverse to the letter), then
//           the tail K4h's filter runs (adapt_steps.hpp, adapt_error_tail): y, e = d - y, and where mu_o != 0 E = the spectrum
//           of (0_B, e), G_o = mu_o E / den[j] into an [outputs][B] scratch;
//   update: grid ((input, group of partitions), output): W_{o,i,p} += the constrained conj(X_{i,j-p}) G_o: the kernel K4h
//           launches (adapt_steps.hpp, k_adapt_update) on input i's ring and path (o, i)'s weights.
// With one input the chains are K4h's: e, y and W have llz_adapt_mc's bits.  Frozen (every mu zero) y has llz_fir_matrix_mc's.
//
// Choices, with their reasons:
//   * Layout and power-of-two scalings are K4h's (fir_adapt.hip): the ring holds X' = 2 X, W' = W / (2 N), den' = 4 D + 4 delta,
//     the window of the constraint scales by 1 / (4 N^2).  Packed bin 0 is two real bins in the product, the power and the
//     quotient.  den is stored as the two denominators of a position (equal but for position 0).
//   * The power is a launch of its own, not part of the product: the product's walk is split over input groups and outputs,
//     the power is one chain over ALL inputs and the same for every output.  One bin per thread; the chain is I P fmas long and
//     one wave owns a bin from end to end, so the walk is written for few instructions per slot (see the kernel).
//   * The update folds (input, partition group) into grid.x (up to 4096 x 2049) and keeps the outputs on grid.y (<= 4096), so no
//     legal shape meets the 65535 limit.  No two workgroups touch one W_{o,i,p}: no atomics, no fences, and the grouping (the
//     adapt_ppw override, default 4 from 4096 (path, partition) pairs on, else 1) cannot change a bit.
//   * A frozen output's error workgroup stops behind e and its update workgroups return at once; the host launches no power
//     and no update when every output is frozen.
//   * All index arithmetic over outputs x inputs x partitions x bins is size_t.
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"
#include "adapt_steps.hpp"

namespace {

struct adaptx_power_geom {
    int inputs, P, R;
    int cur;                    // the ring slot of block 0 of the launch
    float delta4;               // 4 delta: the regularisation against the doubled spectra's power
};

struct adaptx_error_geom {
    int outputs;
    int groups;                 // input groups of the partial spectra
    int j;                      // the block of the call
    long pitch;                 // row pitch of d, e and y
};

// power: workgroup (j, tile) -> block j of the call, bins [tile T, (tile + 1) T).  den: [nblk][B] (dx, dy)
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adaptx_power(const float2 *__restrict__ ring, float2 *__restrict__ den, adaptx_power_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), U = 16;     // slots in flight
    const int pos = (int)blockIdx.y * T + (int)threadIdx.x, j = blockIdx.x;
    const int cur = (G.cur + j) % G.R;
    float2 pw = float2{0.f, 0.f};
    auto power = [&](float2 v) {
        pw.x = __builtin_fmaf(v.x, v.x, pw.x);
        pw.y = __builtin_fmaf(v.y, v.y, pw.y);
    };
    // n slots downwards from `top`, in that order.  The chain is I P fmas long and one wave owns a bin from end to end, so
    // what counts is the instructions per slot: whole batches read at constant offsets from a pointer that only steps, and the
    // last, short batch reads its last slot again in the places it does not use
    auto walk = [&](const float2 *top, int n) {
        const float2 *q = top;
        int k = n;
#pragma unroll 1
        for (; k >= U; k -= U, q -= (size_t)U * B) {
            float2 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = *(q - (size_t)u * B);
#pragma unroll
            for (int u = 0; u < U; u++) power(v[u]);
        }
        if (k > 0) {
            float2 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = *(q - (size_t)(u < k ? u : k - 1) * B);
#pragma unroll
            for (int u = 0; u < U; u++)
                if (u < k) power(v[u]);
        }
    };
    // X_{i,j-p} lies in slot (cur - p) mod R: slots cur .. 0 for p <= cur, then R - 1 downwards
    const int n1 = G.P <= cur + 1 ? G.P : cur + 1;
    for (int i = 0; i < G.inputs; i++) {
        const float2 *rc = ring + (size_t)i * (size_t)G.R * B + pos;
        walk(rc + (size_t)cur * B, n1);
        walk(rc + (size_t)(G.R - 1) * B, G.P - n1);
    }
    const bool packed0 = pos == 0;
    const float dsum = pw.x + pw.y;
    const float dx = (packed0 ? pw.x : dsum) + G.delta4, dy = (packed0 ? pw.y : dsum) + G.delta4;
    den[(size_t)j * B + pos] = float2{dx, dy};
}

// error: workgroup o -> output o, block G.j of the call.  Y: [groups][outputs][B] partial spectra; den: this block's [B]
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adaptx_error(const float2 *__restrict__ Y, const float2 *__restrict__ tw, const float *__restrict__ d, float *__restrict__ e,
               float *__restrict__ y, const float2 *__restrict__ den, float2 *__restrict__ gs, const float *__restrict__ mus,
               adaptx_error_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    const int tid = threadIdx.x, o = blockIdx.x;
    const float2 *spl = tw + B / 2;
    const size_t gstride = (size_t)G.outputs * B;
    const float2 *y0 = Y + (size_t)o * B;
    const size_t row = (size_t)o * (size_t)G.pitch + (size_t)G.j * B;
    const float mu = mus[o];
    int pos[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) pos[g] = (tid + g * T) * V;
    const bool first = tid == 0;                            // owner of position 0, the packed bin

    float2 acc[M];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        load_bins<V>(y0 + pos[g], &acc[g * V]);
        for (int gg = 1; gg < G.groups; gg++) {
            float2 part[V];
            load_bins<V>(y0 + (size_t)gg * gstride + pos[g], part);
#pragma unroll
            for (int v = 0; v < V; v++) acc[g * V + v] = c_add(acc[g * V + v], part[v]);
        }
        store_bins<V>(lds + pos[g], &acc[g * V]);
    }
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
    // y, e = d - y, and where the output adapts G = mu E / den: the denominators of a position come from the block's den row
    adapt_error_tail<LOG2B>(lds, tw, tid, pos, d + row, e, y, row, nullptr, nullptr, mu, gs + (size_t)o * B,
                            [&](int g, float2 *dn) { load_bins<V>(den + pos[g], dn); });
}

// inputs and outputs: 1 .. 4096 each, so that no legal shape meets a grid limit
bool adaptx_ports_ok(int ports) { return ports >= 1 && ports <= 4096; }

} // namespace

// den[j][block] (two floats per position) = delta + the power of the P spectra behind block j of every input, for the nblk
// blocks whose spectra lie in ring slots (slot + j) mod R; ring = [inputs][R][block] complex as llzs_fir_matrix_fwd_f32 fills it.
extern "C" int llzs_fir_adapt_matrix_power_f32(int block, int flt_len, const float *ring, float *den, float delta, int inputs,
                                               int nblk, int P, int R, int slot, void *stream)
{
    int log2b;
    const bool ok = adapt_log2(block, &log2b);
    if (!adapt_geom_ok(ok, block, flt_len, P, R, slot) || !adaptx_ports_ok(inputs) || !ring || !den || nblk < 1 || !(delta > 0.f)) {
        llzs_set_error("fir_adapt_matrix_power_f32: bad arguments (block=%d flt_len=%d inputs=%d nblk=%d P=%d R=%d slot=%d)", block,
                       flt_len, inputs, nblk, P, R, slot);
        return LLZ_ERR_ARG;
    }
    const adaptx_power_geom G = {inputs, P, R, slot, 4.f * delta};
    const float2 *rg = reinterpret_cast<const float2 *>(ring);
    float2 *dn = reinterpret_cast<float2 *>(den);
    hipStream_t st = as_stream(stream);
#define POWER(L)                                                                                                                 \
    hipLaunchKernelGGL((k_adaptx_power<L>), dim3((unsigned)nblk, (unsigned)((1 << L) / stream_threads(L))),                      \
                       dim3(stream_threads(L)), 0, st, rg, dn, G)
    ADAPT_DISPATCH(log2b, POWER)
#undef POWER
    LLZ_LAUNCH_CHECK("k_adaptx_power");
    return LLZ_OK;
}

// Block j of a call behind llzs_fir_matrix_mac_f32 of that block alone: ypart = [groups][outputs][block] complex; d, e, y =
// [outputs][pitch] (y may be null), the block's samples at [j block, (j + 1) block); den = the block's [block] denominators;
// g = [outputs][block] complex, written for the outputs whose mu is not zero; mu = [outputs] on the device.
extern "C" int llzs_fir_adapt_matrix_error_f32(int block, const float *ypart, const float *tw, const float *den, float *g,
                                               const float *mu, const float *d, float *e, float *y, int outputs, int groups,
                                               int j, long pitch, void *stream)
{
    int log2b;
    const bool ok = adapt_log2(block, &log2b);
    if (!ok || !adaptx_ports_ok(outputs) || groups < 1 || !(ypart && tw && den && g && mu && d && e) || j < 0 ||
        pitch < ((long)j + 1) * block) {
        llzs_set_error("fir_adapt_matrix_error_f32: bad arguments (block=%d outputs=%d groups=%d j=%d pitch=%ld)", block, outputs,
                       groups, j, pitch);
        return LLZ_ERR_ARG;
    }
    const adaptx_error_geom G = {outputs, groups, j, pitch};
    const float2 *Y = reinterpret_cast<const float2 *>(ypart), *TW = reinterpret_cast<const float2 *>(tw);
    const float2 *dn = reinterpret_cast<const float2 *>(den);
    float2 *gs = reinterpret_cast<float2 *>(g);
    hipStream_t st = as_stream(stream);
#define ERRK(L)                                                                                                                 \
    hipLaunchKernelGGL((k_adaptx_error<L>), dim3((unsigned)outputs), dim3(stream_threads(L)), 0, st, Y, TW, d, e, y, dn, gs, mu, G)
    ADAPT_DISPATCH(log2b, ERRK)
#undef ERRK
    LLZ_LAUNCH_CHECK("k_adaptx_error");
    return LLZ_OK;
}

// The weight update behind llzs_fir_adapt_matrix_error_f32 of the same block: w[o][i][p] += the constrained conj(X_{i,j-p}) g_o
// for every path and partition of every output whose mu is not zero; slot = the ring slot of the block's spectra.
extern "C" int llzs_fir_adapt_matrix_update_f32(int block, int flt_len, float *w, const float *tw, const float *ring,
                                                const float *g, const float *mu, int inputs, int outputs, int P, int R, int slot,
                                                void *stream)
{
    int log2b;
    const bool ok = adapt_log2(block, &log2b);
    if (!adapt_geom_ok(ok, block, flt_len, P, R, slot) || !adaptx_ports_ok(inputs) || !adaptx_ports_ok(outputs) ||
        !(w && tw && ring && g && mu)) {
        llzs_set_error("fir_adapt_matrix_update_f32: bad arguments (block=%d flt_len=%d inputs=%d outputs=%d P=%d R=%d slot=%d)",
                       block, flt_len, inputs, outputs, P, R, slot);
        return LLZ_ERR_ARG;
    }
    const adapt_update_geom G = {inputs, P, R, slot, flt_len};
    const int ppw = adapt_ppw((long)outputs * inputs * P), nq = (P + ppw - 1) / ppw;
    const dim3 grid((unsigned)inputs * (unsigned)nq, (unsigned)outputs);
    float2 *W = reinterpret_cast<float2 *>(w);
    const float2 *TW = reinterpret_cast<const float2 *>(tw), *rg = reinterpret_cast<const float2 *>(ring);
    const float2 *gs = reinterpret_cast<const float2 *>(g);
    hipStream_t st = as_stream(stream);
#define UPDATE(L) hipLaunchKernelGGL((k_adapt_update<L, true>), grid, dim3(stream_threads(L)), 0, st, W, TW, rg, gs, mu, G, ppw, nq)
    ADAPT_DISPATCH(log2b, UPDATE)
#undef UPDATE
    LLZ_LAUNCH_CHECK("k_adaptx_update");
    return LLZ_OK;
}
