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
//   error:  grid (output): the partials added g ascending, the inverse split and transform (K4g's inverse to the letter), y, e =
//           d - y, and where mu_o != 0 E = the spectrum of (0_B, e), G_o = mu_o E / den[j] into an [outputs][B] scratch (K4h's
//           filter tail to the letter);
//   update: grid ((input, group of partitions), output): W_{o,i,p} += the constrained conj(X_{i,j-p}) G_o, K4h's update loop to
//           the letter on input i's ring and path (o, i)'s weights.
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

namespace {

struct adaptx_geom {
    int inputs, outputs, P, R;
    int cur;                    // the ring slot of the block (power: of block 0 of the launch)
    int j;                      // the block of the call
    int groups;                 // input groups of the partial spectra
    int flt_len;
    long pitch;                 // row pitch of d, e and y
    float delta4;               // 4 delta: the regularisation against the doubled spectra's power
};

// power: workgroup (j, tile) -> block j of the call, bins [tile T, (tile + 1) T).  den: [nblk][B] (dx, dy)
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adaptx_power(const float2 *__restrict__ ring, float2 *__restrict__ den, adaptx_geom G)
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
               adaptx_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, o = blockIdx.x;
    const float2 *spl = tw + B / 2;
    const size_t gstride = (size_t)G.outputs * B;
    const float2 *y0 = Y + (size_t)o * B;
    const size_t row = (size_t)o * (size_t)G.pitch + (size_t)G.j * B;
    const float *drow = d + row;
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
    // y: the last B real samples; e = d - y; (0, e) is the image of the error's transform
    for (int t = tid; t < B; t += T) {
        const float yv = lf[B + t], ev = drow[t] - yv;
        __builtin_nontemporal_store(ev, &e[row + t]);
        if (y) __builtin_nontemporal_store(yv, &y[row + t]);
        lf[t] = 0.f;
        lf[B + t] = ev;
    }
    if (mu == 0.f) return;                                  // frozen: the same for the whole workgroup

    part_fft_dif<LOG2B, T>(lds, tw, tid);
    float2 gv[M];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        float2 dn[V];
        load_bins<V>(den + pos[g], dn);
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int m = g * V + v, i = pos[g] + v;
            const float2 a = lds[i];
            float2 ee = split_fwd(a, lds[mirror<LOG2B>(i)], spl[i]);
            if (m == 0 && first) ee = split_fwd0(a);
            gv[m] = float2{mu * ee.x / dn[v].x, mu * ee.y / dn[v].y};
        }
    }
    float2 *gc = gs + (size_t)o * B;
#pragma unroll
    for (int g = 0; g < NG; g++) store_bins<V>(gc + pos[g], &gv[g * V]);
}

// update: workgroup (i nq + q, o) -> path (o, i), partitions [q ppw, min(P, (q + 1) ppw)).  W: [outputs][inputs][P][B]
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adaptx_update(float2 *__restrict__ W, const float2 *__restrict__ tw, const float2 *__restrict__ ring,
                const float2 *__restrict__ gs, const float *__restrict__ mus, adaptx_geom G, int ppw, int nq)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, o = blockIdx.y;
    const int i = (int)(blockIdx.x / (unsigned)nq), q = (int)(blockIdx.x % (unsigned)nq);
    if (mus[o] == 0.f) return;                              // frozen: W keeps its bits
    const float2 *spl = tw + B / 2;
    const float2 *rc = ring + (size_t)i * (size_t)G.R * B;
    float2 *wc = W + ((size_t)o * (size_t)G.inputs + (size_t)i) * (size_t)G.P * B;
    const float2 *gc = gs + (size_t)o * B;
    constexpr float scale = 1.f / (16.f * (float)B * (float)B);        // 1 / (4 N^2)

    int pos[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) pos[g] = (tid + g * T) * V;
    const bool first = tid == 0;
    float2 gv[M];
#pragma unroll
    for (int g = 0; g < NG; g++) load_bins<V>(gc + pos[g], &gv[g * V]);

    const int p0 = q * ppw, p1 = p0 + ppw < G.P ? p0 + ppw : G.P;
    for (int p = p0; p < p1; p++) {
        int s = G.cur - p;
        if (s < 0) s += G.R;
        const float2 *xs = rc + (size_t)s * B;
        float2 *wp = wc + (size_t)p * B;
        float2 dw[M];
#pragma unroll
        for (int g = 0; g < NG; g++) {
            float2 xv[V];
            load_bins<V>(xs + pos[g], xv);
#pragma unroll
            for (int v = 0; v < V; v++) {
                const int m = g * V + v;
                dw[m] = c_mul<true>(gv[m], xv[v]);          // G conj(X)
                if (m == 0 && first) dw[m] = float2{xv[v].x * gv[m].x, xv[v].y * gv[m].y};
            }
        }
        // inverse split, inverse transform
        __syncthreads();                                    // the partition before: every mirror read is done
#pragma unroll
        for (int g = 0; g < NG; g++) store_bins<V>(lds + pos[g], &dw[g * V]);
        __syncthreads();
        float2 zz[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int k = pos[m / V] + m % V;
            zz[m] = split_inv(dw[m], lds[mirror<LOG2B>(k)], spl[k]);
            if (m == 0 && first) zz[m] = split_inv0(dw[m]);
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NG; g++) store_bins<V>(lds + pos[g], &zz[g * V]);
        part_fft_dit_inv<LOG2B, T>(lds, tw, tid);
        // the constraint: samples [0, lim) kept (and scaled), the rest zero
        const long left = (long)G.flt_len - (long)p * B;
        const int lim = left < B ? (int)left : B;
        for (int t = tid; t < B; t += T) {
            lf[t] = t < lim ? lf[t] * scale : 0.f;
            lf[B + t] = 0.f;
        }
        part_fft_dif<LOG2B, T>(lds, tw, tid);
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int k = pos[m / V] + m % V;
            const float2 a = lds[k];
            dw[m] = split_fwd(a, lds[mirror<LOG2B>(k)], spl[k]);
            if (m == 0 && first) dw[m] = split_fwd0(a);
        }
#pragma unroll
        for (int g = 0; g < NG; g++) {
            float2 w[V];
            load_bins<V>(wp + pos[g], w);
#pragma unroll
            for (int v = 0; v < V; v++) w[v] = c_add(w[v], dw[g * V + v]);
            store_bins<V>(wp + pos[g], w);
        }
    }
}

// block = 2^*log2b, 64 .. 2048
bool adaptx_log2(int block, int *log2b) { return stream_log2(block, log2b) && *log2b <= 11; }

#define ADAPTX_DISPATCH(log2b, call)                                                                                             \
    switch (log2b) {                                                                                                             \
    case 6: call(6); break;                                                                                                      \
    case 7: call(7); break;                                                                                                      \
    case 8: call(8); break;                                                                                                      \
    case 9: call(9); break;                                                                                                      \
    case 10: call(10); break;                                                                                                    \
    default: call(11); break;                                                                                                    \
    }

bool adaptx_geom_ok(bool log2ok, int block, int flt_len, int inputs, int outputs, int P, int R, int slot)
{
    return log2ok && inputs >= 1 && inputs <= 4096 && outputs >= 1 && outputs <= 4096 && flt_len >= 1 &&
           flt_len <= LLZS_FIR_PART_MAX_TAPS && P == (flt_len + block - 1) / block && R >= P && slot >= 0 && slot < R;
}

} // namespace

// den[j][block] (two floats per position) = delta + the power of the P spectra behind block j of every input, for the nblk
// blocks whose spectra lie in ring slots (slot + j) mod R; ring = [inputs][R][block] complex as llzs_fir_matrix_fwd_f32 fills it.
extern "C" int llzs_fir_adapt_matrix_power_f32(int block, int flt_len, const float *ring, float *den, float delta, int inputs,
                                               int nblk, int P, int R, int slot, void *stream)
{
    int log2b;
    const bool ok = adaptx_log2(block, &log2b);
    if (!adaptx_geom_ok(ok, block, flt_len, inputs, 1, P, R, slot) || !ring || !den || nblk < 1 || !(delta > 0.f)) {
        llzs_set_error("fir_adapt_matrix_power_f32: bad arguments (block=%d flt_len=%d inputs=%d nblk=%d P=%d R=%d slot=%d)", block,
                       flt_len, inputs, nblk, P, R, slot);
        return LLZ_ERR_ARG;
    }
    adaptx_geom G = {};
    G.inputs = inputs; G.P = P; G.R = R; G.cur = slot; G.flt_len = flt_len; G.delta4 = 4.f * delta;
    const float2 *rg = reinterpret_cast<const float2 *>(ring);
    float2 *dn = reinterpret_cast<float2 *>(den);
    hipStream_t st = as_stream(stream);
#define POWER(L)                                                                                                                 \
    hipLaunchKernelGGL((k_adaptx_power<L>), dim3((unsigned)nblk, (unsigned)((1 << L) / stream_threads(L))),                      \
                       dim3(stream_threads(L)), 0, st, rg, dn, G)
    ADAPTX_DISPATCH(log2b, POWER)
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
    const bool ok = adaptx_log2(block, &log2b);
    if (!ok || outputs < 1 || outputs > 4096 || groups < 1 || !(ypart && tw && den && g && mu && d && e) || j < 0 ||
        pitch < ((long)j + 1) * block) {
        llzs_set_error("fir_adapt_matrix_error_f32: bad arguments (block=%d outputs=%d groups=%d j=%d pitch=%ld)", block, outputs,
                       groups, j, pitch);
        return LLZ_ERR_ARG;
    }
    adaptx_geom G = {};
    G.outputs = outputs; G.groups = groups; G.j = j; G.pitch = pitch;
    const float2 *Y = reinterpret_cast<const float2 *>(ypart), *TW = reinterpret_cast<const float2 *>(tw);
    const float2 *dn = reinterpret_cast<const float2 *>(den);
    float2 *gs = reinterpret_cast<float2 *>(g);
    hipStream_t st = as_stream(stream);
#define ERRK(L)                                                                                                                 \
    hipLaunchKernelGGL((k_adaptx_error<L>), dim3((unsigned)outputs), dim3(stream_threads(L)), 0, st, Y, TW, d, e, y, dn, gs, mu, G)
    ADAPTX_DISPATCH(log2b, ERRK)
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
    const bool ok = adaptx_log2(block, &log2b);
    if (!adaptx_geom_ok(ok, block, flt_len, inputs, outputs, P, R, slot) || !(w && tw && ring && g && mu)) {
        llzs_set_error("fir_adapt_matrix_update_f32: bad arguments (block=%d flt_len=%d inputs=%d outputs=%d P=%d R=%d slot=%d)",
                       block, flt_len, inputs, outputs, P, R, slot);
        return LLZ_ERR_ARG;
    }
    adaptx_geom G = {};
    G.inputs = inputs; G.outputs = outputs; G.P = P; G.R = R; G.cur = slot; G.flt_len = flt_len;
    const int tuned = llzs_tune(LLZS_TUNE_ADAPT_PPW);
    const int ppw = tuned >= 1 ? (tuned < 64 ? tuned : 64) : (long)outputs * inputs * P >= 4096 ? 4 : 1;
    const int nq = (P + ppw - 1) / ppw;
    const dim3 grid((unsigned)inputs * (unsigned)nq, (unsigned)outputs);
    float2 *W = reinterpret_cast<float2 *>(w);
    const float2 *TW = reinterpret_cast<const float2 *>(tw), *rg = reinterpret_cast<const float2 *>(ring);
    const float2 *gs = reinterpret_cast<const float2 *>(g);
    hipStream_t st = as_stream(stream);
#define UPDATE(L) hipLaunchKernelGGL((k_adaptx_update<L>), grid, dim3(stream_threads(L)), 0, st, W, TW, rg, gs, mu, G, ppw, nq)
    ADAPTX_DISPATCH(log2b, UPDATE)
#undef UPDATE
    LLZ_LAUNCH_CHECK("k_adaptx_update");
    return LLZ_OK;
}
