// adapt_steps.hpp -- what the two adaptive filters share: fir_adapt.hip (K4h, llz_adapt_mc) and fir_adapt_matrix.hip (K4i,
// llz_adapt_matrix_mc).  The tail of the error kernels behind the inverse transform (y, e, the frozen return, the spectrum of
// (0_B, e), G = mu E / den), the constrained weight update as one kernel template that both files instantiate, and the launch
// preamble of their launchers: the block sizes, the dispatch over the six of them, the part of the geometry check that does not
// count ports, and the partitions per update workgroup.  Written once so that "one input has llz_adapt_mc's bits", "the
// grouping changes no bit" and "a frozen row keeps its bits" hold by construction in both files.  The scalings are K4h's (see
// fir_adapt.hip): ring X' = 2 X, W' = W / (2 N), den' = 4 D + 4 delta, the window of the constraint scales by 1 / (4 N^2).
//
// The shapes are chosen by the compiler's register counts (DESIGN.md, K4h "Shared code"): the update is a __global__ template
// and not a __forceinline__ step called from two kernels, which cost 16 VGPRs at B = 1024 and 58 at B = 2048; the tail is a
// __forceinline__ step that takes the denominators of a position group through a callable.
#pragma once
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"

namespace {

// The error tail.  On entry lds holds the inverse transform of the output block's spectrum (behind part_fft_dit_inv's barrier)
// and pos[] the positions the thread owns.  y = the last B real samples and e = d - y go to row `row` + t of y (may be null) and
// e; (0_B, e) is the image of the error's transform: the first half is read by nobody behind the inverse's barrier, lf[B + t]
// only by the thread that writes it here.  keep != null: the call's last block, src[t] is handed over to keep[t] in the same
// walk (K4h: the input block becomes the next call's previous block).  mu == 0: frozen, the same for the whole workgroup,
// nothing more is written.  Else gc[position] = mu E / den, where den(g, dn) gives the two denominators of each of the V
// positions from pos[g] on: equal but for position 0, the packed bin, whose halves are two real bins.
template <int LOG2B, class DEN>
__device__ __forceinline__ void adapt_error_tail(float2 *lds, const float2 *__restrict__ tw, int tid, const int *pos,
                                                 const float *__restrict__ drow, float *__restrict__ e, float *__restrict__ y,
                                                 size_t row, float *keep, const float *src, float mu, float2 *__restrict__ gc,
                                                 DEN den)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    float *lf = reinterpret_cast<float *>(lds);
    const float2 *spl = tw + B / 2;
    const bool first = tid == 0;                            // owner of position 0, the packed bin
    for (int t = tid; t < B; t += T) {
        const float yv = lf[B + t], ev = drow[t] - yv;
        __builtin_nontemporal_store(ev, &e[row + t]);
        if (y) __builtin_nontemporal_store(yv, &y[row + t]);
        lf[t] = 0.f;
        lf[B + t] = ev;
        if (keep) keep[t] = src[t];
    }
    if (mu == 0.f) return;

    part_fft_dif<LOG2B, T>(lds, tw, tid);
    float2 gv[M];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        float2 dn[V];
        den(g, dn);
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int m = g * V + v, i = pos[g] + v;
            const float2 a = lds[i];
            float2 ee = split_fwd(a, lds[mirror<LOG2B>(i)], spl[i]);
            if (m == 0 && first) ee = split_fwd0(a);
            gv[m] = float2{mu * ee.x / dn[v].x, mu * ee.y / dn[v].y};
        }
    }
#pragma unroll
    for (int g = 0; g < NG; g++) store_bins<V>(gc + pos[g], &gv[g * V]);
}

// one update launch: `inputs` rings of R slots of B bins; a row of weights is P partitions of B bins
struct adapt_update_geom {
    int inputs;                 // weight rows per row of G (K4h: 1)
    int P, R, cur;              // partitions, ring slots, the slot of the block's spectra
    int flt_len;
};

// The constrained weight update: for the workgroup's partitions p, W_p += the forward transform of the windowed inverse
// transform of conj(X_{j-p}) G; every sample t >= min(B, flt_len - p B) is zeroed, the kept ones scaled by 1 / (4 N^2).
//   PATHS false (K4h): workgroup (c, q) -> channel c: ring c, weight row c, row c of G and mu; W: [channels][P][B];
//   PATHS true (K4i):  workgroup (i nq + q, o) -> path (o, i): ring i, weight row o inputs + i, row o of G and mu;
//                      W: [outputs][inputs][P][B].
// Partitions [q ppw, min(P, (q + 1) ppw)).  A row whose mu is zero is frozen: its workgroups return at once and W keeps its
// bits.  No two workgroups touch one W_p: no atomics, no fences, and ppw cannot change a bit.
template <int LOG2B, bool PATHS>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_adapt_update(float2 *__restrict__ W, const float2 *__restrict__ tw, const float2 *__restrict__ ring,
               const float2 *__restrict__ gs, const float *__restrict__ mus, adapt_update_geom G, int ppw, int nq)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x;
    const int own = PATHS ? blockIdx.y : blockIdx.x;        // the row of G and mu
    const int in = PATHS ? (int)(blockIdx.x / (unsigned)nq) : own;
    const int q = PATHS ? (int)(blockIdx.x % (unsigned)nq) : (int)blockIdx.y;
    if (mus[own] == 0.f) return;                            // frozen: W keeps its bits
    const float2 *spl = tw + B / 2;
    const float2 *rc = ring + (size_t)in * (size_t)G.R * B;
    float2 *wc = W + (PATHS ? (size_t)own * (size_t)G.inputs + (size_t)in : (size_t)own) * (size_t)G.P * B;
    const float2 *gc = gs + (size_t)own * B;
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
            const int i = pos[m / V] + m % V;
            zz[m] = split_inv(dw[m], lds[mirror<LOG2B>(i)], spl[i]);
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
            const int i = pos[m / V] + m % V;
            const float2 a = lds[i];
            dw[m] = split_fwd(a, lds[mirror<LOG2B>(i)], spl[i]);
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

// ------------------------------------------------------------------------------------------------ the launch preamble
// block = 2^*log2b, 64 .. 2048: at 4096 a thread would own 16 bins
bool adapt_log2(int block, int *log2b) { return stream_log2(block, log2b) && *log2b <= 11; }

// `call(LOG2B);` for the block size; call: a macro of one argument
#define ADAPT_DISPATCH(log2b, call)                                                                                              \
    switch (log2b) {                                                                                                             \
    case 6: call(6); break;                                                                                                      \
    case 7: call(7); break;                                                                                                      \
    case 8: call(8); break;                                                                                                      \
    case 9: call(9); break;                                                                                                      \
    case 10: call(10); break;                                                                                                    \
    default: call(11); break;                                                                                                    \
    }

// the part of a launch's geometry that does not count channels or ports
bool adapt_geom_ok(bool log2ok, int block, int flt_len, int P, int R, int slot)
{
    return log2ok && flt_len >= 1 && flt_len <= LLZS_FIR_PART_MAX_TAPS && P == (flt_len + block - 1) / block && R >= P &&
           slot >= 0 && slot < R;
}

// partitions per update workgroup for `pairs` (weight row, partition) pairs: the adapt_ppw override clamped to 1 .. 64, else one
// where the grid would otherwise not fill the device (fewer than 4096 pairs: 16 workgroups per CU), else 4
int adapt_ppw(long pairs)
{
    const int tuned = llzs_tune(LLZS_TUNE_ADAPT_PPW);
    return tuned >= 1 ? (tuned < 64 ? tuned : 64) : pairs >= 4096 ? 4 : 1;
}

} // namespace
