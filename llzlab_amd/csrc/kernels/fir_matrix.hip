// fir_matrix.hip -- K4g: the many-in, many-out stream convolver (llz_fir_matrix_mc, include/llz_fir.h part 6): y_o = sum_i x_i *
// h_{o,i}, K4f (fir_stream.hip) with a sum over inputs.  One frequency-domain delay line per INPUT (a ring of R packed
// half-spectra and the last input block), tap spectra H[o][i][p][B], and output block j of output o is the last B samples of
// IDFT_N(sum_i sum_p X_{i,j-p} H_{o,i,p}): I forward and O inverse transforms per block where a bank of I O stream channels
// runs I O of each, and I rings where it keeps I O.
//
// Three kernels per call, ordered by the stream alone -- no device-scope fence, no atomic:
//   1. k_fir_matrix_fwd, grid (input, block of the call): (previous block, block) through the B-point transform and the forward
//      split into ring slot (head + j) mod R.  The blocks of a call do not depend on each other.  The carried last block is
//      double-buffered: block 0 reads prev_in, block k - 1 writes prev_out, the host swaps them.
//   2. k_fir_matrix_mac, grid (output, block of the call, bin tile x input group): a thread owns one bin (two neighbours, 16-byte
//      loads, from B = 512 on), walks its group's inputs ascending and p ascending within an input in ONE fma chain per bin that
//      starts at zero (bin 0: its DC and Nyquist halves separately), about 8 bins of ring and of H in flight, and writes the
//      partial spectrum Y[g][o][j][B].  A path (o, i) whose entry of `conn` is 0 (all its taps are zero) is skipped by a
//      workgroup-uniform branch: no traffic, and nothing of x_i -- not even a NaN -- reaches y_o.
//   3. k_fir_matrix_inv, grid (output, block): the G partials added g ascending, the inverse split, the inverse transform, the
//      last B samples stored non-temporally.
// G, the number of input groups, splits the sum over inputs over workgroups (64 inputs into 2 outputs would otherwise run on two
// workgroups); the host fixes it at init from (inputs, outputs, block).  The order of every sum is fixed by (G, inputs, P), so
// how calls group the blocks changes no bit and a fresh handle repeats its bits.  With every input but one at zero a bin's
// chain is K4f's chain with exact zeros added: the stream convolver's values.
// Flush: kernel 1 once per input on (last block, zeros) into slot `head` (free: the flush ends in a reset), then kernels 2 and
// 3 over the flush's blocks side by side, block j starting at p = j.
// All index arithmetic over outputs x inputs x partitions x bins is size_t.
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"
#include "fir_matrix.hpp"

namespace {

// 1. workgroup (i, j): the spectrum of input i's block pair (j - 1, j) into its ring slot
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_matrix_fwd(const float *__restrict__ in, const float2 *__restrict__ tw, float2 *__restrict__ ring,
                 const float *__restrict__ prev_in, float *__restrict__ prev_out, matrix_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, i = blockIdx.x, j = blockIdx.y;
    const float2 *spl = tw + B / 2;
    const float *irow = in + (size_t)i * (size_t)G.in_pitch;        // a flush has no input and never reads it
    const float *older = (G.flush || j == 0) ? prev_in + (size_t)i * B : irow + (size_t)(j - 1) * B;
    for (int t = tid; t < B; t += T) {
        const float nw = G.flush ? 0.f : irow[(size_t)j * B + t];
        lf[t] = older[t];
        lf[B + t] = nw;
        if (!G.flush && j == G.nblk - 1) prev_out[(size_t)i * B + t] = nw;      // the next call's previous block
    }
    part_fft_dif<LOG2B, T>(lds, tw, tid);
    float2 *slot = ring + ((size_t)i * (size_t)G.R + (size_t)((G.head + j) % G.R)) * B;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        float2 x[V];
        const int pos = (tid + g * T) * V;
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int q = pos + v;
            const float2 a = lds[q];
            x[v] = split_fwd(a, lds[mirror<LOG2B>(q)], spl[q]);
            if (q == 0) x[v] = split_fwd0(a);
        }
        store_bins<V>(slot + pos, x);
    }
}

// 2. workgroup (o, j, tile + tiles g): the partial spectrum of output o's block j over the inputs of group g
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_matrix_mac(const float2 *__restrict__ H, const float2 *__restrict__ ring, const unsigned char *__restrict__ conn,
                 float2 *__restrict__ Y, matrix_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), V = mac_v(LOG2B), TILES = mac_tiles(LOG2B);
    constexpr int U = 8 / V;                                // partitions in flight
    const int tid = threadIdx.x, o = blockIdx.x, j = blockIdx.y;
    const int tile = (int)blockIdx.z % TILES, g = (int)blockIdx.z / TILES;
    const int pos = (tile * T + tid) * V;
    const bool first = pos == 0;                            // owner of position 0, the packed bin
    const int jj = G.j0 + j;                                // the block's place behind `head`: only a flush starts past 0
    const int cur = (G.head + jj) % G.R, p0 = G.flush ? jj : 0;
    const int i0 = g * G.gsize, i1 = i0 + G.gsize < G.inputs ? i0 + G.gsize : G.inputs;
    float2 acc[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = float2{0.f, 0.f};
    for (int i = i0; i < i1; i++) {
        if (!conn[(size_t)o * (size_t)G.inputs + (size_t)i]) continue;      // the same for the whole workgroup
        const float2 *rc = ring + (size_t)i * (size_t)G.R * B + pos;
        const float2 *hc = H + ((size_t)o * (size_t)G.inputs + (size_t)i) * (size_t)G.P * B + pos;
        // slot of X_{j-p} = (cur - p) mod R
        auto step = [&](int pp) {
            int s = cur - pp;
            if (s < 0) s += G.R;
            float2 xv[V], h[V];
            load_bins<V>(rc + (size_t)s * B, xv);
            load_bins<V>(hc + (size_t)pp * B, h);
#pragma unroll
            for (int v = 0; v < V; v++) bin_mac(acc[v], xv[v], h[v], v == 0 && first);
        };
        int p = p0;
#pragma unroll 1
        for (; p + U <= G.P; p += U) {
#pragma unroll
            for (int u = 0; u < U; u++) step(p + u);
        }
#pragma unroll 1
        for (; p < G.P; p++) step(p);
    }
    store_bins<V>(Y + (((size_t)g * (size_t)G.outputs + (size_t)o) * (size_t)G.nblk + (size_t)j) * B + pos, acc);
}

// 3. workgroup (o, j): the partials added, g ascending; inverse split and transform; the last B samples out
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_matrix_inv(const float2 *__restrict__ Y, const float2 *__restrict__ tw, float *__restrict__ out, matrix_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, o = blockIdx.x, j = blockIdx.y;
    const float2 *spl = tw + B / 2;
    const size_t gstride = (size_t)G.outputs * (size_t)G.nblk * B;
    const float2 *y0 = Y + ((size_t)o * (size_t)G.nblk + (size_t)j) * B;
    float2 acc[M];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const int pos = (tid + g * T) * V;
        load_bins<V>(y0 + pos, &acc[g * V]);
        for (int gg = 1; gg < G.G; gg++) {
            float2 part[V];
            load_bins<V>(y0 + (size_t)gg * gstride + pos, part);
#pragma unroll
            for (int v = 0; v < V; v++) acc[g * V + v] = c_add(acc[g * V + v], part[v]);
        }
        store_bins<V>(lds + pos, &acc[g * V]);
    }
    __syncthreads();
    float2 zz[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int q = (tid + (m / V) * T) * V + m % V;
        zz[m] = split_inv(acc[m], lds[mirror<LOG2B>(q)], spl[q]);
        if (q == 0) zz[m] = split_inv0(acc[m]);
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; g++) store_bins<V>(lds + (tid + g * T) * V, &zz[g * V]);
    part_fft_dit_inv<LOG2B, T>(lds, tw, tid);
    float *orow = out + (size_t)o * (size_t)G.out_pitch;
    for (int t = tid; t < B; t += T) {
        const long n = (long)j * B + t;
        if (n < G.n_out) __builtin_nontemporal_store(lf[B + t], &orow[n]);
    }
}

template <int LOG2B>
int fwd_launch(const float *in, const float2 *tw, float2 *ring, const float *prev_in, float *prev_out, const matrix_geom &G,
               hipStream_t st)
{
    const dim3 grid((unsigned)G.inputs, (unsigned)G.nblk), wg(stream_threads(LOG2B));
    hipLaunchKernelGGL((k_fir_matrix_fwd<LOG2B>), grid, wg, 0, st, in, tw, ring, prev_in, prev_out, G);
    LLZ_LAUNCH_CHECK("k_fir_matrix_fwd");
    return LLZ_OK;
}

template <int LOG2B>
int mac_launch(const float2 *H, const float2 *ring, const unsigned char *conn, float2 *Y, const matrix_geom &G, hipStream_t st)
{
    const dim3 grid((unsigned)G.outputs, (unsigned)G.nblk, (unsigned)(mac_tiles(LOG2B) * G.G)), wg(stream_threads(LOG2B));
    hipLaunchKernelGGL((k_fir_matrix_mac<LOG2B>), grid, wg, 0, st, H, ring, conn, Y, G);
    LLZ_LAUNCH_CHECK("k_fir_matrix_mac");
    return LLZ_OK;
}

template <int LOG2B>
int inv_launch(const float2 *Y, const float2 *tw, float *out, const matrix_geom &G, hipStream_t st)
{
    const dim3 grid((unsigned)G.outputs, (unsigned)G.nblk), wg(stream_threads(LOG2B));
    hipLaunchKernelGGL((k_fir_matrix_inv<LOG2B>), grid, wg, 0, st, Y, tw, out, G);
    LLZ_LAUNCH_CHECK("k_fir_matrix_inv");
    return LLZ_OK;
}

} // namespace

// 1. the spectra of the nblk blocks of in ([inputs][in_pitch]) into ring slots (head + j) mod R; prev_in [inputs][block] is the
// block in front of block 0, prev_out (another buffer) receives block nblk - 1.  flush != 0: nblk == 1, the spectrum of
// (prev_in, zeros) into slot head; in and prev_out are not touched.  tw as llzs_fir_stream_f32's.
extern "C" int llzs_fir_matrix_fwd_f32(int block, const float *tw, float *ring, const float *prev_in, float *prev_out,
                                       const float *in, int inputs, int nblk, int flush, long in_pitch, int R, int head,
                                       void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    if (!matrix_shape_ok(ok, inputs, 1, nblk, 1, R, head) || !tw || !ring || !prev_in ||
        (!flush && (!in || !prev_out || prev_out == prev_in || in_pitch < (long)nblk * block)) || (flush && nblk != 1)) {
        llzs_set_error("fir_matrix_fwd_f32: bad arguments (block=%d inputs=%d nblk=%d R=%d head=%d flush=%d)", block, inputs, nblk,
                       R, head, flush);
        return LLZ_ERR_ARG;
    }
    matrix_geom G = {};
    G.inputs = inputs; G.R = R; G.head = head; G.nblk = nblk; G.flush = flush ? 1 : 0; G.in_pitch = in_pitch;
    const float2 *W = reinterpret_cast<const float2 *>(tw);
    float2 *rg = reinterpret_cast<float2 *>(ring);
    hipStream_t st = as_stream(stream);
#define FWD(L) fwd_launch<L>(in, W, rg, prev_in, prev_out, G, st)
    STREAM_DISPATCH(log2b, FWD)
#undef FWD
}

// 2. ypart[g][o][j][block] = sum over the connected inputs i of group g (inputs g gsize .. , ascending) and p ascending of
// ring_i[(head + j - p) mod R] H[o][i][p]; flush != 0: the launch's block j is block j0 + j of the flush and starts at p =
// j0 + j (j0 + nblk <= P; else j0 == 0).  hspec: [outputs][inputs][P][block] as llz_host_stream_spectra builds a row; conn:
// [outputs][inputs] bytes, 0 = the path is skipped.
extern "C" int llzs_fir_matrix_mac_f32(int block, const float *hspec, const float *ring, const unsigned char *conn, float *ypart,
                                       int inputs, int outputs, int nblk, int flush, int j0, int P, int R, int head,
                                       int groups, int group_size, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    if (!matrix_shape_ok(ok, inputs, outputs, nblk, P, R, head) || !hspec || !ring || !conn || !ypart ||
        !matrix_groups_ok(block, inputs, nblk, flush, j0, P, groups, group_size)) {
        llzs_set_error("fir_matrix_mac_f32: bad arguments (block=%d inputs=%d outputs=%d nblk=%d j0=%d P=%d R=%d head=%d groups=%d x "
                       "%d)", block, inputs, outputs, nblk, j0, P, R, head, groups, group_size);
        return LLZ_ERR_ARG;
    }
    matrix_geom G = {};
    G.inputs = inputs; G.outputs = outputs; G.P = P; G.R = R; G.head = head; G.nblk = nblk; G.flush = flush ? 1 : 0;
    G.j0 = j0; G.G = groups; G.gsize = group_size;
    const float2 *H = reinterpret_cast<const float2 *>(hspec), *rg = reinterpret_cast<const float2 *>(ring);
    float2 *Y = reinterpret_cast<float2 *>(ypart);
    hipStream_t st = as_stream(stream);
#define MAC(L) mac_launch<L>(H, rg, conn, Y, G, st)
    STREAM_DISPATCH(log2b, MAC)
#undef MAC
}

// 3. out[o][j block ..) = the last block samples of the inverse real transform of sum_g ypart[g][o][j], g ascending; the
// first n_out <= nblk block samples of every output are stored ([outputs][out_pitch])
extern "C" int llzs_fir_matrix_inv_f32(int block, const float *ypart, const float *tw, float *out, int outputs, int nblk,
                                       int groups, long n_out, long out_pitch, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    if (!matrix_shape_ok(ok, 1, outputs, nblk, 1, 1, 0) || !ypart || !tw || !out || groups < 1 || n_out < 1 ||
        n_out > (long)nblk * block || out_pitch < n_out) {
        llzs_set_error("fir_matrix_inv_f32: bad arguments (block=%d outputs=%d nblk=%d groups=%d n_out=%ld out_pitch=%ld)", block,
                       outputs, nblk, groups, n_out, out_pitch);
        return LLZ_ERR_ARG;
    }
    matrix_geom G = {};
    G.outputs = outputs; G.nblk = nblk; G.G = groups; G.n_out = n_out; G.out_pitch = out_pitch;
    const float2 *Y = reinterpret_cast<const float2 *>(ypart), *W = reinterpret_cast<const float2 *>(tw);
    hipStream_t st = as_stream(stream);
#define INV(L) inv_launch<L>(Y, W, out, G, st)
    STREAM_DISPATCH(log2b, INV)
#undef INV
}
