// fir_stream.hip -- K4f: the block convolver that keeps spectra between calls (llz_fir_stream_mc, include/llz_fir.h part 5): a
// uniformly partitioned overlap-save with a FREQUENCY-DOMAIN DELAY LINE.  The block B is the caller's (64 .. 4096), the taps are
// cut into P = ceil(flt_len / B) partitions, and the spectra of the last input blocks of every channel stay in device memory
// in a ring of R slots.  A call of k blocks transforms only its k new blocks; output block j is the last B samples of
// IDFT_N(sum_{p < P} X_{j-p} H_p), N = 2 B, X_q the spectrum of input blocks (q - 1, q).  A call of one block reads P B 8 bytes
// of ring per channel (1 MB at 131073 taps, at any B) where K4d transforms and re-reads the whole history.
//
// Choices, with their reasons:
//   * Real transform: one real block pair per spectrum (K4d's pairing of blocks k and k + Kh of ONE call does not carry across
//     calls), so the N real samples go as B complex values z[i] = x[2 i] + j x[2 i + 1] through a B-point transform (the passes
//     of part_fft.hpp, shared with fir_part.hip) and a split step to the half-spectrum: B packed bins, bins 1 .. B - 1 complex,
//     DC and Nyquist -- both real -- as the two halves of bin 0.  The inverse runs the same steps backwards.  Everything stays
//     in the order the decimation-in-frequency transform leaves (position i holds bin bitrev(i)): the host builds H_p and the
//     split twiddles in that order, so nothing is bit-reversed on the device.
//   * Scaling: the split steps leave out their halvings and the inverse its 1 / B: H_p carries 1 / (2 N), a power of two.
//   * One fused kernel, one launch per call, one workgroup per channel, which walks the call's blocks in order.  A thread owns
//     the same positions (bins) for the whole kernel: it computes its bins of the new spectrum from the LDS image (its own
//     position and the mirror bin's), keeps them in registers for p = 0, writes them to ring slot (head + j) mod R, sums
//     X_{j-p} H_p over p ascending from the ring -- no atomics, the same call gives the same bits -- and hands the sum to the
//     inverse split through LDS.  The ring bins a thread reads are those it wrote itself or an earlier launch wrote: no
//     device-scope fence.  Bin 0 multiplies its two real halves separately.
//   * The ring head comes by value with the launch (the host advances it): no device-side counter.  A launch captured into a
//     graph would therefore replay one slot: not supported (llz_fir.h).
//   * Workgroup sized to the block, min(B, 256) threads, instead of several channels per 256-thread workgroup: a 64-sample
//     block is exactly one wave, nothing idles in the product (where the kernel spends its time: P steps against one
//     transform pair), a channel's arithmetic involves that channel's values alone by construction, and there is no ragged
//     last group to mask.  From B = 512 on a thread owns B / 256 bins as pairs of neighbours: 16-byte loads of ring and H.
//   * The product's loads do not depend on each other, only the sums do: the partition loop is unrolled so that about 8 bins of
//     ring and of H are in flight per thread.
//   * Flush: behind the input only one spectrum is not zero, that of (last input block, zeros), so the flush's blocks do not
//     depend on each other and run as a grid of (channel, block) workgroups through the same kernel: block j transforms that
//     pair itself, starts its sum at p = j with it (the terms before are zero spectra), goes on through the ring and writes
//     no slot.  Walked in sequence by one workgroup per channel the flush of a long filter would take P times a call.
//   * All index arithmetic over channels x slots x bins is size_t / long.
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"

namespace {

// K4f: workgroup c (a flush: (c, block)) -> channel c.  tw: [B / 2] W_B^m, then [B] split twiddles W_N^bitrev(i) by position.
// BANK: H is [channels][P][B], channel c's own spectra
template <int LOG2B, bool BANK>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_stream(const float *__restrict__ in, float *__restrict__ out, const float2 *__restrict__ H, const float2 *__restrict__ tw,
             float2 *ring, float *prev, stream_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    constexpr int U = M >= 8 ? 1 : 8 / M;                   // partitions in flight
    __shared__ __align__(16) float2 lds[B];              // store_bins<2> writes it 16 bytes at a time
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, c = blockIdx.x;
    const float2 *spl = tw + B / 2;
    const float *irow = in + (size_t)c * (size_t)G.in_pitch;      // a flush has no input and never reads it
    float *orow = out + (size_t)c * (size_t)G.out_pitch;
    float *prow = prev + (size_t)c * B;
    float2 *rc = ring + (size_t)c * (size_t)G.R * B;
    const float2 *hc = BANK ? H + (size_t)c * (size_t)G.P * B : H;

    // the positions this thread owns: NG groups of V neighbours
    int pos[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) pos[g] = (tid + g * T) * V;
    const bool first = tid == 0;                            // owner of position 0, the packed bin

    const int jb = G.flush ? (int)blockIdx.y : 0, je = G.flush ? jb + 1 : G.nblk;
    for (int j = jb; j < je; j++) {
        const int cur = (G.head + j) % G.R;
        float2 acc[M];
        // (previous block, this block) as B complex values; a flush block: (the last input block, zeros) -- the one spectrum
        // behind the input that is not zero, met by partition j.  The last reads of the LDS image (the stores of the block
        // before) were of lf[B + t] by the thread that writes it here, behind the inverse transform's barrier.
        const int p0 = G.flush ? j : 0;
        const float *older = (G.flush || j == 0) ? prow : irow + (size_t)(j - 1) * B;
        for (int t = tid; t < B; t += T) {
            lf[t] = older[t];
            lf[B + t] = G.flush ? 0.f : irow[(size_t)j * B + t];
        }
        part_fft_dif<LOG2B, T>(lds, tw, tid);
        // forward split (stream_bins.hpp) into the bins this thread owns
        float2 x[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int i = pos[m / V] + m % V;
            const float2 a = lds[i];
            x[m] = split_fwd(a, lds[mirror<LOG2B>(i)], spl[i]);
            if (m == 0 && first) x[m] = split_fwd0(a);
        }
        float2 *slot = rc + (size_t)cur * B;
        const float2 *h0 = hc + (size_t)p0 * B;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            float2 h[V];
            if (!G.flush) store_bins<V>(slot + pos[g], &x[g * V]);
            load_bins<V>(h0 + pos[g], h);
#pragma unroll
            for (int v = 0; v < V; v++) {
                acc[g * V + v] = float2{0.f, 0.f};
                bin_mac(acc[g * V + v], x[g * V + v], h[v], g == 0 && v == 0 && first);
            }
        }
        int p = p0 + 1;
        // Y = sum_p X_{j-p} H_p, p ascending; slot of X_{j-p} = (cur - p) mod R
        auto step = [&](int pp) {
            int s = cur - pp;
            if (s < 0) s += G.R;
            const float2 *xs = rc + (size_t)s * B, *hs = hc + (size_t)pp * B;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                float2 xv[V], h[V];
                load_bins<V>(xs + pos[g], xv);
                load_bins<V>(hs + pos[g], h);
#pragma unroll
                for (int v = 0; v < V; v++) bin_mac(acc[g * V + v], xv[v], h[v], g == 0 && v == 0 && first);
            }
        };
#pragma unroll 1
        for (; p + U <= G.P; p += U) {
#pragma unroll
            for (int u = 0; u < U; u++) step(p + u);
        }
#pragma unroll 1
        for (; p < G.P; p++) step(p);

        // inverse split (stream_bins.hpp) through LDS
        __syncthreads();                                    // every mirror read of the forward split is done
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
        // the last B real samples: z'[B / 2 ..) as floats
        for (int t = tid; t < B; t += T) {
            const long n = (long)j * B + t;
            if (n < G.n_out) __builtin_nontemporal_store(lf[B + t], &orow[n]);
        }
    }
    if (!G.flush) {
        // the frame's last block is the next call's previous block
        for (int t = tid; t < B; t += T) prow[t] = irow[(size_t)(G.nblk - 1) * B + t];
    }
}

template <int LOG2B>
int stream_launch(bool bank, const float *in, float *out, const float2 *H, const float2 *tw, float2 *ring, float *prev,
                  const stream_geom &G, int channels, hipStream_t st)
{
    const dim3 grid((unsigned)channels, G.flush ? (unsigned)G.nblk : 1u), wg(stream_threads(LOG2B));
    if (bank) hipLaunchKernelGGL((k_fir_stream<LOG2B, true>), grid, wg, 0, st, in, out, H, tw, ring, prev, G);
    else hipLaunchKernelGGL((k_fir_stream<LOG2B, false>), grid, wg, 0, st, in, out, H, tw, ring, prev, G);
    LLZ_LAUNCH_CHECK("k_fir_stream");
    return LLZ_OK;
}

} // namespace

// One launch: nblk blocks of every channel in order (flush = 0), or the nblk zero blocks of a flush side by side (flush = 1,
// in unused, ring and prev only read).  hspec: [P][block] packed bins (bank: [channels][P][block]) as llz_host_stream_spectra
// builds them; tw: [block / 2] W_block^m then [block] W_(2 block)^bitrev(i); ring: [channels][R][block] complex; prev:
// [channels][block].  Stores the first n_out samples of each channel's nblk blocks.
extern "C" int llzs_fir_stream_f32(int block, const float *hspec, int bank, const float *tw, float *ring, float *prev,
                                   const float *in, float *out, int channels, int nblk, int flush, long n_out, long in_pitch,
                                   long out_pitch, int P, int R, int head, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    const stream_geom G = {P, R, head, nblk, flush ? 1 : 0, n_out, in_pitch, out_pitch};
    if (!stream_launch_ok(G, ok, block, channels, hspec && tw && ring && prev && out, in)) {
        llzs_set_error("fir_stream_f32: bad arguments (block=%d channels=%d nblk=%d P=%d R=%d head=%d n_out=%ld)", block, channels,
                       nblk, P, R, head, n_out);
        return LLZ_ERR_ARG;
    }
    const float2 *H = reinterpret_cast<const float2 *>(hspec), *W = reinterpret_cast<const float2 *>(tw);
    float2 *rg = reinterpret_cast<float2 *>(ring);
    hipStream_t st = as_stream(stream);
    const bool bk = bank != 0;
#define PLAIN(L) stream_launch<L>(bk, in, out, H, W, rg, prev, G, channels, st)
    STREAM_DISPATCH(log2b, PLAIN)
#undef PLAIN
}
