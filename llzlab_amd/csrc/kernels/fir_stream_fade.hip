// fir_stream_fade.hip -- K4f while tap rows fade (llz_fir_xfade_stream_mc, include/llz_fir.h part 5): k_fir_stream's walk -- one
// workgroup per channel, or per (channel, block) in a flush, the same thread-to-bin ownership, the same ring -- with a second
// table of spectra (the NEW taps) beside the handle's.  For the span of the fade a fading row runs both filters on the same
// input and blends the two outputs sample by sample in the time domain (a ramp is not a per-bin operation):
//     y[n] = fmaf(w[n], y_new[n] - y_old[n], y_old[n]),   w[n] = (float)n / (float)(F B), n counted from the fade's first sample.
// The delay line holds INPUT spectra, so both filters share the forward transform and every ring slot: a fading block costs a
// second product sum and a second inverse transform.  Calls with no fade in flight run k_fir_stream (fir_stream.hip); the two
// kernels share the split steps and the launch preamble of stream_bins.hpp.
//
// Choices, with their reasons:
//   * A workgroup-uniform branch per block: a row that does not fade, and a block of a fading row past the fade's end, go through
//     the plain chain (bin_mac over p ascending from a zero accumulator as in k_fir_stream, and the split steps it calls too:
//     every operation there is an add, a subtract, a product that feeds an fma as its addend, or an explicit fma, so there is
//     nothing for the compiler to contract differently) against the old spectra or, past the end, the new ones: the bits of
//     k_fir_stream.  The old filter's half of a fading block is that same chain.
//   * B <= 1024 (a thread owns 1 .. 4 bins): ONE pass over the ring with two accumulator sets -- every ring bin is loaded once and
//     multiplied into both sums; the ring is the traffic the kernel is bound by.  B = 2048 / 4096 (8 / 16 bins per thread, where
//     k_fir_stream already takes 162 / 238 VGPRs): TWO passes in sequence through one code site.  What has to outlive a
//     pass -- the block's own spectrum (the p = 0 term of the second sum), then the old output's B / T samples per thread --
//     waits in a second LDS array of B 8 bytes, each thread in slots of its own, so that the product loop keeps k_fir_stream's
//     register footprint (held in registers, 4096 took 256 VGPRs, 106 AGPRs and spilt 4 SGPRs).  The ring is read twice (from
//     L2 the second time where a channel's P B 8 bytes fit).
//   * The head, fade_done and fade_blocks come by value with the launch: no device-side counter, no atomics.  The weight depends
//     on the sample's index within the fade alone, so how calls group the blocks does not change a bit.
//   * w[n] by one IEEE division of two exact floats (n < F B <= 2^24): correctly rounded.
//   * All index arithmetic over channels x slots x bins is size_t / long.
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"

namespace {

struct fade_geom : stream_geom, fade_pos {};   // block j of this launch is block fade_done + j of the fade

// workgroup c (a flush: (c, block)) -> channel c.  H: the handle's spectra, Hn: the new taps' (same layout; only fading rows are
// read), fading: one byte per tap row.  tw: as k_fir_stream's
template <int LOG2B, bool BANK>
__global__ void __launch_bounds__(stream_threads(LOG2B), LOG2B == 12 ? 2 : 1)
k_fir_stream_fade(const float *__restrict__ in, float *__restrict__ out, const float2 *__restrict__ H, const float2 *__restrict__ Hn,
                  const unsigned char *__restrict__ fading, const float2 *__restrict__ tw, float2 *ring, float *prev, fade_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    constexpr int U = M >= 8 ? 1 : 8 / M;                   // partitions in flight
    constexpr bool ONE_PASS = M <= 4;                       // both sums in one walk of the ring
    __shared__ __align__(16) float2 lds[B];
    __shared__ __align__(16) float2 xkeep[ONE_PASS ? 1 : B];   // two passes: the block's spectrum, then the old output, by owner
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, c = blockIdx.x;
    const float2 *spl = tw + B / 2;
    const float *irow = in + (size_t)c * (size_t)G.in_pitch;      // a flush has no input and never reads it
    float *orow = out + (size_t)c * (size_t)G.out_pitch;
    float *prow = prev + (size_t)c * B;
    float2 *rc = ring + (size_t)c * (size_t)G.R * B;
    const size_t hoff = BANK ? (size_t)c * (size_t)G.P * B : 0;
    const float2 *ho = H + hoff, *hn = Hn + hoff;
    const bool frow = fading[BANK ? c : 0] != 0;            // the same for the whole workgroup
    const float den = (float)((long)G.fade_blocks * B);     // F B <= 2^24: exact

    int pos[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) pos[g] = (tid + g * T) * V;
    const bool first = tid == 0;                            // owner of position 0, the packed bin

    const int jb = G.flush ? (int)blockIdx.y : 0, je = G.flush ? jb + 1 : G.nblk;
    for (int j = jb; j < je; j++) {
        const int cur = (G.head + j) % G.R;
        const int fb = G.fade_done + j;                     // this block's place in the fade
        const bool blend = frow && fb < G.fade_blocks;
        const float2 *hp = frow ? hn : ho;                  // the plain chain's spectra: a fading row past the end is on the new ones
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
        if (!G.flush) {
            float2 *slot = rc + (size_t)cur * B;
#pragma unroll
            for (int g = 0; g < NG; g++) store_bins<V>(slot + pos[g], &x[g * V]);
        }

        // acc = sum_p X_{j-p} h_p, p ascending from a zero accumulator, the p0 term from registers: k_fir_stream's chain
        auto chain = [&](const float2 *hc, float2 *acc, const float2 *x) {
            const float2 *h0 = hc + (size_t)p0 * B;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                float2 h[V];
                load_bins<V>(h0 + pos[g], h);
#pragma unroll
                for (int v = 0; v < V; v++) {
                    acc[g * V + v] = float2{0.f, 0.f};
                    bin_mac(acc[g * V + v], x[g * V + v], h[v], g == 0 && v == 0 && first);
                }
            }
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
            int p = p0 + 1;
#pragma unroll 1
            for (; p + U <= G.P; p += U) {
#pragma unroll
                for (int u = 0; u < U; u++) step(p + u);
            }
#pragma unroll 1
            for (; p < G.P; p++) step(p);
        };
        // both chains in one walk: every ring bin loaded once; each sum is the chain above, term for term
        auto chain2 = [&](float2 *acco, float2 *accn) {
            const float2 *h0o = ho + (size_t)p0 * B, *h0n = hn + (size_t)p0 * B;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                float2 a[V], b[V];
                load_bins<V>(h0o + pos[g], a);
                load_bins<V>(h0n + pos[g], b);
#pragma unroll
                for (int v = 0; v < V; v++) {
                    acco[g * V + v] = float2{0.f, 0.f};
                    accn[g * V + v] = float2{0.f, 0.f};
                    bin_mac(acco[g * V + v], x[g * V + v], a[v], g == 0 && v == 0 && first);
                    bin_mac(accn[g * V + v], x[g * V + v], b[v], g == 0 && v == 0 && first);
                }
            }
            auto step = [&](int pp) {
                int s = cur - pp;
                if (s < 0) s += G.R;
                const float2 *xs = rc + (size_t)s * B, *hso = ho + (size_t)pp * B, *hsn = hn + (size_t)pp * B;
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    float2 xv[V], a[V], b[V];
                    load_bins<V>(xs + pos[g], xv);
                    load_bins<V>(hso + pos[g], a);
                    load_bins<V>(hsn + pos[g], b);
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        bin_mac(acco[g * V + v], xv[v], a[v], g == 0 && v == 0 && first);
                        bin_mac(accn[g * V + v], xv[v], b[v], g == 0 && v == 0 && first);
                    }
                }
            };
            int p = p0 + 1;
#pragma unroll 1
            for (; p + U <= G.P; p += U) {
#pragma unroll
                for (int u = 0; u < U; u++) step(p + u);
            }
#pragma unroll 1
            for (; p < G.P; p++) step(p);
        };
        // inverse split through LDS and the inverse transform: the block's B output samples are lf[B ..) afterwards.  Opens on a
        // barrier: every read of the LDS image before it (the forward split's mirrors, the old output's samples) is done
        auto inverse = [&](const float2 *acc) {
            __syncthreads();
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
        };

        if constexpr (ONE_PASS) {
            if (!blend) {
                float2 acc[M];
                chain(hp, acc, x);
                inverse(acc);
                for (int t = tid; t < B; t += T) {
                    const long n = (long)j * B + t;
                    if (n < G.n_out) __builtin_nontemporal_store(lf[B + t], &orow[n]);
                }
            } else {
                float2 acco[M], accn[M];
                float yo[M];                                // the old filter's samples of this thread: t = tid + i T
                chain2(acco, accn);
                inverse(acco);
#pragma unroll
                for (int i = 0; i < M; i++) yo[i] = lf[B + tid + i * T];
                inverse(accn);
#pragma unroll
                for (int i = 0; i < M; i++) {
                    const int t = tid + i * T;
                    const long n = (long)j * B + t;
                    const float w = __fdiv_rn((float)((long)fb * B + t), den);
                    if (n < G.n_out) __builtin_nontemporal_store(fade_blend(w, yo[i], lf[B + t]), &orow[n]);
                }
            }
        } else {
            // one code site for the chain, walked once or (a fading block) twice.  A thread parks its own bins of the new spectrum
            // in its own slots of xkeep and takes them back itself at the head of a pass -- no barrier of their own -- and in the
            // second pass leaves the old filter's samples there instead: the product loop carries neither
#pragma unroll
            for (int g = 0; g < NG; g++) store_bins<V>(xkeep + pos[g], &x[g * V]);
            const int npass = blend ? 2 : 1;
#pragma unroll 1
            for (int pass = 0; pass < npass; pass++) {
                float2 xp[M], acc[M];
#pragma unroll
                for (int g = 0; g < NG; g++) load_bins<V>(xkeep + pos[g], &xp[g * V]);
                if (pass) {
#pragma unroll
                    for (int m = 0; m < M; m++) xkeep[pos[m / V] + m % V].x = lf[B + tid + m * T];
                }
                chain(blend ? (pass ? hn : ho) : hp, acc, xp);
                inverse(acc);
            }
            if (!blend) {
                for (int t = tid; t < B; t += T) {
                    const long n = (long)j * B + t;
                    if (n < G.n_out) __builtin_nontemporal_store(lf[B + t], &orow[n]);
                }
            } else {
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const int t = tid + m * T;
                    const long n = (long)j * B + t;
                    const float w = __fdiv_rn((float)((long)fb * B + t), den);
                    const float yo = xkeep[pos[m / V] + m % V].x;
                    if (n < G.n_out) __builtin_nontemporal_store(fade_blend(w, yo, lf[B + t]), &orow[n]);
                }
            }
        }
    }
    if (!G.flush) {
        // the frame's last block is the next call's previous block
        for (int t = tid; t < B; t += T) prow[t] = irow[(size_t)(G.nblk - 1) * B + t];
    }
}

template <int LOG2B>
int fade_launch(bool bank, const float *in, float *out, const float2 *H, const float2 *Hn, const unsigned char *fading,
                const float2 *tw, float2 *ring, float *prev, const fade_geom &G, int channels, hipStream_t st)
{
    const dim3 grid((unsigned)channels, G.flush ? (unsigned)G.nblk : 1u), wg(stream_threads(LOG2B));
    if (bank) hipLaunchKernelGGL((k_fir_stream_fade<LOG2B, true>), grid, wg, 0, st, in, out, H, Hn, fading, tw, ring, prev, G);
    else hipLaunchKernelGGL((k_fir_stream_fade<LOG2B, false>), grid, wg, 0, st, in, out, H, Hn, fading, tw, ring, prev, G);
    LLZ_LAUNCH_CHECK("k_fir_stream_fade");
    return LLZ_OK;
}

} // namespace

// llzs_fir_stream_f32's launch with a fade in flight.  hspec_new: the new taps' spectra, laid out as hspec (only the rows marked
// in `fading` are read); fading: one byte per tap row on the device (bank: channels rows, else one); block j of this launch is
// block fade_done + j of the fade's fade_blocks.
extern "C" int llzs_fir_stream_fade_f32(int block, const float *hspec, int bank, const float *tw, float *ring, float *prev,
                                        const float *in, float *out, int channels, int nblk, int flush, long n_out, long in_pitch,
                                        long out_pitch, int P, int R, int head, const float *hspec_new,
                                        const unsigned char *fading, int fade_done, int fade_blocks, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    fade_geom G = {{P, R, head, nblk, flush ? 1 : 0, n_out, in_pitch, out_pitch}, {fade_done, fade_blocks}};
    if (!stream_launch_ok(G, ok, block, channels, hspec && hspec_new && fading && tw && ring && prev && out, in) ||
        !fade_pos_ok(G)) {
        llzs_set_error("fir_stream_fade_f32: bad arguments (block=%d channels=%d nblk=%d P=%d R=%d head=%d n_out=%ld fade %d of %d)",
                       block, channels, nblk, P, R, head, n_out, fade_done, fade_blocks);
        return LLZ_ERR_ARG;
    }
    const float2 *H = reinterpret_cast<const float2 *>(hspec), *Hn = reinterpret_cast<const float2 *>(hspec_new);
    const float2 *W = reinterpret_cast<const float2 *>(tw);
    float2 *rg = reinterpret_cast<float2 *>(ring);
    hipStream_t st = as_stream(stream);
    const bool bk = bank != 0;
#define FADE(L) fade_launch<L>(bk, in, out, H, Hn, fading, W, rg, prev, G, channels, st)
    STREAM_DISPATCH(log2b, FADE)
#undef FADE
}
