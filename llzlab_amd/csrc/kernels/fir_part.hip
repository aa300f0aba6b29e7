// fir_part.hip -- K4d: uniformly partitioned overlap-save, the batch FIR for long filters (LLZ_FIR_ALGO_PARTITIONED, 1..131073
// taps, one tap set for every channel), and K4e: the same three kernels with a tap set per channel (the partitioned bank).
//
// The taps are cut into P = ceil(flt_len / B) partitions of B = N / 2 taps, H_p = DFT_N(partition p, zero-padded) / N.  With
// X_k = DFT_N of samples [(k - 1) B, (k + 1) B) of a channel's frame (negative indices: the history, before it zeros),
// output block k is the last B samples of IDFT_N(Y_k), Y_k = sum_{p < P} X_{k-p} H_p.  Forward e^{-j} unscaled, 1 / N in H,
// as in fir_ols.hip.  The cost per sample grows with flt_len / B, not flt_len.
//
// Choices, with their reasons:
//   * Two real sequences per complex transform: block k rides with block k + Kh OF THE SAME CHANNEL (Kh = ceil(K / 2), K the
//     blocks of the call), Z_q = X_q + j X_{q+Kh} for q = -(P-1) .. Kh-1.  The taps are real, so IDFT(sum_p Z_{q-p} H_p) holds
//     output block q in its real and block q + Kh in its imaginary part: the spectra are never separated, and a channel's
//     output depends on that channel's samples alone, to the bit.  Two channels in one transform would halve the work for
//     short frames but leak the rounding noise of a loud channel into a quiet one.  The price: Kh + P - 1 forward transforms
//     per channel instead of (K + P - 1) / 2, which only shows when the frame is much shorter than the filter.
//   * Transform: N points of a workgroup in LDS (8 N bytes: 8 .. 64 KB), decimation in frequency forward (natural in,
//     bit-reversed out), decimation in time back (bit-reversed in, natural out), two radix-2 stages per LDS round trip.  The
//     product is bin-wise, so nothing is ever bit-reversed: the host stores H_p in the forward transform's output order.  The
//     register transforms of fft32.hpp serve 1024 points per half-wave; composing them to 8192 costs the 8192-point rung its
//     pairs of waves and fixed overlaps, and the transforms are not where this form spends its time (the product's scratch
//     traffic is), so one LDS form serves all four sizes.  The passes live in part_fft.hpp, shared with fir_stream.hip (K4f).
//   * Three kernels, not fused: forward (samples -> Z in scratch), product (Z, H -> Y in scratch), inverse (Y -> samples).  A
//     fused product + inverse would have to hold a run of N-point accumulators per workgroup (64 KB each at 8192 points: a
//     run of 2), and without a run every output block reads P spectra.  The product kernel's thread owns ONE bin of a run of
//     PART_RUN consecutive blocks: PART_RUN accumulators and a sliding window of PART_RUN Z values in registers, one Z and one
//     H load per partition step.  Scratch reads per run: PART_RUN + P - 1 spectra instead of PART_RUN x P; H comes from L2
//     (P x 8 N bytes, 2.1 MB at the top size).  The window slides by register renaming (the partition loop is unrolled by
//     PART_RUN).  Every sum runs over p ascending in one thread: no atomics, the same call gives the same bits.
//   * Channels go in passes of as many as the scratch holds ((2 Kh + P - 1) x 8 N bytes per channel), in sequence on the
//     stream.  All index arithmetic over channels x blocks x N is size_t / long.
//   * The bank (K4e): only the product reads the taps, so only the product kernel has a second instance, BANK = true, which
//     reads channel c's spectra at H + c P N.  A template parameter, not a pitch argument: the shared instance keeps the
//     instructions it had.  In passes H advances with in, out and hist.  Measured 2 .. 8 % behind the shared form (H is no
//     longer one table in L2); reading Z with nontemporal loads to spare H's cache lines was 6 .. 17 % behind and dropped
//     (DESIGN.md K4e).
#include "common.hpp"
#include "part_fft.hpp"

namespace {

constexpr int PART_THREADS = 256;
constexpr int PART_RUN = 16;

struct part_geom {
    int n, keep;                // samples per channel of this call, flt_len - 1
    int N, B, P;                // transform points, block, partitions
    int Kh, S;                  // complex output blocks per channel, complex spectra per channel = Kh + P - 1
    long in_pitch, out_pitch;
};

// sample t of concat(zeros, history, frame, zeros) of one channel; t = 0 is the frame's first sample
__device__ __forceinline__ float part_sample(const float *__restrict__ row, const float *__restrict__ hrow, long t, int n, int keep)
{
    if (t >= n) return 0.f;
    if (t >= 0) return row[t];
    if (t >= -(long)keep) return hrow[keep + t];
    return 0.f;
}

// K4d-1: workgroup (s, c) -> spectrum s of channel c: Z_q = DFT_N(block q + j block q + Kh), q = s - (P - 1)
template <int LOG2N>
__global__ void __launch_bounds__(PART_THREADS)
k_fir_part_fwd(const float *__restrict__ in, const float *__restrict__ hist, const float2 *__restrict__ tw,
               float2 *__restrict__ Z, part_geom G)
{
    constexpr int N = 1 << LOG2N;
    extern __shared__ float2 part_lds[];
    const int tid = threadIdx.x, c = blockIdx.y;
    const long s = blockIdx.x, q = s - (G.P - 1);
    const float *row = in + (size_t)c * (size_t)G.in_pitch;
    const float *hrow = hist ? hist + (size_t)c * (size_t)G.keep : nullptr;
    const int keep = hrow ? G.keep : 0;
    const long t0 = (q - 1) * G.B, t1 = t0 + (long)G.Kh * G.B;
    for (int i = tid; i < N; i += PART_THREADS)
        part_lds[i] = float2{part_sample(row, hrow, t0 + i, G.n, keep), part_sample(row, hrow, t1 + i, G.n, keep)};
    part_fft_dif<LOG2N, PART_THREADS>(part_lds, tw, tid);
    float2 *dst = Z + ((size_t)c * (size_t)G.S + (size_t)s) * N;
    for (int i = tid; i < N; i += PART_THREADS) dst[i] = part_lds[i];
}

// K4d-2: workgroup (run, bin tile, c): Y_q[bin] = sum_{p < P} Z_{q-p}[bin] H_p[bin] for the PART_RUN blocks q0 .. of the run.
// BANK: H is [channels][P][N], channel c's own spectra
template <bool BANK>
__global__ void __launch_bounds__(PART_THREADS)
k_fir_part_mac(const float2 *__restrict__ Z, const float2 *__restrict__ H, float2 *__restrict__ Y, part_geom G, int tiles)
{
    const int c = blockIdx.y;
    const long run = blockIdx.x / tiles;
    const int bin = (int)(blockIdx.x - run * tiles) * PART_THREADS + threadIdx.x;
    const long q0 = run * PART_RUN;
    const size_t N = (size_t)G.N;
    const float2 *zc = Z + (size_t)c * (size_t)G.S * N + bin;          // spectrum s = q + P - 1 at zc[s * N]
    const float2 *h = BANK ? H + (size_t)c * (size_t)G.P * N + bin : H + bin;
    float2 acc[PART_RUN], w[PART_RUN];
#pragma unroll
    for (int r = 0; r < PART_RUN; r++) {
        acc[r] = float2{0.f, 0.f};
        w[r] = q0 + r < G.Kh ? zc[(size_t)(q0 + r + G.P - 1) * N] : float2{0.f, 0.f};
    }
    for (int p0 = 0; p0 < G.P; p0 += PART_RUN) {
#pragma unroll
        for (int u = 0; u < PART_RUN; u++) {
            const int p = p0 + u;
            if (p < G.P) {                                              // uniform over the grid
                // block q0 + r meets Z_{q0 + r - p}: slot (r - u) mod PART_RUN of the window
                const float2 hp = h[(size_t)p * N];
#pragma unroll
                for (int r = 0; r < PART_RUN; r++) {
                    const float2 z = w[(r - u + PART_RUN) % PART_RUN];
                    acc[r].x = __builtin_fmaf(-z.y, hp.y, __builtin_fmaf(z.x, hp.x, acc[r].x));
                    acc[r].y = __builtin_fmaf(z.y, hp.x, __builtin_fmaf(z.x, hp.y, acc[r].y));
                }
                // the window slides: Z_{q0 - (p + 1)} takes the slot of the block that leaves
                if (p + 1 < G.P) w[(PART_RUN - 1 - u) % PART_RUN] = zc[(size_t)(q0 + G.P - 2 - p) * N];
            }
        }
    }
    float2 *yc = Y + (size_t)c * (size_t)G.Kh * N + bin;
#pragma unroll
    for (int r = 0; r < PART_RUN; r++)
        if (q0 + r < G.Kh) yc[(size_t)(q0 + r) * N] = acc[r];
}

// K4d-3: workgroup (q, c): IDFT_N(Y_q), its last B samples: the real parts are block q, the imaginary parts block q + Kh
template <int LOG2N>
__global__ void __launch_bounds__(PART_THREADS)
k_fir_part_inv(const float2 *__restrict__ Y, const float2 *__restrict__ tw, float *__restrict__ out, part_geom G)
{
    constexpr int N = 1 << LOG2N, B = N / 2;
    extern __shared__ float2 part_lds[];
    const int tid = threadIdx.x, c = blockIdx.y;
    const long q = blockIdx.x;
    const float2 *src = Y + ((size_t)c * (size_t)G.Kh + (size_t)q) * N;
    for (int i = tid; i < N; i += PART_THREADS) part_lds[i] = src[i];
    part_fft_dit_inv<LOG2N, PART_THREADS>(part_lds, tw, tid);
    float *orow = out + (size_t)c * (size_t)G.out_pitch;
    const long ta = q * B, tb = (q + G.Kh) * B;
    for (int i = tid; i < B; i += PART_THREADS) {
        const float2 v = part_lds[B + i];
        if (ta + i < G.n) __builtin_nontemporal_store(v.x, &orow[ta + i]);
        if (tb + i < G.n) __builtin_nontemporal_store(v.y, &orow[tb + i]);
    }
}

int part_log2(int nfft)
{
    return nfft == 1024 ? 10 : nfft == 2048 ? 11 : nfft == 4096 ? 12 : nfft == 8192 ? 13 : 0;
}

part_geom part_geom_of(int nfft, int flt_len, int n, long in_pitch, long out_pitch)
{
    part_geom G;
    G.n = n;
    G.keep = flt_len - 1;
    G.N = nfft;
    G.B = nfft / 2;
    G.P = (flt_len + G.B - 1) / G.B;
    const int K = (n + G.B - 1) / G.B;
    G.Kh = (K + 1) / 2;
    G.S = G.Kh + G.P - 1;
    G.in_pitch = in_pitch;
    G.out_pitch = out_pitch;
    return G;
}

} // namespace

// scratch bytes one channel of a call of n samples needs: Kh + P - 1 spectra Z and Kh spectra Y
static size_t part_need(int nfft, int flt_len, int n)
{
    const part_geom G = part_geom_of(nfft, flt_len, n, n, n);
    return ((size_t)G.S + (size_t)G.Kh) * (size_t)nfft * sizeof(float2);
}

extern "C" int llzs_fir_part_need(int nfft, int flt_len, int n, size_t *bytes)
{
    if (!part_log2(nfft) || flt_len < 1 || n < 1 || !bytes) {
        llzs_set_error("fir_part_need: bad arguments (nfft=%d flt_len=%d n=%d)", nfft, flt_len, n);
        return LLZ_ERR_ARG;
    }
    *bytes = part_need(nfft, flt_len, n);
    return LLZ_OK;
}

// plan[4] = {transform points, partitions, channels per pass, passes}; LLZ_ERR_NOMEM when not one channel fits
extern "C" int llzs_fir_part_plan(int nfft, int flt_len, int n, int channels, size_t scratch_bytes, int plan[4])
{
    if (!part_log2(nfft) || flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS || n < 1 || channels < 1 || !plan) {
        llzs_set_error("fir_part: bad arguments (nfft=%d flt_len=%d n=%d channels=%d)", nfft, flt_len, n, channels);
        return LLZ_ERR_ARG;
    }
    const size_t need = part_need(nfft, flt_len, n);
    const size_t fit = scratch_bytes / need;
    if (fit < 1) {
        llzs_set_error("fir_part: one channel of %d samples at %d taps needs %zu B of scratch, %zu B allowed", n, flt_len, need,
                       scratch_bytes);
        return LLZ_ERR_NOMEM;
    }
    const int per_pass = fit < (size_t)channels ? (int)fit : channels;
    plan[0] = nfft;
    plan[1] = (flt_len + nfft / 2 - 1) / (nfft / 2);
    plan[2] = per_pass;
    plan[3] = (channels + per_pass - 1) / per_pass;
    return LLZ_OK;
}

template <int LOG2N, bool BANK>
static int part_run_pass(const part_geom &G, const float2 *H, const float2 *tw, float2 *Z, float2 *Y, const float *in, float *out,
                         const float *hist, int count, hipStream_t st)
{
    constexpr int N = 1 << LOG2N;
    const size_t lds = sizeof(float2) * N;
    const int tiles = N / PART_THREADS;
    const long runs = (G.Kh + PART_RUN - 1) / PART_RUN;
    hipLaunchKernelGGL(k_fir_part_fwd<LOG2N>, dim3((unsigned)G.S, (unsigned)count), dim3(PART_THREADS), lds, st, in, hist, tw, Z, G);
    LLZ_LAUNCH_CHECK("k_fir_part_fwd");
    hipLaunchKernelGGL(k_fir_part_mac<BANK>, dim3((unsigned)(runs * tiles), (unsigned)count), dim3(PART_THREADS), 0, st, Z, H, Y, G, tiles);
    LLZ_LAUNCH_CHECK("k_fir_part_mac");
    hipLaunchKernelGGL(k_fir_part_inv<LOG2N>, dim3((unsigned)G.Kh, (unsigned)count), dim3(PART_THREADS), lds, st, Y, tw, out, G);
    LLZ_LAUNCH_CHECK("k_fir_part_inv");
    return LLZ_OK;
}

// bank: hpart is [channels][P][nfft] complex, a channel's own spectra; else [P][nfft], one tap set shared by all channels
static int part_launch(int nfft, const float *hpart, bool bank, const float *tw, float *scratch, size_t scratch_bytes,
                       const float *in, float *out, const float *hist, int channels, int n, long in_pitch, long out_pitch,
                       int flt_len, void *stream)
{
    int plan[4];
    if (!hpart || !tw || !scratch || !in || !out || in_pitch < n || out_pitch < n || channels > 65535 || (flt_len > 1 && !hist)) {
        llzs_set_error("fir_part_f32: bad arguments (channels=%d n=%d flt_len=%d)", channels, n, flt_len);
        return LLZ_ERR_ARG;
    }
    int rc = llzs_fir_part_plan(nfft, flt_len, n, channels, scratch_bytes, plan);
    if (rc != LLZ_OK) return rc;
    const part_geom G = part_geom_of(nfft, flt_len, n, in_pitch, out_pitch);
    if ((size_t)G.S * (size_t)(nfft / PART_THREADS) > 0x7fffffffUL) {
        llzs_set_error("fir_part_f32: %d samples per call are more blocks than a grid holds", n);
        return LLZ_ERR_RANGE;
    }
    const size_t h_pitch = bank ? 2 * (size_t)G.P * (size_t)nfft : 0;     // floats from one channel's spectra to the next
    const int per_pass = plan[2];
    float2 *Z = reinterpret_cast<float2 *>(scratch);
    float2 *Y = Z + (size_t)per_pass * (size_t)G.S * (size_t)nfft;
    const float2 *W = reinterpret_cast<const float2 *>(tw);
    hipStream_t st = as_stream(stream);
    for (int c0 = 0; c0 < channels && rc == LLZ_OK; c0 += per_pass) {
        const int count = channels - c0 < per_pass ? channels - c0 : per_pass;
        const float *pin = in + (size_t)c0 * (size_t)in_pitch;
        float *pout = out + (size_t)c0 * (size_t)out_pitch;
        const float *ph = flt_len > 1 ? hist + (size_t)c0 * (size_t)(flt_len - 1) : nullptr;
        // a bank's spectra advance with the channels of the pass
        const float2 *H = reinterpret_cast<const float2 *>(hpart + (size_t)c0 * h_pitch);
        switch (nfft) {
        case 1024: rc = bank ? part_run_pass<10, true>(G, H, W, Z, Y, pin, pout, ph, count, st)
                             : part_run_pass<10, false>(G, H, W, Z, Y, pin, pout, ph, count, st); break;
        case 2048: rc = bank ? part_run_pass<11, true>(G, H, W, Z, Y, pin, pout, ph, count, st)
                             : part_run_pass<11, false>(G, H, W, Z, Y, pin, pout, ph, count, st); break;
        case 4096: rc = bank ? part_run_pass<12, true>(G, H, W, Z, Y, pin, pout, ph, count, st)
                             : part_run_pass<12, false>(G, H, W, Z, Y, pin, pout, ph, count, st); break;
        default: rc = bank ? part_run_pass<13, true>(G, H, W, Z, Y, pin, pout, ph, count, st)
                           : part_run_pass<13, false>(G, H, W, Z, Y, pin, pout, ph, count, st); break;
        }
    }
    return rc;
}

extern "C" int llzs_fir_part_f32(int nfft, const float *hpart, const float *tw, float *scratch, size_t scratch_bytes,
                                 const float *in, float *out, const float *hist, int channels, int n, long in_pitch,
                                 long out_pitch, int flt_len, void *stream)
{
    return part_launch(nfft, hpart, false, tw, scratch, scratch_bytes, in, out, hist, channels, n, in_pitch, out_pitch, flt_len, stream);
}

// the bank: hbank [channels][P][nfft] complex, channel c filtered with its own spectra
extern "C" int llzs_fir_part_bank_f32(int nfft, const float *hbank, const float *tw, float *scratch, size_t scratch_bytes,
                                      const float *in, float *out, const float *hist, int channels, int n, long in_pitch,
                                      long out_pitch, int flt_len, void *stream)
{
    return part_launch(nfft, hbank, true, tw, scratch, scratch_bytes, in, out, hist, channels, n, in_pitch, out_pitch,
                       flt_len, stream);
}
