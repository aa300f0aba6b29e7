// lpc.hip -- linear prediction of many frames (the autocorrelation method; reference libllzfilter/llz_lpc.c:69-95 per frame).
//
//  k_lpc_fused_f32<NL>  p <= 8 NL <= 32: a wave takes a block of B frames, computes their autocorrelations one after another
//                       with the register form of k_autocorr_reg_f32 (acf_reg.hpp: the same bits) and parks each frame's p + 1
//                       sums in its private LDS; then lane j runs the Levinson-Durbin recursion of frame j of the block.
//  k_levinson_f64<PMAX> the recursion alone, from r in global memory (read into the same LDS rows): 33 <= p <= 64, and the
//                       cross-check of the fused form (llz_hip_tune("lpc_split", 1)).
//  k_window_f32         x * win in float32 for the split path.
//
// The recursion is llz_levinson's (llz_levinson.c:29-67) in double with contraction off and IEEE division, from (double) r, and
// every output is rounded once to float32.  The coefficients live in registers (the loops are unrolled to PMAX with a uniform
// guard at p, so every index is a constant); a[j] and a[i-j] are updated as a pair, which gives the reference's values without its copy.
// acof and r leave through the same LDS rows so that their stores are coalesced.
#include "common.hpp"
#include "acf_reg.hpp"

namespace {

constexpr int LPC_WAVES = 4;
constexpr long LPC_MAX_BLOCKS = 256L * 4;      // persistent grid, as llzs_autocorr_mc_f32

// the wave's own LDS accesses are done before other lanes of the wave touch the same words (no workgroup barrier: the rows
// are private to the wave)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// nf consecutive rows of `len` floats, row i at rs + i * S, to / from dst[0 .. nf * len) with consecutive lanes on
// consecutive words
__device__ __forceinline__ void rows_to_global(const float *rs, int S, int nf, int len, float *__restrict__ dst, int lane)
{
    for (int e = lane; e < nf * len; e += 64) {
        const int fr = e / len;
        dst[e] = rs[fr * S + (e - fr * len)];
    }
}

// Lane j < nf: the recursion of frame f0 + j from row j of rs (stride S >= PMAX + 1, r[0 .. p]); writes acof [nf][p+1] (through
// the LDS rows), kcof [nf][p], err, gain of the block (each may be NULL but acof).  Row j is overwritten.
template <int PMAX>
__device__ __forceinline__ void lpc_block_solve(float *rs, int S, long f0, int nf, int p, int n, int lane,
                                                float *__restrict__ acof, float *__restrict__ kcof,
                                                float *__restrict__ err, float *__restrict__ gain)
{
#pragma clang fp contract(off)
    const bool mine = lane < nf;
    float *rl = rs + (mine ? lane : 0) * S;
    double a[PMAX + 1];
#pragma unroll
    for (int i = 0; i <= PMAX; i++) a[i] = i == 0 ? 1.0 : 0.0;
    // kcof straight from the recursion (lane j's p values are contiguous, a block's are one range): keeping them for an LDS
    // pass would cost PMAX registers and occupancy
    float *kl = kcof && mine ? kcof + (f0 + lane) * p : nullptr;
    const double r0 = mine ? (double)rl[0] : 0.0;
    double e = 0.0;
    if (r0 == 0.0 && kl) {
        for (int i = 0; i < p; i++) kl[i] = 0.f;
    }
    if (r0 != 0.0) {                                     // a silent frame keeps a = [1, 0, ...], k = 0, e = 0
        e = r0;
#pragma unroll
        for (int i = 1; i <= PMAX; i++) {
            if (i <= p) {                                // p is uniform: a scalar branch
                double acc = (double)rl[i];
#pragma unroll
                for (int j = 1; j < i; j++) acc = acc + a[j] * (double)rl[i - j];
                const double k = -acc / e;
                if (kl) kl[i - 1] = (float)k;
#pragma unroll
                for (int j = 1; 2 * j < i; j++) {
                    const double aj = a[j], am = a[i - j];
                    a[j] = aj + k * am;
                    a[i - j] = am + k * aj;
                }
                if (i % 2 == 0) a[i / 2] = a[i / 2] + k * a[i / 2];
                a[i] = k;
                e = e * (1 - k * k);
            }
        }
    }
    if (mine) {
        if (err) err[f0 + lane] = (float)(e / (double)n);
        if (gain) gain[f0 + lane] = e > 0 ? (float)(r0 / e) : 0.f;
    }
    wave_lds_sync();                                     // every lane is done reading r
    if (mine) {
#pragma unroll
        for (int k = 0; k <= PMAX; k++)
            if (k <= p) rl[k] = (float)a[k];
    }
    wave_lds_sync();
    rows_to_global(rs, S, nf, p + 1, acof + f0 * (p + 1), lane);
}

template <int NL, bool WIN>
__global__ void __launch_bounds__(64 * LPC_WAVES)
k_lpc_fused_f32(const float *__restrict__ x, const float *__restrict__ win, float *__restrict__ acof, float *__restrict__ kcof,
                float *__restrict__ err, float *__restrict__ gain, float *__restrict__ r, int frames, int n, int p, int B)
{
    extern __shared__ float lds_lpc[];
    constexpr int S = 8 * NL + 1;                       // odd: lane j's row starts in bank (j S) mod 64, all different
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *rs = lds_lpc + wave * B * S;
    const long nblk = ((long)frames + B - 1) / B, waves_total = (long)gridDim.x * LPC_WAVES;
    for (long blk = (long)blockIdx.x * LPC_WAVES + wave; blk < nblk; blk += waves_total) {
        const long f0 = blk * B;
        const int nf = (int)(frames - f0 < B ? frames - f0 : B);
        wave_lds_sync();                                 // the previous block's rows have been read
        for (int i = 0; i < nf; i++) {
            float acc[S];
            acf_reg_frame<NL, WIN>(x + (size_t)(f0 + i) * n, win, n, lane, acc);
            int k;
            const float v = wave_sums(acc, lane, &k);
            if (k <= p) rs[i * S + k] = v;
        }
        wave_lds_sync();
        if (r) rows_to_global(rs, S, nf, p + 1, r + f0 * (p + 1), lane);
        lpc_block_solve<8 * NL>(rs, S, f0, nf, p, n, lane, acof, kcof, err, gain);
    }
}

template <int PMAX>
__global__ void __launch_bounds__(64 * LPC_WAVES)
k_levinson_f64(const float *__restrict__ r, float *__restrict__ acof, float *__restrict__ kcof, float *__restrict__ err,
               float *__restrict__ gain, int frames, int n, int p, int B)
{
    extern __shared__ float lds_lpc[];
    constexpr int S = PMAX + 1 + (PMAX % 2);            // odd
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *rs = lds_lpc + wave * B * S;
    const long nblk = ((long)frames + B - 1) / B, waves_total = (long)gridDim.x * LPC_WAVES;
    for (long blk = (long)blockIdx.x * LPC_WAVES + wave; blk < nblk; blk += waves_total) {
        const long f0 = blk * B;
        const int nf = (int)(frames - f0 < B ? frames - f0 : B);
        const float *src = r + f0 * (p + 1);
        wave_lds_sync();
        for (int e = lane; e < nf * (p + 1); e += 64) {
            const int fr = e / (p + 1);
            rs[fr * S + (e - fr * (p + 1))] = src[e];
        }
        wave_lds_sync();
        lpc_block_solve<PMAX>(rs, S, f0, nf, p, n, lane, acof, kcof, err, gain);
    }
}

__global__ void __launch_bounds__(256)
k_window_f32(const float *__restrict__ x, const float *__restrict__ win, float *__restrict__ y, int n, long total)
{
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const float v = x[e] * win[e % n];
        y[e] = v;
    }
}

// frames per wave block: whole 64-lane blocks when they fill every wave of the grid, else smaller ones (the recursion then
// leaves lanes idle, the correlation does not leave waves idle)
int lpc_block_frames(int frames, int cap)
{
    int B = cap;
    while (B > 16 && ((long)frames + B - 1) / B < LPC_MAX_BLOCKS * LPC_WAVES) B /= 2;
    return B;
}

long lpc_grid(int frames, int B)
{
    const long nblk = ((long)frames + B - 1) / B;
    const long g = (nblk + LPC_WAVES - 1) / LPC_WAVES;
    return g < LPC_MAX_BLOCKS ? g : LPC_MAX_BLOCKS;
}

} // namespace

extern "C" int llzs_lpc_fused_f32(const float *x, const float *win, float *acof, float *kcof, float *err, float *gain, float *r,
                                  int frames, int n, int p, void *stream)
{
    if (!x || !acof || frames < 1 || n < 1 || p < 0 || p > 32 || p >= n) {
        llzs_set_error("lpc_fused_f32: bad arguments (frames=%d n=%d p=%d; p < n, p <= 32)", frames, n, p);
        return LLZ_ERR_ARG;
    }
    const int nl = p <= 8 ? 1 : (p + 7) / 8;             // the lag groups llzs_autocorr_mc_f32 takes for this p
    const int B = lpc_block_frames(frames, 64);
    const dim3 grid((unsigned)lpc_grid(frames, B)), block(64 * LPC_WAVES);
    const size_t lds = sizeof(float) * LPC_WAVES * B * (8 * nl + 1);
#define LLZ_LPC_FUSED(NLV)                                                                                                  \
    do {                                                                                                                    \
        if (win)                                                                                                            \
            hipLaunchKernelGGL((k_lpc_fused_f32<NLV, true>), grid, block, lds, as_stream(stream), x, win, acof, kcof, err,  \
                               gain, r, frames, n, p, B);                                                                   \
        else                                                                                                                \
            hipLaunchKernelGGL((k_lpc_fused_f32<NLV, false>), grid, block, lds, as_stream(stream), x, win, acof, kcof, err, \
                               gain, r, frames, n, p, B);                                                                   \
    } while (0)
    if (nl == 1) LLZ_LPC_FUSED(1);
    else if (nl == 2) LLZ_LPC_FUSED(2);
    else if (nl == 3) LLZ_LPC_FUSED(3);
    else LLZ_LPC_FUSED(4);
#undef LLZ_LPC_FUSED
    LLZ_LAUNCH_CHECK("k_lpc_fused_f32");
    return LLZ_OK;
}

extern "C" int llzs_levinson_f32(const float *r, float *acof, float *kcof, float *err, float *gain, int frames, int n, int p,
                                 void *stream)
{
    if (!r || !acof || frames < 1 || n < 1 || p < 0 || p > 64) {
        llzs_set_error("levinson_f32: bad arguments (frames=%d n=%d p=%d; p <= 64)", frames, n, p);
        return LLZ_ERR_ARG;
    }
    const int pmax = p <= 32 ? (p <= 8 ? 8 : (p + 7) / 8 * 8) : (p <= 48 ? 48 : 64);
    const int B = lpc_block_frames(frames, pmax > 32 ? 32 : 64);    // LDS of a workgroup stays under 64 KiB
    const dim3 grid((unsigned)lpc_grid(frames, B)), block(64 * LPC_WAVES);
    const size_t lds = sizeof(float) * LPC_WAVES * B * (pmax + 1);  // every pmax is even: S = pmax + 1
#define LLZ_LEV(PM)                                                                                                      \
    hipLaunchKernelGGL(k_levinson_f64<PM>, grid, block, lds, as_stream(stream), r, acof, kcof, err, gain, frames, n, p, B)
    switch (pmax) {
    case 8: LLZ_LEV(8); break;
    case 16: LLZ_LEV(16); break;
    case 24: LLZ_LEV(24); break;
    case 32: LLZ_LEV(32); break;
    case 48: LLZ_LEV(48); break;
    default: LLZ_LEV(64); break;
    }
#undef LLZ_LEV
    LLZ_LAUNCH_CHECK("k_levinson_f64");
    return LLZ_OK;
}

extern "C" int llzs_window_f32(const float *x, const float *win, float *y, int frames, int n, void *stream)
{
    if (!x || !win || !y || frames < 1 || n < 1) {
        llzs_set_error("window_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const long total = (long)frames * n;
    long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_window_f32, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, win, y, n, total);
    LLZ_LAUNCH_CHECK("k_window_f32");
    return LLZ_OK;
}
