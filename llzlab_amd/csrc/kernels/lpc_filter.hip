// lpc_filter.hip -- the two filters that apply llz_lpc_mc's output (include/llz_lpc.h part 3): the prediction-error filter
// A_f(z) (k_lpc_residual) and the all-pole filter 1 / A_f(z) (k_lpc_synth), both with a coefficient set per (channel, frame).
// x, e, y: planar [channels][frames * frame_len] float32; acof: [channels][frames][p + 1] float32, acof[..][0] never read.
//
// k_lpc_residual: e[t] = fmaf chain over k = p .. 1 from acc = x[t], float32 (the order is the contract).  A workgroup takes
// 1024 consecutive outputs of one channel, placed so that every lane's four outputs are one 16-byte store whatever the
// alignment of the row; the input span with its p-sample halo (from the row, or from the handle's history in front of the
// call) is read with 16-byte loads on the input row's own 16-byte grid and staged in LDS, as are the coefficient sets of the
// frames the tile touches (a tile is not tied to a frame: at frame_len 160 a tile of one frame would leave most of a
// workgroup idle).  A lane slides a register window over the span: per four lags one 16-byte LDS read of samples and one each
// of the coefficients of the two frames its four outputs can lie in, chosen per output by a select.
//
// k_lpc_synth<ORD>: y[t] = e[t] - sum a_f[k] y[t-k] in double, oldest term first, rounded multiply then rounded subtract, a
// lane per channel and NO split in time: iir_df1.hip starts later segments from zero state `warm` samples early, which
// needs one impulse response to decay over -- with a coefficient set per frame there is none, so a channel is one lane
// from its first sample to its last.  The delay line is in registers with static indices: H[i] = y(t0 - 1 - i) in front of
// a block, the block's own outputs in N[], and one shift of H per block of 16 (not per sample).  The current frame's
// coefficients are registers too (converted to double once per frame, which is exact), reloaded at each frame's start.  A
// frame is walked in blocks of 16 samples per lane (four 16-byte loads, the next block's issued ahead, four 16-byte stores)
// and its last frame_len % 16 samples one by one, so that a block never holds two coefficient sets.
#include "common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) u4 { f32x4 v; };     // a 16-byte access at a 4-byte aligned address

constexpr int ORD_MAX = 64;             // LLZ_LEVINSON_ORDER_MAX: the stride of both states in the handle
constexpr int RES_TILE = 1024, RES_THREADS = 256;

__device__ __forceinline__ int elem_phase(const void *row) { return (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3); }

// LDS: xs[HP + RES_TILE + 8] then as[nf_max][cs].  HP = p rounded up to 4, cs = HP + 4.  With s0t the row index of the tile's
// first output, sample s sits at xs[s - s0t + HP + 4] and a_f[k] at as[(f - f_first) * cs + k + 3]: a lane's window
// x[s0 - 4m ..] and the four coefficients a[4m - 3 .. 4m] are then 16-byte aligned in LDS.
__global__ void __launch_bounds__(RES_THREADS)
k_lpc_residual(const float *__restrict__ x, const float *__restrict__ acof, float *__restrict__ e,
               const float *__restrict__ hist_in, float *__restrict__ hist_out, int frames, int frame_len, int p, int tiles)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int c = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)c * (unsigned)tiles);
    const long T = (long)frames * frame_len;
    const float *xrow = x + (size_t)c * T;
    float *erow = e + (size_t)c * T;
    const int HP = (p + 3) & ~3, cs = HP + 4;
    float *xs = lds, *as = lds + HP + RES_TILE + 8;

    if (tile == 0 && tid < p) hist_out[(size_t)c * ORD_MAX + tid] = xrow[T - 1 - tid];    // x(-1 - i) of the next call
    const long s0t = (long)RES_TILE * tile - elem_phase(erow);          // outputs s0t + 4 tid + j: 16-byte stores
    if (s0t >= T) return;                                                // (a row's phase can leave the last tile empty)

    // ---- stage the samples s0t - HP - mx .. on the input row's 16-byte grid
    const int mx = (int)(((long)(reinterpret_cast<uintptr_t>(xrow) >> 2) + s0t - HP) & 3);
    const long base = s0t - HP - mx;
    const int chunks = (mx + HP + RES_TILE + 3) >> 2;
    for (int ch = tid; ch < chunks; ch += RES_THREADS) {
        const long s = base + 4 * ch;
        f32x4 v;
        if (s >= 0 && s + 3 < T) {
            v = *reinterpret_cast<const f32x4 *>(xrow + s);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const long sj = s + j;
                v[j] = sj >= T ? 0.0f : sj >= 0 ? xrow[sj] : sj >= -p ? hist_in[(size_t)c * ORD_MAX + (-1 - sj)] : 0.0f;
            }
        }
        float *dst = xs + (4 * ch - mx + 4);
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
    }
    // ---- and the coefficient sets of the frames f_first .. f_last the tile's outputs lie in
    const long s_lo = s0t > 0 ? s0t : 0, s_hi = s0t + RES_TILE - 1 < T - 1 ? s0t + RES_TILE - 1 : T - 1;
    const int f_first = (int)(s_lo / frame_len), f_last = (int)(s_hi / frame_len);
    const int P1 = p + 1, ncoef = (f_last - f_first + 1) * P1;
    const float *arow = acof + ((size_t)c * frames + f_first) * P1;
    for (int i = tid; i < ncoef; i += RES_THREADS) {
        const int f = i / P1, k = i - f * P1;
        as[f * cs + k + 3] = arow[i];
    }
    __syncthreads();

    const long s0 = s0t + 4 * tid;
    if (s0 + 3 < 0 || s0 >= T) return;
    const int q0 = 4 * tid + HP + 4;
    f32x4 acc = *reinterpret_cast<const f32x4 *>(xs + q0);
    if (frame_len < 4) {
        // (p <= 2) four outputs can lie in more than two frames: each with its own frame
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long sj = s0 + j;
            if (sj < 0 || sj >= T) continue;
            const float *a = as + ((int)(sj / frame_len) - f_first) * cs + 3;
            for (int k = p; k >= 1; k--) acc[j] = fmaf(a[k], xs[q0 + j - k], acc[j]);
        }
    } else {
        // outputs j < split lie in frame f_lo, the others in the next one
        const int s0c = (int)(s0 > 0 ? s0 : 0);
        const int f_lo = s0c / frame_len;
        const long split = (long)(f_lo + 1) * frame_len - s0;
        const int f_hi = f_lo + 1 <= f_last ? f_lo + 1 : f_last;
        const float *alo = as + (f_lo - f_first) * cs + 3, *ahi = as + (f_hi - f_first) * cs + 3;
        const bool lo0 = split > 0, lo1 = split > 1, lo2 = split > 2, lo3 = split > 3;
        const int M = p >> 2;
        for (int k = p; k > 4 * M; k--) {                               // the p % 4 oldest lags, one at a time
            const float l = alo[k], h = ahi[k];
            acc[0] = fmaf(lo0 ? l : h, xs[q0 + 0 - k], acc[0]);
            acc[1] = fmaf(lo1 ? l : h, xs[q0 + 1 - k], acc[1]);
            acc[2] = fmaf(lo2 ? l : h, xs[q0 + 2 - k], acc[2]);
            acc[3] = fmaf(lo3 ? l : h, xs[q0 + 3 - k], acc[3]);
        }
        if (M > 0) {
            f32x4 A = *reinterpret_cast<const f32x4 *>(xs + q0 - 4 * M);         // A[i] = x[s0 - 4m + i], B[i] = x[s0 - 4m + 4 + i]
            for (int m = M; m >= 1; m--) {
                const f32x4 B = *reinterpret_cast<const f32x4 *>(xs + q0 - 4 * m + 4);
                const f32x4 L = *reinterpret_cast<const f32x4 *>(alo + 4 * m - 3);   // L[i] = a[4m - 3 + i]
                const f32x4 Hc = *reinterpret_cast<const f32x4 *>(ahi + 4 * m - 3);
                // lag 4m
                acc[0] = fmaf(lo0 ? L[3] : Hc[3], A[0], acc[0]);
                acc[1] = fmaf(lo1 ? L[3] : Hc[3], A[1], acc[1]);
                acc[2] = fmaf(lo2 ? L[3] : Hc[3], A[2], acc[2]);
                acc[3] = fmaf(lo3 ? L[3] : Hc[3], A[3], acc[3]);
                // lag 4m - 1
                acc[0] = fmaf(lo0 ? L[2] : Hc[2], A[1], acc[0]);
                acc[1] = fmaf(lo1 ? L[2] : Hc[2], A[2], acc[1]);
                acc[2] = fmaf(lo2 ? L[2] : Hc[2], A[3], acc[2]);
                acc[3] = fmaf(lo3 ? L[2] : Hc[2], B[0], acc[3]);
                // lag 4m - 2
                acc[0] = fmaf(lo0 ? L[1] : Hc[1], A[2], acc[0]);
                acc[1] = fmaf(lo1 ? L[1] : Hc[1], A[3], acc[1]);
                acc[2] = fmaf(lo2 ? L[1] : Hc[1], B[0], acc[2]);
                acc[3] = fmaf(lo3 ? L[1] : Hc[1], B[1], acc[3]);
                // lag 4m - 3
                acc[0] = fmaf(lo0 ? L[0] : Hc[0], A[3], acc[0]);
                acc[1] = fmaf(lo1 ? L[0] : Hc[0], B[0], acc[1]);
                acc[2] = fmaf(lo2 ? L[0] : Hc[0], B[1], acc[2]);
                acc[3] = fmaf(lo3 ? L[0] : Hc[0], B[2], acc[3]);
                A = B;
            }
        }
    }
    if (s0 >= 0 && s0 + 3 < T) {
        *reinterpret_cast<f32x4 *>(erow + s0) = acc;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (s0 + j >= 0 && s0 + j < T) erow[s0 + j] = acc[j];
    }
}

// NB samples from `in` to `out`, all of one frame (coefficients a[1 .. p])
template <int ORD, int NB>
__device__ __forceinline__ void synth_block(const float (&in)[NB], float (&out)[NB], double (&H)[ORD], const double (&a)[ORD + 1],
                                            int p)
{
#pragma clang fp contract(off)
    double N[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) {
        double acc = (double)in[j];
#pragma unroll
        for (int k = ORD; k >= 1; k--) {
            const double h = k <= j ? N[k <= j ? j - k : 0] : H[k > j ? k - j - 1 : 0];
            const double prod = a[k] * h;
            const double next = acc - prod;
            // a lag above p is skipped, not multiplied by zero: the difference is dropped by a select (a branch per term
            // splits the block into a thousand pieces and the register allocator gives up).  The kernel for ORD serves
            // ORD / 2 < p <= ORD (ORD 8: 0 <= p), so only the upper half can be above p
            acc = (ORD > 8 && 2 * k <= ORD) || k <= p ? next : acc;
        }
        N[j] = acc;
        out[j] = (float)acc;
    }
#pragma unroll
    for (int i = ORD - 1; i >= 0; i--) H[i] = i < NB ? N[NB - 1 - i] : H[i >= NB ? i - NB : 0];
}

template <int ORD>
__global__ void __launch_bounds__(64)
k_lpc_synth(const float *__restrict__ e, const float *__restrict__ acof, float *__restrict__ y, double *__restrict__ state,
            int channels, int frames, int frame_len, int p)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= channels) return;
    const long T = (long)frames * frame_len;
    const float *er = e + (size_t)c * T;
    float *yr = y + (size_t)c * T;
    const float *anext = acof + (size_t)c * frames * (p + 1);
    double *st = state + (size_t)c * ORD_MAX;
    double H[ORD];
    double a[ORD + 1];
#pragma unroll
    for (int k = 0; k < ORD; k++) {
        const double s = st[k];                                          // (lags p .. 63 of the state are never written: zeros)
        H[k] = k < p ? s : 0.0;
        a[k + 1] = 0.0;
    }
    a[0] = 1.0;
    constexpr int BLK = 16;
    long t = 0;
    for (int f = 0; f < frames; f++) {
        if (p > 0) {                                                     // the frame's coefficients 1 .. p
#pragma unroll
            for (int k = 1; k <= ORD; k++) a[k] = (double)anext[k < p ? k : p];
            anext += p + 1;
        }
        const long fend = t + frame_len;
        // whole blocks of the frame, the next one's loads issued in front of this one's steps; then single samples up to the
        // frame's end (a block never holds two coefficient sets)
        if (t + BLK <= fend) {
            float cur[BLK], nxt[BLK], o[BLK];
#pragma unroll
            for (int q = 0; q < BLK / 4; q++) {
                const f32x4 v = reinterpret_cast<const u4 *>(er + t + 4 * q)->v;
                cur[4 * q] = v[0]; cur[4 * q + 1] = v[1]; cur[4 * q + 2] = v[2]; cur[4 * q + 3] = v[3];
            }
            for (; t + BLK <= fend; t += BLK) {
                const bool more = t + 2 * BLK <= fend;
                if (more) {
#pragma unroll
                    for (int q = 0; q < BLK / 4; q++) {
                        const f32x4 v = reinterpret_cast<const u4 *>(er + t + BLK + 4 * q)->v;
                        nxt[4 * q] = v[0]; nxt[4 * q + 1] = v[1]; nxt[4 * q + 2] = v[2]; nxt[4 * q + 3] = v[3];
                    }
                }
                synth_block<ORD, BLK>(cur, o, H, a, p);
#pragma unroll
                for (int q = 0; q < BLK / 4; q++) {
                    f32x4 v;
                    v[0] = o[4 * q]; v[1] = o[4 * q + 1]; v[2] = o[4 * q + 2]; v[3] = o[4 * q + 3];
                    reinterpret_cast<u4 *>(yr + t + 4 * q)->v = v;
                }
                if (more) {
#pragma unroll
                    for (int q = 0; q < BLK; q++) cur[q] = nxt[q];
                }
            }
        }
        for (; t < fend; t++) {
            float i1[1] = {er[t]}, o1[1];
            synth_block<ORD, 1>(i1, o1, H, a, p);
            yr[t] = o1[0];
        }
    }
#pragma unroll
    for (int k = 0; k < ORD; k++)
        if (k < p) st[k] = H[k];
}

} // namespace

// the frames a tile of RES_TILE consecutive outputs can lie in
static int res_frames_per_tile(int frames, int frame_len)
{
    const long nf = (RES_TILE - 1) / frame_len + 2;
    return nf < frames ? (int)nf : frames;
}

// hist_in / hist_out: [channels][64] floats, [c][i] = x(-1 - i) in front of / behind this call, i < p; two different buffers
// (a row's first tile reads the one while it writes the other)
extern "C" int llzs_lpc_residual_f32(const float *x, const float *acof, float *e, const float *hist_in, float *hist_out,
                                     int channels, int frames, int frame_len, int p, void *stream)
{
    if (!x || !acof || !e || !hist_in || !hist_out || hist_in == hist_out || channels < 1 || frames < 1 || p < 0 || p > ORD_MAX ||
        frame_len <= p || (long)frames * frame_len > 0x7fffffffL || (long)channels * frames > 0x7fffffffL) {
        llzs_set_error("lpc_residual_f32: bad arguments (channels=%d frames=%d frame_len=%d p=%d)", channels, frames, frame_len, p);
        return LLZ_ERR_ARG;
    }
    const long T = (long)frames * frame_len;
    const long tiles = (T + 3 + RES_TILE - 1) / RES_TILE;
    if (tiles * channels > 0x7fffffffL) {
        llzs_set_error("lpc_residual_f32: %ld tiles of %d samples x %d channels exceed one launch", tiles, RES_TILE, channels);
        return LLZ_ERR_RANGE;
    }
    const int HP = (p + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)HP + RES_TILE + 8 + (size_t)res_frames_per_tile(frames, frame_len) * (HP + 4));
    hipLaunchKernelGGL(k_lpc_residual, dim3((unsigned)(tiles * channels)), dim3(RES_THREADS), lds, as_stream(stream), x, acof, e,
                       hist_in, hist_out, frames, frame_len, p, (int)tiles);
    LLZ_LAUNCH_CHECK("k_lpc_residual");
    return LLZ_OK;
}

// state: [channels][64] doubles, [c][i] = y(-1 - i), i < p, read at the start and written at the end by the channel's lane
extern "C" int llzs_lpc_synth_f32(const float *e, const float *acof, float *y, double *state, int channels, int frames,
                                  int frame_len, int p, void *stream)
{
    if (!e || !acof || !y || !state || channels < 1 || frames < 1 || p < 0 || p > ORD_MAX || frame_len <= p ||
        (long)frames * frame_len > 0x7fffffffL || (long)channels * frames > 0x7fffffffL) {
        llzs_set_error("lpc_synth_f32: bad arguments (channels=%d frames=%d frame_len=%d p=%d)", channels, frames, frame_len, p);
        return LLZ_ERR_ARG;
    }
    const dim3 grid((unsigned)((channels + 63) / 64)), block(64);
#define LLZ_SYNTH(ORD) hipLaunchKernelGGL(k_lpc_synth<ORD>, grid, block, 0, as_stream(stream), e, acof, y, state, channels, \
                                          frames, frame_len, p)
    if (p <= 8) LLZ_SYNTH(8);
    else if (p <= 16) LLZ_SYNTH(16);
    else if (p <= 32) LLZ_SYNTH(32);
    else LLZ_SYNTH(64);
#undef LLZ_SYNTH
    LLZ_LAUNCH_CHECK("k_lpc_synth");
    return LLZ_OK;
}
