// fft.hip -- K4/K5 standalone: batched radix-2 complex FFT in LDS for gfx950, three arithmetic flavours that share
// the reference's exact dataflow (reference libllzfilter/llz_fft.c:61-198, llz_fft_fixed.c:61-218):
//
//   forward : DIF butterflies, half-span = N/2 ... 1, twiddle index q * (N / span), w = cos - j sin, no scaling,
//             then the bit-reversal gather to natural order;
//   inverse : bit-reversal gather (float: each element divided by N there), DIT butterflies half-span 1 ... N/2,
//             w = cos + j sin (fixed point: arithmetic >> log2 N once at the very end).
//
//   float   tolerance path (batched float32, the overlap-save building block)
//   double  the reference's own arithmetic, rounded multiply / add in its expression order, no contraction:
//           bit-identical to llz_fft / llz_ifft for the same host-built twiddle table
//   int32   Q15 twiddles, (int64 a * b) >> 15 per product, wrapping adds: bit-identical to llz_fft_fixed
//
// A workgroup holds 2048 points in LDS (one 2048/4096-point transform or several smaller ones); the log2 N radix-2
// stages run as 1-3 passes of up to four stages fused in registers (16 elements per lane), a barrier between passes (fft_core.hpp).
// Twiddle tables come from the host (never recomputed on the device: SURVEY.md H4/H5).
//
// Beside the staged kernel: the float32 register transforms of the square (E^2), 2 x square and 1024-point sizes and the
// Q15 register transform (shared pieces in fft_square.hpp), and the register MDCT built on them.  The fused FFT
// autocorrelation lives in acf_fft.hip, the windowed-FFT analysis / synthesis frames in stft.hip, sizes above 4096 in
// fft_large.hip.
#include <stdlib.h>
#include "fft_square.hpp"

namespace {

// groups: up to four passes, G of pass p in bits [4p, 4p+4) (0 = no pass). tpw transforms per workgroup.
template <typename A, bool INVERSE>
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_radix2(typename A::data_t *__restrict__ data, int count, int size, int log2n,
             const typename A::tw_t *__restrict__ cs /* size cos, then size sin */, int tpw, unsigned groups)
{
    typedef typename A::data_t T;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<T> *s = reinterpret_cast<cpx<T> *>(smem_raw);
    const int tid = threadIdx.x;
    const int tr0 = blockIdx.x * tpw;
    const int ntr = min(tpw, count - tr0);                 // transforms this workgroup really has
    cpx<T> *g = reinterpret_cast<cpx<T> *>(data) + (size_t)tr0 * size;
    const int tstride = fft_tstride(size);
    const int total = ntr << log2n;
    cpx<typename A::tw_t> *tw = reinterpret_cast<cpx<typename A::tw_t> *>(s + (size_t)tpw * tstride);
    fft_load_twiddles(tw, cs, size, tid);

    // load (inverse: through the bit-reversal, float flavour divides by N here: llz_fft.c:187-195)
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2n, i = e & (size - 1);
        if (!INVERSE) {
            s[tr * tstride + fft_phys(i)] = g[e];
        } else {
            cpx<T> v = g[(tr << log2n) + (int)(__brev((unsigned)i) >> (32 - log2n))];
            v.re = A::scale_in(v.re, size, log2n);
            v.im = A::scale_in(v.im, size, log2n);
            s[tr * tstride + fft_phys(i)] = v;
        }
    }
    __syncthreads();

    fft_run<A, INVERSE>(s, ntr, size, log2n, tstride, tw, groups, tid);

    // store (forward: through the bit-reversal gather, llz_fft.c:155-163; fixed inverse: >> log2 N, :212-215)
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2n, i = e & (size - 1);
        if (!INVERSE) {
            g[e] = s[tr * tstride + fft_phys((int)(__brev((unsigned)i) >> (32 - log2n)))];
        } else {
            cpx<T> v = s[tr * tstride + fft_phys(i)];
            v.re = A::scale_out(v.re, log2n);
            v.im = A::scale_out(v.im, log2n);
            g[e] = v;
        }
    }
}


// 1024-point float32 transforms, the overlap-save size: one HALF-WAVE per transform, two in-register 32-point passes and
// one LDS transpose between them (fft32.hpp, the machinery of K4).  Input goes from HBM straight into registers (lane l
// takes x[l + 32 j]: 256-byte runs) and the result straight back (X[l + 32 k2]), so a transform costs ~600 vector
// instructions per lane pair instead of the ~1550 of the staged radix-2 passes, which are bound by instruction issue.
template <bool INV>
__global__ void __launch_bounds__(256)
k_fft1024_f32(float *__restrict__ data, int count, const float *__restrict__ cs /* 1024 cos, then 1024 sin */)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ float2 s_tw[1024];                                  // W_1024^(a*b) = exp(-2 pi j a b / 1024), [a][b]
    __shared__ float bufs[8][OLS_XBUF];
    const int tid = threadIdx.x, hw = tid >> 5, l5 = tid & 31;
    load_tw1024(s_tw, cs, tid);
    __syncthreads();
    const long t = (long)blockIdx.x * 8 + hw;
    if (t >= count) return;
    f32x2 *g = reinterpret_cast<f32x2 *>(data) + t * 1024;
    cf v[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const f32x2 x = __builtin_nontemporal_load(&g[l5 + 32 * j]);
        // the inverse divides by N on the way in, as llz_ifft does (llz_fft.c:187-195); 1/1024 is exact
        v[j] = INV ? cf{x.x * (1.0f / 1024.0f), x.y * (1.0f / 1024.0f)} : cf{x.x, x.y};
    }
    fft32<INV>(v);                                                 // over j: v[q] = Y[k1 = brev5(q)] of column l5
    transpose_twiddle<INV>(v, bufs[hw], s_tw, l5);                 // * W^(k1 * l5), then lane k1 holds row k1
    fft32<INV>(v);                                                 // over the column index: v[q] = X[l5 + 32 brev5(q)]
#pragma unroll
    for (int q = 0; q < 32; q++)
        __builtin_nontemporal_store((f32x2){v[q].x, v[q].y}, &g[l5 + 32 * brev5(q)]);
}

// tw2d: [E][E] float2, entry [k1][l] = exp(-2 pi j k1 l / N); one transform per group of E lanes, 256 / E per workgroup
// E = 64 needs ~300 VGPRs: at least two waves per SIMD are asked for (256 registers, a few spilled), which beats one
// wave with everything in registers: N = 4096 0.248 -> 0.197 ms
template <int E, bool INV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(E == 64 ? 2 : 1)))
k_fft_square_f32(float *__restrict__ data, int count, const float2 *__restrict__ tw2d)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int N = E * E, GROUPS = 256 / E, PITCH = E + 1;
    __shared__ float bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    long t = (long)blockIdx.x * GROUPS + grp;
    if (t >= count) return;                                     // whole groups leave together: no barrier below
    // a whole wave per transform: tell the compiler the base is wave-uniform, so that the 2 x 64 accesses are scalar base +
    // one lane offset + immediates instead of 128 separate 64-bit address pairs (400+ -> ~300 VGPRs; still one wave per
    // SIMD: the 64-element network itself holds ~220, fencing the butterflies in groups did not lower it)
    if (E == 64) t = (long)blockIdx.x * GROUPS + __builtin_amdgcn_readfirstlane(grp);
    f32x2 *g = reinterpret_cast<f32x2 *>(data) + t * N;
    float *buf = bufs[grp];
    cf v[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        const f32x2 x = __builtin_nontemporal_load(&g[lg + E * j]);
        v[j] = INV ? cf{x.x * (1.0f / N), x.y * (1.0f / N)} : cf{x.x, x.y};
    }
    square_core<E, INV>(v, buf, tw2d, lg);                      // v[q] = X[lg + E brevE(q)]
#pragma unroll
    for (int q = 0; q < E; q++)
        __builtin_nontemporal_store((f32x2){v[q].x, v[q].y}, &g[lg + E * brevE<E>(q)]);
}

// N = 2 E^2 (E = 16: 512, E = 32: 2048): one radix-2 step around two E x E transforms held by the same lane group.
//   forward: s = x[n] + x[n + N/2], d = (x[n] - x[n + N/2]) W_N^n;  X[2k] = F(s)[k], X[2k+1] = F(d)[k]  (stored as one
//            16-byte pair per lane);
//   inverse: the mirror image, 1/N folded into the loads.
// tw1: [E][E] float2, entry [j][l] = W_N^(l + E j).
template <int E, bool INV>
__global__ void __launch_bounds__(256)
k_fft_2xsquare_f32(float *__restrict__ data, int count, const float2 *__restrict__ tw2d, const float2 *__restrict__ tw1)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int H = E * E, N = 2 * H, GROUPS = 256 / E, PITCH = E + 1;
    __shared__ float bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    const long t = (long)blockIdx.x * GROUPS + grp;
    if (t >= count) return;
    float *base = data + t * (2 * N);
    f32x2 *g2 = reinterpret_cast<f32x2 *>(base);
    f32x4 *g4 = reinterpret_cast<f32x4 *>(base);
    float *buf = bufs[grp];
    cf s[E], d[E];
    if (!INV) {
#pragma unroll
        for (int j = 0; j < E; j++) {
            const f32x2 a = __builtin_nontemporal_load(&g2[lg + E * j]);
            const f32x2 b = __builtin_nontemporal_load(&g2[lg + E * j + H]);
            const float2 w = tw1[j * E + lg];
            s[j] = cf{a.x + b.x, a.y + b.y};
            d[j] = cmul<false>(cf{a.x - b.x, a.y - b.y}, cf{w.x, w.y});
        }
        square_core<E, false>(s, buf, tw2d, lg);
        square_core<E, false>(d, buf, tw2d, lg);
#pragma unroll
        for (int q = 0; q < E; q++)                                   // bins 2k and 2k+1, k = lg + E brevE(q)
            __builtin_nontemporal_store((f32x4){s[q].x, s[q].y, d[q].x, d[q].y}, &g4[lg + E * brevE<E>(q)]);
    } else {
        constexpr float sc = 1.0f / N;
#pragma unroll
        for (int j = 0; j < E; j++) {
            const f32x4 x = __builtin_nontemporal_load(&g4[lg + E * j]);
            s[j] = cf{x.x * sc, x.y * sc};
            d[j] = cf{x.z * sc, x.w * sc};
        }
        square_core<E, true>(s, buf, tw2d, lg);
        square_core<E, true>(d, buf, tw2d, lg);
#pragma unroll
        for (int q = 0; q < E; q++) {                                 // n = lg + E brevE(q)
            const float2 w = tw1[brevE<E>(q) * E + lg];
            const cf wd = cmul<true>(d[q], cf{w.x, w.y});             // d * conj(W_N^n)
            __builtin_nontemporal_store((f32x2){s[q].x + wd.x, s[q].y + wd.y}, &g2[lg + E * brevE<E>(q)]);
            __builtin_nontemporal_store((f32x2){s[q].x - wd.x, s[q].y - wd.y}, &g2[lg + E * brevE<E>(q) + H]);
        }
    }
}

// Q15 transforms (llz_fft_fixed.c:61-218) of N = E^2 (E = 8, 16, 32, 64) or 2 E^2 (TWO; E = 8, 16, 32) points on a group
// of E lanes, the layout of the float32 register kernels: the radix-2 stages run as two register passes of log2 E stages
// with one LDS transpose between them (TWO: one more stage across the two halves, which the same lanes hold) -- every
// butterfly is the reference's butterfly on the reference's operands (arith_q15::rot: four separately floored
// (int64 * int64) >> 15 products, wrapping adds), so the result is bit-identical; what goes is the index arithmetic and
// the LDS round trips of the staged passes, which is what those were bound by (0.93e12 butterflies/s at every size: ~30
// vector instructions per butterfly, 12 of them arithmetic).
// Forward (DIF), one half: element i = l + E j in register j of lane l; stages with half-span E^2/2 .. E pair registers;
// transpose; lane m then holds i = E m + c and stages E/2 .. 1 pair registers again; the bit-reversed gather becomes the
// store pattern.  Inverse (DIT): the mirror image, >> log2 N at the end (llz_fft_fixed.c:212-215).
template <int E, bool TWO, bool INV>
__global__ void __launch_bounds__(256)
k_fft_reg_q15(int *__restrict__ data, int count, const short *__restrict__ cs /* N cos, then N sin, Q15 */)
{
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    constexpr int H = E * E, N = TWO ? 2 * H : H, GROUPS = 256 / E, PITCH = E + 1, NH = TWO ? 2 : 1;
    constexpr int LOG = E == 8 ? 3 : E == 16 ? 4 : E == 32 ? 5 : 6, LN = 2 * LOG + (TWO ? 1 : 0);
    __shared__ int s_tw[N / 2];                                    // (cos, sin) of 2 pi e / N as a pair of shorts
    __shared__ int bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    for (int e = tid; e < N / 2; e += 256)
        s_tw[e] = (int)((unsigned)(unsigned short)cs[e] | ((unsigned)(unsigned short)cs[N + e] << 16));
    __syncthreads();
    const long t = (long)blockIdx.x * GROUPS + grp;
    if (t >= count) return;                                        // whole groups leave together: no barrier below
    i32x2 *g = reinterpret_cast<i32x2 *>(data) + t * N;
    int *buf = bufs[grp];
    const int lrev = (int)(__brev((unsigned)lg) >> (32 - LOG));
    int vr[NH][E], vi[NH][E];
    auto transpose = [&](int h) {                                  // (lane a, register b) -> (lane b, register a)
#pragma unroll
        for (int b = 0; b < E; b++) buf[b * PITCH + lg] = vr[h][b];
        OLS_WAVE_SYNC();
#pragma unroll
        for (int b = 0; b < E; b++) vr[h][b] = buf[lg * PITCH + b];
        OLS_WAVE_SYNC();
#pragma unroll
        for (int b = 0; b < E; b++) buf[b * PITCH + lg] = vi[h][b];
        OLS_WAVE_SYNC();
#pragma unroll
        for (int b = 0; b < E; b++) vi[h][b] = buf[lg * PITCH + b];
        OLS_WAVE_SYNC();
    };
    // one butterfly of the reference on (ar, ai), (br, bi) with the table entry idx
    auto bfly = [&](int &ar, int &ai, int &br, int &bi, int idx) {
        const int tw = s_tw[idx];
        const short wr = (short)(tw & 0xffff), ws = (short)(tw >> 16);
        const int ur = ar, ui = ai, wre = br, wim = bi;
        if (!INV) {                                                // llz_fft_fixed.c:76-92
            int yr, yi;
            arith_q15::rot(arith_q15::sub(ur, wre), arith_q15::sub(ui, wim), wr, arith_q15::neg(ws), yr, yi);
            ar = arith_q15::add(ur, wre); ai = arith_q15::add(ui, wim);
            br = yr; bi = yi;
        } else {                                                   // llz_fft_fixed.c:122-137
            int dr, di;
            arith_q15::rot(wre, wim, wr, ws, dr, di);
            ar = arith_q15::add(ur, dr); ai = arith_q15::add(ui, di);
            br = arith_q15::sub(ur, dr); bi = arith_q15::sub(ui, di);
        }
    };
    if (!INV) {
#pragma unroll
        for (int h = 0; h < NH; h++)
#pragma unroll
            for (int j = 0; j < E; j++) { const i32x2 x = g[lg + E * j + H * h]; vr[h][j] = x.x; vi[h][j] = x.y; }
        if (TWO) {                                                 // half-span N/2: the two halves of a lane
#pragma unroll
            for (int j = 0; j < E; j++) bfly(vr[0][j], vi[0][j], vr[NH - 1][j], vi[NH - 1][j], lg + E * j);
        }
#pragma unroll
        for (int h = 0; h < NH; h++) {
#pragma unroll
            for (int gq = 0; gq < LOG; gq++) {                     // half-spans E^2/2 .. E: registers hj apart
                const int hj = (E / 2) >> gq;
#pragma unroll
                for (int j = 0; j < E; j++)
                    if (!(j & hj)) bfly(vr[h][j], vi[h][j], vr[h][j + hj], vi[h][j + hj],
                                        (lg + E * (j & (hj - 1))) << (gq + (TWO ? 1 : 0)));
            }
            transpose(h);                                          // lane m: register c = element E m + c of the half
#pragma unroll
            for (int gq = 0; gq < LOG; gq++) {                     // half-spans E/2 .. 1
                const int hc = (E / 2) >> gq;
#pragma unroll
                for (int c = 0; c < E; c++)
                    if (!(c & hc)) bfly(vr[h][c], vi[h][c], vr[h][c + hc], vi[h][c + hc], (c & (hc - 1)) << (LN - LOG + gq));
            }
        }
#pragma unroll
        for (int h = 0; h < NH; h++)                               // llz_fft_fixed.c:170-174: out[brev(i)] = work[i]
#pragma unroll
            for (int c = 0; c < E; c++) g[((brevE<E>(c) * E + lrev) * NH) + h] = (i32x2){vr[h][c], vi[h][c]};
    } else {
#pragma unroll
        for (int h = 0; h < NH; h++)
#pragma unroll
            for (int c = 0; c < E; c++) { const i32x2 x = g[((brevE<E>(c) * E + lrev) * NH) + h]; vr[h][c] = x.x; vi[h][c] = x.y; }
#pragma unroll
        for (int h = 0; h < NH; h++) {
#pragma unroll
            for (int gq = 0; gq < LOG; gq++) {                     // half-spans 1 .. E/2
                const int hc = 1 << gq;
#pragma unroll
                for (int c = 0; c < E; c++)
                    if (!(c & hc)) bfly(vr[h][c], vi[h][c], vr[h][c + hc], vi[h][c + hc], (c & (hc - 1)) << (LN - 1 - gq));
            }
            transpose(h);                                          // lane l: register j = element l + E j of the half
#pragma unroll
            for (int gq = 0; gq < LOG; gq++) {                     // half-spans E .. E^2/2
                const int hj = 1 << gq;
#pragma unroll
                for (int j = 0; j < E; j++)
                    if (!(j & hj)) bfly(vr[h][j], vi[h][j], vr[h][j + hj], vi[h][j + hj],
                                        (lg + E * (j & (hj - 1))) << (LN - 1 - LOG - gq));
            }
        }
        if (TWO) {
#pragma unroll
            for (int j = 0; j < E; j++) bfly(vr[0][j], vi[0][j], vr[NH - 1][j], vi[NH - 1][j], lg + E * j);
        }
#pragma unroll
        for (int h = 0; h < NH; h++)
#pragma unroll
            for (int j = 0; j < E; j++) g[lg + E * j + H * h] = (i32x2){vr[h][j] >> LN, vi[h][j] >> LN};   // :212-215
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// MDCT by the N/4-point FFT (llz_mdct.c:266-353, mdct2 / imdct2) on the register transforms: a group of E lanes per
// frame, N/4 = E^2 (TWO = false: N = 256, 1024, 4096) or 2 E^2 (TWO = true: N = 512, 2048, 8192).  The pre-twiddled
// points are formed straight from HBM into the registers of the lane that transforms them and the post-twiddled results
// go straight back (the rotations 2k / N-1-2k are stride-2 walks up and down the same rows: every line is used whole,
// half by each walk), so the only LDS traffic left is the transpose inside the group.
//   forward: in = x [count][N], out = X [count][N/2];   inverse: in = X [count][N/2], out = x [count][N]
// tc/ts: cos and sin of -2 pi (k + 1/8) / N, k < N/4 (llz_mdct.c:459-462).  Both directions use the FORWARD transform.
// (N = 8192 forward needs 300 VGPRs: two waves per SIMD are forced there, the little that does not fit is spilled --
//  0.94 -> 0.51 ms; the inverse at 344 loses with the same treatment, 0.53 -> 0.57 ms, and keeps one wave)
// FRAMES: the windowed 50 %-overlap frames of llz_asmodel.c:313-463 in batch form (time-domain alias cancellation).  A block
// is (channel c, frame f) of a planar signal [channels][frames F], F = N/2:
//   forward: the transform's input is w[i] xbuf[i], xbuf = the previous frame followed by frame f = the signal from
//            (f-1) F on (frame 0: its first half is the handle's state, the last frame of the previous call); the block of the
//            last frame leaves that frame in state_out;
//   inverse: w[j] y[j] is ADDED to the signal from f F on (llz_asmodel.c:451-452).  Two launches: the even frames store
//            (their ranges [f F, (f+2) F) tile the signal; frame 0 adds the previous call's tail), then the odd frames add to
//            what is there; the last frame's second half is the new tail (state_out).  A sum of two terms does not depend on
//            their order, so the result is that of the reference's sequential overlap-add.
struct mdct_fr {
    const float *win;          // [N]
    const float *state_in;     // [channels][F]
    float *state_out;          // [channels][F], not the same buffer
    int frames;                // frames per channel in this call
    int first, step;           // this launch: frames first, first + step, ...
    int per_channel;           // how many of them (FR = 2: how many runs) per channel
    int run;                   // FR = 2: output segments per group
};

// FR: 0 plain batch, 1 frames (a group per frame), 2 frames, inverse only: a group per RUN of consecutive segments
template <int E, bool TWO, bool INVERSE, int FR>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((E == 32 && TWO && !INVERSE) ? 2 : 1)))
k_mdct_reg_f32(const float *__restrict__ in, float *__restrict__ out, int count, const float *__restrict__ tc,
               const float *__restrict__ ts, const float2 *__restrict__ tw2d, const float2 *__restrict__ tw1,
               float sqrt_cof, mdct_fr fr)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int H = E * E, N4 = TWO ? 2 * H : H, N = 4 * N4, N2 = N / 2, GROUPS = 256 / E, PITCH = E + 1;
    constexpr bool FRAMES = FR != 0, RUN = FR == 2;
    constexpr int VW = TWO ? 4 : 2;                                 // floats per lane and store of the inverse's output
    static_assert(!RUN || INVERSE, "runs of segments are a synthesis form");
    __shared__ float bufs[GROUPS][E * PITCH];
    // FRAMES: the window in LDS, one copy for the workgroup's frames (through the vector memory path it was one load per
    // signal load)
    __shared__ __attribute__((aligned(16))) float s_win[FRAMES ? N : 4];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    if constexpr (FRAMES) {
        for (int i = 4 * tid; i < N; i += 4 * 256) *reinterpret_cast<f32x4 *>(s_win + i) = *reinterpret_cast<const f32x4 *>(fr.win + i);
        __syncthreads();
    }
    const long t = (long)blockIdx.x * GROUPS + grp;
    if (t >= count) return;                                        // whole groups leave together: no barrier below
    const float *x;
    float *y;
    int fc = 0, ff = 0;                                            // FRAMES: channel and frame of this block
    int s0 = 0, f_end = 0;                                         // RUN: segments s0 .. f_end - 1 are this group's
    float tail[RUN ? N2 / E : 1];                                  // RUN: the previous frame's windowed second half, in the
                                                                   // lane's own store layout (VW floats per VW E outputs)
    if constexpr (RUN) {
        fc = (int)(t / fr.per_channel);
        s0 = fr.run * (int)(t - (long)fc * fr.per_channel);
        f_end = min(s0 + fr.run, fr.frames);
        ff = s0 ? s0 - 1 : 0;                                      // the frame in front is transformed again for its tail
        const float *prev = fr.state_in + (size_t)fc * N2;         // segment 0 starts from the previous call's tail
#pragma unroll
        for (int i = 0; i < N2 / E; i += VW) {
#pragma unroll
            for (int c = 0; c < VW; c++) tail[i + c] = s0 ? 0.f : prev[i * E + VW * lg + c];
        }
    }
    for (;;) {                                                      // (one trip unless RUN)
    if constexpr (FRAMES) {
        if constexpr (!RUN) {
            fc = (int)(t / fr.per_channel);
            ff = fr.first + fr.step * (int)(t - (long)fc * fr.per_channel);
        }
        const size_t sig = (size_t)fc * fr.frames * N2;            // the channel's signal: frames * F samples, F = N2
        if (!INVERSE) {
            x = in + sig + (long)(ff - 1) * N2;                    // xbuf[i] = x[i] (frame 0: i < F comes from the state)
            y = out + (sig + (size_t)ff * N2);                     // coefficients [channels][frames][F]
        } else {
            x = in + (sig + (size_t)ff * N2);
            y = out + sig + (size_t)ff * N2;                       // y[j], j < 2F: the signal from f F on
        }
    } else {
        x = in + t * (INVERSE ? N2 : N);
        y = out + t * (INVERSE ? N : N2);
    }
    const float *st_in = FRAMES ? fr.state_in + (size_t)fc * N2 : nullptr;
    float *st_out = FRAMES ? fr.state_out + (size_t)fc * N2 : nullptr;
    const bool last = FRAMES && ff == fr.frames - 1;
    float *buf = bufs[grp];
    // The point k and its mirror N/4-1-k share their rows pairwise: x[2k] goes to k, x[2k+1] to the mirror, and so on.
    // The mirror of (lane lg, register j) is (lane E-1-lg, register E-1-j) -- in bin order (lane E-1-lg, register q^(E-1))
    // -- so every HBM access is an aligned pair (or quad) per lane and the other half changes lanes by one swizzle.
    auto mir = [](float v) {
        return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), ((E - 1) << 10) | 0x1F));   // lane ^ (E-1)
    };
    // rot[i] = -x[i + 3N/4] (i < N/4), x[i - N/4] otherwise (llz_mdct.c:279-283); pairs never straddle N/4
    // (ib = the part of i that does not depend on the lane, a multiple of 2E: which quarter i falls in is decided on it, at
    //  compile time after unrolling -- every access is then base + lane offset + constant)
    const float *xlo = x;                                          // FRAMES forward: where xbuf[0 .. F) lives
    if constexpr (FRAMES && !INVERSE) xlo = ff == 0 ? st_in : x;
    auto rot2 = [&](int ib, int lane2) {
        const bool neg = ib < N4;
        const int idx = (neg ? ib + 3 * N4 : ib - N4) + lane2;
        const bool hi_half = neg || ib >= 3 * N4;                  // idx >= N/2
        f32x2 v;
        if constexpr (FRAMES && !INVERSE) {
            v = *reinterpret_cast<const f32x2 *>((hi_half ? x : xlo) + idx);
            if (hi_half && last) *reinterpret_cast<f32x2 *>(st_out + idx - N2) = v;       // the next call's previous frame
            v *= *reinterpret_cast<const f32x2 *>(s_win + idx);
        } else {
            v = *reinterpret_cast<const f32x2 *>(x + idx);
        }
        return neg ? -v : v;
    };
    // z[k] = 0.5 (re + j im) (c + j s), (c, s) = cos, sin of -2 pi (k + 1/8) / N
    auto pre = [&](int k, float re, float im) {
        const float c = tc[k], sn = ts[k];
        return cf{0.5f * (re * c - im * sn), 0.5f * (re * sn + im * c)};
    };
    cf s[E], d[E];                                                 // d: the odd-bin half of TWO (unused otherwise)
#pragma unroll
    for (int j = 0; j < E / 2; j++) {
        const int jm = E - 1 - j;
        // square: points k = lg + E j and lg + E jm.  TWO: a-points n = lg + E j (registers of s) and b-points n + H (d);
        // the mirror of an a-point is a b-point and vice versa.
        const int ka = lg + E * j, kb = lg + E * jm;
        if (!INVERSE) {
            // own: r0 = rot[2k], r3 = rot[N/2+2k];  from the mirror: r2 = rot[2k+1] (= rot[N/2-1-2k']), r1 = rot[N/2+2k+1]
            if (!TWO) {
                const f32x2 Aa = rot2(2 * E * j, 2 * lg), Ba = rot2(N2 + 2 * E * j, 2 * lg), Ab = rot2(2 * E * jm, 2 * lg), Bb = rot2(N2 + 2 * E * jm, 2 * lg);
                const float r2a = mir(Ab.y), r1a = mir(Bb.y), r2b = mir(Aa.y), r1b = mir(Ba.y);
                s[j] = pre(ka, Aa.x - r1a, r2a - Ba.x);
                s[jm] = pre(kb, Ab.x - r1b, r2b - Bb.x);
            } else {
                const f32x2 Aa = rot2(2 * E * j, 2 * lg), Ba = rot2(N2 + 2 * E * j, 2 * lg), Ab = rot2(2 * E * jm, 2 * lg), Bb = rot2(N2 + 2 * E * jm, 2 * lg);
                const f32x2 Ca = rot2(2 * E * j + 2 * H, 2 * lg), Da = rot2(N2 + 2 * E * j + 2 * H, 2 * lg);
                const f32x2 Cb = rot2(2 * E * jm + 2 * H, 2 * lg), Db = rot2(N2 + 2 * E * jm + 2 * H, 2 * lg);
                // a-point ka <- mirror lane's b-point kb + H (its register jm = our j's partner): C/D of index b
                const cf a0 = pre(ka, Aa.x - mir(Db.y), mir(Cb.y) - Ba.x);
                const cf b0 = pre(ka + H, Ca.x - mir(Bb.y), mir(Ab.y) - Da.x);
                const cf a1 = pre(kb, Ab.x - mir(Da.y), mir(Ca.y) - Bb.x);
                const cf b1 = pre(kb + H, Cb.x - mir(Ba.y), mir(Aa.y) - Db.x);
                const float2 w0 = tw1[j * E + lg], w1 = tw1[jm * E + lg];
                s[j] = cadd(a0, b0); d[j] = cmul<false>(csub(a0, b0), cf{w0.x, w0.y});
                s[jm] = cadd(a1, b1); d[jm] = cmul<false>(csub(a1, b1), cf{w1.x, w1.y});
            }
        } else {
            // re = X[2k] (own), im = X[N/2-1-2k] = X[2k'+1] of the mirror (llz_mdct.c:322-324)
            if (!TWO) {
                const f32x2 Pa = *reinterpret_cast<const f32x2 *>(x + 2 * ka), Pb = *reinterpret_cast<const f32x2 *>(x + 2 * kb);
                s[j] = pre(ka, Pa.x, mir(Pb.y));
                s[jm] = pre(kb, Pb.x, mir(Pa.y));
            } else {
                const f32x2 Pa = *reinterpret_cast<const f32x2 *>(x + 2 * ka), Pb = *reinterpret_cast<const f32x2 *>(x + 2 * kb);
                const f32x2 Qa = *reinterpret_cast<const f32x2 *>(x + 2 * (ka + H)), Qb = *reinterpret_cast<const f32x2 *>(x + 2 * (kb + H));
                const cf a0 = pre(ka, Pa.x, mir(Qb.y)), b0 = pre(ka + H, Qa.x, mir(Pb.y));
                const cf a1 = pre(kb, Pb.x, mir(Qa.y)), b1 = pre(kb + H, Qb.x, mir(Pa.y));
                const float2 w0 = tw1[j * E + lg], w1 = tw1[jm * E + lg];
                s[j] = cadd(a0, b0); d[j] = cmul<false>(csub(a0, b0), cf{w0.x, w0.y});
                s[jm] = cadd(a1, b1); d[jm] = cmul<false>(csub(a1, b1), cf{w1.x, w1.y});
            }
        }
    }
    square_core<E, false>(s, buf, tw2d, lg);                       // square: s[q] = Z[lg + E brevE(q)]
    if constexpr (TWO) square_core<E, false>(d, buf, tw2d, lg);    // TWO: s[q] = Z[2 kq], d[q] = Z[2 kq + 1], kq = lg + E brevE(q)
    // post-twiddle: (c + j s) v
    auto post = [&](int k, cf v) {
        const float c = tc[k], sn = ts[k];
        return cf{v.x * c - v.y * sn, v.x * sn + v.y * c};
    };
    // rot[ri], rot[ri+1] = (v0, v1) -> x (llz_mdct.c:331-352): x[i] = rot[N/4 + i] cof (i < 3N/4), -rot[i - 3N/4] cof else
    // FRAMES: windowed, then stored / added into the signal or left as the new overlap-add tail (see mdct_fr)
    // (jb / rb = the lane-independent part of the index, a multiple of 2E: which half / quarter it falls in is decided on it
    //  at compile time, as in rot2)
    float *ylo = y;                                                 // FRAMES inverse: second half of the last frame -> tail
    auto put = [&](int jb, int lane_off, auto v) {
        typedef decltype(v) vec;
        const int j = jb + lane_off;
        if constexpr (RUN) {
            // first halves are finished with the tail of the frame before; second halves become the tail.  (The caller puts
            // j < N/2 before j + N/2: they share the tail's slot.)
            constexpr int W = sizeof(vec) / sizeof(float);
            v *= *reinterpret_cast<const vec *>(s_win + j);
            const int slot = (jb & (N2 - 1)) / E;                    // = (jb / (W E)) W: a constant after unrolling
            if (jb >= N2) {
                if (last) *reinterpret_cast<vec *>(st_out + j - N2) = v;
#pragma unroll
                for (int c = 0; c < W; c++) tail[slot + c] = v[c];
            } else if (ff >= s0) {
#pragma unroll
                for (int c = 0; c < W; c++) v[c] += tail[slot + c];
                *reinterpret_cast<vec *>(y + j) = v;
            }
            return;
        } else if constexpr (FRAMES && INVERSE) {
            v *= *reinterpret_cast<const vec *>(s_win + j);
            if (jb >= N2) {
                if (last) {
                    *reinterpret_cast<vec *>(st_out + j - N2) = v;
                    return;
                }
                if (fr.first) v += *reinterpret_cast<const vec *>(y + j);                // odd frames: add to the even frames' stores
            } else {
                if (fr.first) v += *reinterpret_cast<const vec *>(y + j);
                else if (ff == 0) v += *reinterpret_cast<const vec *>(st_in + j);         // the previous call's tail
            }
        }
        *reinterpret_cast<vec *>(ylo + j) = v;
    };
    auto unrot2 = [&](int rb, int lane_off, float v0, float v1) {
        if (rb >= N4) put(rb - N4, lane_off, (f32x2){v0 * sqrt_cof, v1 * sqrt_cof});
        else put(rb + 3 * N4, lane_off, (f32x2){-v0 * sqrt_cof, -v1 * sqrt_cof});
    };
    auto unrot4 = [&](int rb, int lane_off, float v0, float v1, float v2, float v3) {
        if (rb >= N4) put(rb - N4, lane_off, (f32x4){v0, v1, v2, v3} * sqrt_cof);
        else put(rb + 3 * N4, lane_off, (f32x4){v0, v1, v2, v3} * -sqrt_cof);
    };
    // rot[b ...] and rot[N/2 + b ...] land half a frame apart: RUN needs the one in the first half put first
    auto both2 = [&](int b, float a0, float a1, float c0, float c1) {
        if (RUN && b < N4) { unrot2(N2 + b, 2 * lg, c0, c1); unrot2(b, 2 * lg, a0, a1); }
        else { unrot2(b, 2 * lg, a0, a1); unrot2(N2 + b, 2 * lg, c0, c1); }
    };
    auto both4 = [&](int b, f32x4 a, f32x4 c) {
        if (RUN && b < N4) { unrot4(N2 + b, 4 * lg, c.x, c.y, c.z, c.w); unrot4(b, 4 * lg, a.x, a.y, a.z, a.w); }
        else { unrot4(b, 4 * lg, a.x, a.y, a.z, a.w); unrot4(N2 + b, 4 * lg, c.x, c.y, c.z, c.w); }
    };
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int qm = q ^ (E - 1);
        if (q > qm) continue;                                      // pairs (q, qm): bins kq and (on the mirror lane) N4-1-kq
        const int kq = lg + E * brevE<E>(q), km = lg + E * brevE<E>(qm);
        if (!INVERSE) {
            // X[2b] = 2 Re', X[N/2-1-2b] = -2 Im' (llz_mdct.c:296-301); X[2b+1] is the -2 Im' of the mirror bin
            if (!TWO) {
                const cf pa = post(kq, s[q]), pb = post(km, s[qm]);
                const float oa = mir(-2.f * pb.y), ob = mir(-2.f * pa.y);
                *reinterpret_cast<f32x2 *>(y + 2 * kq) = (f32x2){2.f * pa.x, oa};
                *reinterpret_cast<f32x2 *>(y + 2 * km) = (f32x2){2.f * pb.x, ob};
            } else {
                const cf sa = post(2 * kq, s[q]), da = post(2 * kq + 1, d[q]), sb = post(2 * km, s[qm]), db = post(2 * km + 1, d[qm]);
                // the mirror of an even bin is an odd bin of the mirror lane's partner register, and vice versa
                const float e0 = mir(-2.f * db.y), e1 = mir(-2.f * sb.y), f0 = mir(-2.f * da.y), f1 = mir(-2.f * sa.y);
                *reinterpret_cast<f32x4 *>(y + 4 * kq) = (f32x4){2.f * sa.x, e0, 2.f * da.x, e1};
                *reinterpret_cast<f32x4 *>(y + 4 * km) = (f32x4){2.f * sb.x, f0, 2.f * db.x, f1};
            }
        } else {
            // rot[2b] = re', rot[N/2+2b] = im', rot[2b+1] = -im' of the mirror bin, rot[N/2+2b+1] = -re' of the mirror bin
            const float g = 8.f * sqrt_cof;
            if (!TWO) {
                const cf pa = post(kq, s[q]), pb = post(km, s[qm]);
                const float ia = mir(pb.y), ra = mir(pb.x), ib = mir(pa.y), rb = mir(pa.x);
                const int bq = 2 * E * brevE<E>(q), bm = 2 * E * brevE<E>(qm);    // constants after unrolling
                both2(bq, g * pa.x, -g * ia, g * pa.y, -g * ra);
                both2(bm, g * pb.x, -g * ib, g * pb.y, -g * rb);
            } else {
                const cf sa = post(2 * kq, s[q]), da = post(2 * kq + 1, d[q]), sb = post(2 * km, s[qm]), db = post(2 * km + 1, d[qm]);
                const float dbi = mir(db.y), dbr = mir(db.x), sbi = mir(sb.y), sbr = mir(sb.x);
                const float dai = mir(da.y), dar = mir(da.x), sai = mir(sa.y), sar = mir(sa.x);
                const int bq = 4 * E * brevE<E>(q), bm = 4 * E * brevE<E>(qm);
                both4(bq, (f32x4){g * sa.x, -g * dbi, g * da.x, -g * sbi}, (f32x4){g * sa.y, -g * dbr, g * da.y, -g * sbr});
                both4(bm, (f32x4){g * sb.x, -g * dai, g * db.x, -g * sai}, (f32x4){g * sb.y, -g * dar, g * db.y, -g * sar});
            }
        }
    }
    if constexpr (!RUN) break;
    else if (++ff >= f_end) break;
    }
}

template <typename A>
int launch_fft(typename A::data_t *data, int count, int size, const typename A::tw_t *cs, int inverse,
               void *stream, const char *name)
{
    int log2n = 0;
    while ((1 << log2n) < size) log2n++;
    if (!data || !cs || count < 1 || size < 2 || size > 4096 || (1 << log2n) != size) {
        llzs_set_error("%s: size %d must be a power of two in 2..4096 (count %d)", name, size, count);
        return LLZ_ERR_ARG;
    }
    // 2048 points per workgroup pass (256 lanes x 8): several small transforms share a workgroup
    const fft_plan pl = fft_make_plan<A>(size, count);
    if (pl.lds >= 64 * 1024) {
        LLZ_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fft_radix2<A, true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
        LLZ_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fft_radix2<A, false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    }
    fft_pick(inverse != 0, [&](auto inv) {
        hipLaunchKernelGGL((k_fft_radix2<A, inv()>), dim3((unsigned)pl.blocks), dim3(FFT_THREADS), pl.lds, as_stream(stream),
                           data, count, size, log2n, cs, pl.tpw, fft_groups(log2n));
    });
    LLZ_LAUNCH_CHECK(name);
    return LLZ_OK;
}

// the Q15 register transform of size E^2 (2 E^2 with TWO)
template <int E, bool TWO>
int launch_fft_reg_q15(int *data, int count, const short *cs, int inverse, void *stream)
{
    const unsigned blocks = (unsigned)((count + (256 / E) - 1) / (256 / E));
    fft_pick(inverse != 0, [&](auto inv) {
        hipLaunchKernelGGL((k_fft_reg_q15<E, TWO, inv()>), dim3(blocks), dim3(256), 0, as_stream(stream), data, count, cs);
    });
    LLZ_LAUNCH_CHECK("k_fft_reg_q15");
    return LLZ_OK;
}

} // namespace

// tables of fft_derived_tables in this file: kind 1 the square sizes, 2 the 2 x square sizes, 3 the MDCT's
extern "C" int llzs_fft_f32(float *data, int count, int size, const float *cs, int inverse, void *stream)
{
    if ((size == 64 || size == 256 || size == 4096) && data && cs && count >= 1 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        const int E = size == 64 ? 8 : size == 256 ? 16 : 64;
        const float2 *tw2d = nullptr;
        const int rc = fft_derived_tables(1, size, E, 1, false, cs, stream, "square twiddle table", &tw2d, nullptr);
        if (rc != LLZ_OK) return rc;
        const unsigned blocks = (unsigned)((count + (256 / E) - 1) / (256 / E));
        fft_pick_e<8, 16, 64>(E, [&](auto e) {
            fft_pick(inverse != 0, [&](auto inv) {
                hipLaunchKernelGGL((k_fft_square_f32<e(), inv()>), dim3(blocks), dim3(256), 0, as_stream(stream), data, count,
                                   tw2d);
            });
        });
        LLZ_LAUNCH_CHECK("k_fft_square_f32");
        return LLZ_OK;
    }
    if ((size == 128 || size == 512 || size == 2048) && data && cs && count >= 1 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        const int E = size == 128 ? 8 : size == 512 ? 16 : 32;
        const float2 *tw2d = nullptr, *tw1 = nullptr;
        const int rc = fft_derived_tables(2, size, E, 2, true, cs, stream, "2 x square twiddle tables", &tw2d, &tw1);
        if (rc != LLZ_OK) return rc;
        const unsigned blocks = (unsigned)((count + (256 / E) - 1) / (256 / E));
        fft_pick_e<8, 16, 32>(E, [&](auto e) {
            fft_pick(inverse != 0, [&](auto inv) {
                hipLaunchKernelGGL((k_fft_2xsquare_f32<e(), inv()>), dim3(blocks), dim3(256), 0, as_stream(stream), data,
                                   count, tw2d, tw1);
            });
        });
        LLZ_LAUNCH_CHECK("k_fft_2xsquare_f32");
        return LLZ_OK;
    }
    if (size == 1024 && data && cs && count >= 1 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        const unsigned blocks = (unsigned)((count + 7) / 8);
        fft_pick(inverse != 0, [&](auto inv) {
            hipLaunchKernelGGL(k_fft1024_f32<inv()>, dim3(blocks), dim3(256), 0, as_stream(stream), data, count, cs);
        });
        LLZ_LAUNCH_CHECK("k_fft1024_f32");
        return LLZ_OK;
    }
    return launch_fft<arith_f32>(data, count, size, cs, inverse, stream, "k_fft_radix2<f32>");
}

// MDCT frames on the register transforms (see k_mdct_reg_f32).  N in {256, 512, 1024, 2048, 4096, 8192}; cs: the FFT
// table of size N/4 the twiddle tables are derived from once per device and size.  Returns LLZ_ERR_RANGE for other N.
static int mdct_reg_launch(const float *in, float *out, int count, int N, const float *tc, const float *ts,
                           const float *cs, int inverse, void *stream, const mdct_fr *frp)
{
    int E = 0, two = 0;
    switch (N) {
    case 256: E = 8; break;  case 1024: E = 16; break; case 4096: E = 32; break;
    case 512: E = 8; two = 1; break; case 2048: E = 16; two = 1; break; case 8192: E = 32; two = 1; break;
    default: return LLZ_ERR_RANGE;
    }
    if (!in || !out || !tc || !ts || !cs || count < 1) {
        llzs_set_error("mdct4_reg_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const float2 *tw2d = nullptr, *tw1 = nullptr;
    const int rc = fft_derived_tables(3, 2 * E + two, E, two ? 2 : 1, two != 0, cs, stream, "mdct twiddle tables", &tw2d, &tw1);
    if (rc != LLZ_OK) return rc;
    const unsigned blocks = (unsigned)((count + (256 / E) - 1) / (256 / E));
    const float sqrt_cof = (float)(1.0 / sqrt((double)N));
    const mdct_fr fr = frp ? *frp : mdct_fr{};
    fft_pick_e<8, 16, 32>(E, [&](auto e) {
        fft_pick(two != 0, [&](auto tt) {
            fft_pick(inverse != 0, [&](auto ii) {
                constexpr int EE = e();
                constexpr bool TT = tt(), II = ii();
                // a group per run of segments where the tail fits the registers (see llzs_mdct4_frames_f32), else per frame
                constexpr int FR_RUN = (II && (EE == 8 || (EE == 16 && !TT))) ? 2 : 1;
                auto launch = [&](auto frc) {
                    hipLaunchKernelGGL((k_mdct_reg_f32<EE, TT, II, frc()>), dim3(blocks), dim3(256), 0, as_stream(stream), in,
                                       out, count, tc, ts, tw2d, tw1, sqrt_cof, fr);
                };
                if (frp && frp->run > 0) launch(std::integral_constant<int, FR_RUN>{});
                else if (frp) launch(std::integral_constant<int, 1>{});
                else launch(std::integral_constant<int, 0>{});
            });
        });
    });
    LLZ_LAUNCH_CHECK("k_mdct_reg_f32");
    return LLZ_OK;
}

extern "C" int llzs_mdct4_reg_f32(const float *in, float *out, int count, int N, const float *tc, const float *ts,
                                  const float *cs, int inverse, void *stream)
{
    return mdct_reg_launch(in, out, count, N, tc, ts, cs, inverse, stream, nullptr);
}

// Windowed 50 %-overlap MDCT frames in batch (k_mdct_reg_f32<..., FRAMES>): analysis x [channels][frames F] -> X
// [channels][frames][F], synthesis the other way with overlap-add; F = N/2, win [N], state_in / state_out [channels][F]
// (analysis: the previous frame; synthesis: the overlap-add tail), two different buffers.
extern "C" int llzs_mdct4_frames_f32(const float *in, float *out, int channels, int frames, int N, const float *tc,
                                     const float *ts, const float *cs, const float *win, const float *state_in,
                                     float *state_out, int inverse, void *stream)
{
    if (!win || !state_in || !state_out || state_in == state_out || channels < 1 || frames < 1) {
        llzs_set_error("mdct4_frames_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    mdct_fr fr;
    fr.win = win; fr.state_in = state_in; fr.state_out = state_out; fr.frames = frames; fr.run = 0;
    if (!inverse) {
        fr.first = 0; fr.step = 1; fr.per_channel = frames;
        return mdct_reg_launch(in, out, channels * frames, N, tc, ts, cs, 0, stream, &fr);
    }
    // A group per run of consecutive segments (frame lengths up to 512: the tail lives in registers; at 1024 the kernel needs
    // all 256 VGPRs and loses to the two launches, 1.03 against 0.92 ms): every output is written
    // once, finished; the frame in front of a run is transformed a second time for its tail, so runs are as long as the
    // machine stays filled with (about 64 K groups), at most 16.  Short problems keep the two launches below.
    int run = llzs_tune(LLZS_TUNE_MDCT_RUN);
    if (run < 0) {
        const long all = (long)channels * frames;
        run = all >= 4 * 65536 ? (int)(all / 65536 > 16 ? 16 : all / 65536) : 0;
    }
    if (run > 0 && N <= 1024) {
        fr.first = 0; fr.step = 1; fr.run = run; fr.per_channel = (frames + run - 1) / run;
        return mdct_reg_launch(in, out, channels * fr.per_channel, N, tc, ts, cs, 1, stream, &fr);
    }
    fr.first = 0; fr.step = 2; fr.per_channel = (frames + 1) / 2;
    int rc = mdct_reg_launch(in, out, channels * fr.per_channel, N, tc, ts, cs, 1, stream, &fr);
    if (rc == LLZ_OK && frames > 1) {
        fr.first = 1; fr.per_channel = frames / 2;
        rc = mdct_reg_launch(in, out, channels * fr.per_channel, N, tc, ts, cs, 1, stream, &fr);
    }
    return rc;
}

extern "C" int llzs_fft_f64(double *data, int size, const double *cs, int inverse, void *stream)
{
    return launch_fft<arith_f64>(data, 1, size, cs, inverse, stream, "k_fft_radix2<f64>");
}

extern "C" int llzs_fft_fixed(int *data, int count, int size, const short *cs, int inverse, void *stream)
{
    if (data && cs && count >= 1 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        switch (size) {
        case 64: return launch_fft_reg_q15<8, false>(data, count, cs, inverse, stream);
        case 128: return launch_fft_reg_q15<8, true>(data, count, cs, inverse, stream);
        case 256: return launch_fft_reg_q15<16, false>(data, count, cs, inverse, stream);
        case 512: return launch_fft_reg_q15<16, true>(data, count, cs, inverse, stream);
        case 1024: return launch_fft_reg_q15<32, false>(data, count, cs, inverse, stream);
        case 2048: return launch_fft_reg_q15<32, true>(data, count, cs, inverse, stream);
        case 4096: return launch_fft_reg_q15<64, false>(data, count, cs, inverse, stream);
        default: break;
        }
    }
    return launch_fft<arith_q15>(data, count, size, cs, inverse, stream, "k_fft_radix2<q15>");
}

