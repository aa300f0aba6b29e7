// pfb.hip -- uniform DFT polyphase filter bank (include/llz_pfb.h), float32, many channels and frames per launch, on the staged
// passes of fft_core.hpp (M = 8..4096 bands).
//
//   k_pfb_analysis_f32<STAGED>   a workgroup takes a run of n consecutive frames of one channel.  STAGED: the run's span of
//                                L + (n - 1) D samples is read from HBM once into LDS (samples before the call from the handle's
//                                history) and every frame is folded from there; else the fold reads the samples through the
//                                caches.  Groups of tpw frames share the transform images, as in k_stft_analysis_f32.
//   k_pfb_inverse_f32            the 1/M-scaled inverse transforms of a chunk of frames, real parts (rotation undone) into the
//                                handle's scratch [channel][frame][M]
//   k_pfb_ola_f32                one work item per output sample: the tail's partial sum, then g[i] u_m[i mod M] over the chunk's
//                                frames that cover it, oldest first; samples past the chunk's end go to the new tail
// Both analysis forms run pfb_fold's operations in its order, and a transform's passes do not depend on which frames share its
// workgroup: equal bits.
#include "fft_core.hpp"

namespace {

// LDS per workgroup of the staged form: 40 KiB, four workgroups (16 waves) per CU within the 160 KiB of a CU.  The fold and the
// passes are bound by LDS and issue latency, not by HBM: at 64 KiB (two workgroups per CU, longer runs, fewer re-read samples)
// the staged form measured 1.3-1.6x SLOWER than at 40 KiB and slower than the form that reads through the caches; at 32 KiB it
// is within 3 % of 40 KiB either way (polyphase filter bank; 1024 channels, M = 256 and 1024).
constexpr size_t PFB_LDS_BUDGET = 40 * 1024;

// u[r] = sum_p w[r + p M] x[base + p M], p ascending, products and sums rounded one by one (no fused multiply-add).
// AHEAD (the samples come through the caches): all of a residue's loads are issued before the first sum (P is the same for every
// lane: the guards are scalar branches), so the chain of P dependent additions waits for memory once, not P times (M = 1024,
// M / D = 4, P = 8: 2.44 -> 1.82 ms; P = 1 pays 1.07 -> 1.22 ms for the guards, and a plain loop kept beside it for small P cost
// every P registers and time).  From LDS the plain loop is the faster one (P = 1: 0.96 against 1.30 ms).  The same operations in
// the same order either way.
template <bool AHEAD, typename F>
__device__ __forceinline__ float pfb_fold(const float *__restrict__ w, int r, int M, int P, F sample)
{
#pragma clang fp contract(off)
    if (!AHEAD) {
        float acc = w[r] * sample(0);
        for (int p = 1; p < P; p++) {
            const float v = w[r + p * M] * sample(p * M);
            acc = acc + v;
        }
        return acc;
    }
    constexpr int PMAX = 16;                                              // LLZ_PFB_MAX_TAPS
    float wv[PMAX], xv[PMAX];
#pragma unroll
    for (int p = 0; p < PMAX; p++)
        if (p < P) {
            wv[p] = w[r + p * M];
            xv[p] = sample(p * M);
        }
    float acc = wv[0] * xv[0];
#pragma unroll
    for (int p = 1; p < PMAX; p++)
        if (p < P) {
            const float v = wv[p] * xv[p];
            acc = acc + v;
        }
    return acc;
}

template <bool STAGED>
__global__ void __launch_bounds__(FFT_THREADS)
k_pfb_analysis_f32(const float *__restrict__ x, const float *__restrict__ hist, float *__restrict__ re,
                   float *__restrict__ im, const float *__restrict__ w, int frames, int M, int log2m, int D, int P,
                   const float *__restrict__ cs, int tpw, unsigned groups, long x_pitch, int n, int runs, unsigned rot0,
                   unsigned rstep)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tstride = fft_tstride(M);
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    cpx<float> *tw = s + (size_t)tpw * tstride;
    float *span = reinterpret_cast<float *>(tw + tw_entries(M));          // STAGED: L + (n - 1) D floats
    const int tid = threadIdx.x;
    const int c = blockIdx.x / runs, run = blockIdx.x - c * runs;
    const int f0 = run * n, nf = min(n, frames - f0);
    const int L = P * M, keep = L - D, bins = (M >> 1) + 1;
    const long t0 = (long)(f0 + 1) * D - L;                               // the span's first sample, counted from the call's
    const float *row = x + (size_t)c * x_pitch;
    const float *hrow = hist + (size_t)c * keep;
    auto fetch = [&](long t) { return t >= 0 ? row[t] : hrow[keep + t]; };
    fft_load_twiddles(tw, cs, M, tid);
    if (STAGED) {
        const int len = L + (nf - 1) * D;
        for (int q = tid; q < len; q += FFT_THREADS) span[q] = fetch(t0 + q);
    }
    for (int g0 = 0; g0 < nf; g0 += tpw) {
        const int ntr = min(tpw, nf - g0);
        __syncthreads();                                                  // span and twiddles written, s free
        const int total = ntr << log2m;
        for (int e = tid; e < total; e += FFT_THREADS) {
            const int tr = e >> log2m, r = e & (M - 1);
            const int fl = g0 + tr;                                       // frame within the run
            const int base = fl * D + r;                                  // of its sample r within the span
            float acc;
            if (STAGED) acc = pfb_fold<false>(w, r, M, P, [&](int o) { return span[base + o]; });
            else acc = pfb_fold<true>(w, r, M, P, [&](int o) { return fetch(t0 + base + o); });
            const unsigned rot = rot0 + (unsigned)(f0 + fl) * rstep;      // TIME phase: (m + 1) D, taken mod M
            cpx<float> z;
            z.re = acc;
            z.im = 0.f;
            s[tr * tstride + fft_phys((int)((r + rot) & (unsigned)(M - 1)))] = z;
        }
        __syncthreads();
        fft_run<arith_f32, false>(s, ntr, M, log2m, tstride, tw, groups, tid);
        for (int tr = 0; tr < ntr; tr++) {                                // position j holds bin brev(j)
            const size_t o = ((size_t)c * frames + f0 + g0 + tr) * bins;
            for (int b = tid; b < bins; b += FFT_THREADS) {
                const cpx<float> v = s[tr * tstride + fft_phys((int)(__brev((unsigned)b) >> (32 - log2m)))];
                re[o + b] = v.re;
                im[o + b] = v.im;
            }
        }
    }
}

// transform g = c * count + k of the chunk is frame f0 + k of channel c in re / im ([channels][frames][bins])
__global__ void __launch_bounds__(FFT_THREADS)
k_pfb_inverse_f32(const float *__restrict__ re, const float *__restrict__ im, float *__restrict__ u, int frames, int f0,
                  int count, int M, int log2m, const float *__restrict__ cs, int tpw, unsigned groups, long total_tr,
                  unsigned rot0, unsigned rstep)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tstride = fft_tstride(M);
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    cpx<float> *tw = s + (size_t)tpw * tstride;
    const int tid = threadIdx.x;
    const long tr0 = (long)blockIdx.x * tpw;
    const int ntr = (int)min((long)tpw, total_tr - tr0);
    const int bins = (M >> 1) + 1;
    const float inv = 1.0f / (float)M;                                    // a power of two: exact
    fft_load_twiddles(tw, cs, M, tid);
    // spectra into bit-reversed positions: bins 0..M/2 as given, the upper half by Hermitian symmetry
    for (int tr = 0; tr < ntr; tr++) {
        const long g = tr0 + tr;
        const int c = (int)(g / count), k = (int)(g - (long)c * count);
        const size_t o = ((size_t)c * frames + f0 + k) * bins;
        for (int b = tid; b < bins; b += FFT_THREADS) {
            cpx<float> v;
            v.re = re[o + b] * inv;
            v.im = im[o + b] * inv;
            s[tr * tstride + fft_phys((int)(__brev((unsigned)b) >> (32 - log2m)))] = v;
            if (b > 0 && b < (M >> 1)) {
                v.im = -v.im;
                s[tr * tstride + fft_phys((int)(__brev((unsigned)(M - b)) >> (32 - log2m)))] = v;
            }
        }
    }
    __syncthreads();
    fft_run<arith_f32, true>(s, ntr, M, log2m, tstride, tw, groups, tid);
    const int total = ntr << log2m;
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2m, r = e & (M - 1);
        const long g = tr0 + tr;
        const int k = (int)(g % count);
        const unsigned rot = rot0 + (unsigned)k * rstep;
        u[(size_t)g * M + r] = s[tr * tstride + fft_phys((int)((r + rot) & (unsigned)(M - 1)))].re;
    }
}

// position p counts from the chunk's first output sample: p < keep starts from the old tail, p < count D is an output, the
// rest is the new tail
__global__ void __launch_bounds__(256)
k_pfb_ola_f32(const float *__restrict__ u, float *__restrict__ x, const float *__restrict__ tail_old,
              float *__restrict__ tail_new, const float *__restrict__ g, int count, int M, int D, int L, long x_pitch)
{
#pragma clang fp contract(off)
    const int c = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int keep = L - D;
    const long out = (long)count * D;
    if (p >= out + keep) return;
    float a = p < keep ? tail_old[(size_t)c * keep + p] : 0.f;
    const int k_hi = (int)min((long)count - 1, p / D);                    // frames k with 0 <= p - k D < L
    const int k_lo = p < L ? 0 : (int)((p - L) / D) + 1;
    const float *urow = u + (size_t)c * count * M;
    if (k_hi - k_lo < 2) {                                                // one or two terms (R <= 2, a call's edges)
        for (int k = k_lo; k <= k_hi; k++) {
            const int i = (int)(p - (long)k * D);
            const float v = g[i] * urow[(size_t)k * M + (i & (M - 1))];
            a = a + v;
        }
    } else {
        for (int k0 = k_lo; k0 <= k_hi; k0 += 8) {                        // eight frames' loads in flight, the sums in order
            float gv[8], uv[8];                                           // (R = 32: 2.69 -> 2.13 ms at M = 1024, P = 8)
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (k0 + j <= k_hi) {
                    const int i = (int)(p - (long)(k0 + j) * D);
                    gv[j] = g[i];
                    uv[j] = urow[(size_t)(k0 + j) * M + (i & (M - 1))];
                }
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (k0 + j <= k_hi) {
                    const float v = gv[j] * uv[j];
                    a = a + v;
                }
        }
    }
    if (p < out) x[(size_t)c * x_pitch + p] = a;
    else tail_new[(size_t)c * keep + (p - out)] = a;
}

struct pfb_plan {
    int form, n, tpw, runs;
    size_t lds;
};

// analysis: the frames per workgroup.  STAGED where the images, the twiddles and the span of at least one group of tpw frames
// fit PFB_LDS_BUDGET; then as many frames as fit, no more than four prototype lengths of hops (the re-read of L - D samples per
// run is below a quarter by then), and fewer while the grid would stay below 1024 workgroups.
static pfb_plan pfb_analysis_plan(int channels, int frames, int M, int D, int L)
{
    const fft_plan pl = fft_make_plan<arith_f32>(M, frames);
    pfb_plan p;
    p.tpw = pl.tpw;
    const long fit = PFB_LDS_BUDGET >= pl.lds + sizeof(float) * (size_t)L
                         ? (long)((PFB_LDS_BUDGET - pl.lds - sizeof(float) * (size_t)L) / (sizeof(float) * (size_t)D)) + 1 : 0;
    p.form = (fit >= pl.tpw && llzs_tune(LLZS_TUNE_PFB_GLOBAL) != 1) ? 0 : 1;
    long n = pl.tpw;
    if (p.form == 0) {
        n = fit < frames ? fit : frames;
        if (n > 4L * L / D) n = 4L * L / D;
        n -= n % pl.tpw;
        if (n < pl.tpw) n = pl.tpw;
        while (n > pl.tpw && (long)channels * ((frames + n - 1) / n) < 1024) {
            n /= 2;
            n -= n % pl.tpw;
            if (n < pl.tpw) n = pl.tpw;
        }
    }
    p.n = (int)n;
    p.runs = (int)((frames + n - 1) / n);
    p.lds = pl.lds + (p.form == 0 ? sizeof(float) * ((size_t)L + (size_t)(n - 1) * D) : 0);
    return p;
}

static int pfb_shape(const char *who, int channels, int frames, int M, int D, int L, int *log2m)
{
    *log2m = 0;
    while ((1 << *log2m) < M) (*log2m)++;
    const int os = D > 0 ? M / D : 0;
    if (channels < 1 || channels > 65535 || frames < 1 || M < 8 || M > 4096 || (1 << *log2m) != M || D < 1 || os * D != M ||
        (os != 1 && os != 2 && os != 4 && os != 8) || L < M || L % M || L > 16 * M || L > 32768 ||
        (long)frames * D > 2147483647L) {
        llzs_set_error("%s: bad shape (channels=%d frames=%d bands=%d hop=%d length=%d)", who, channels, frames, M, D, L);
        return LLZ_ERR_ARG;
    }
    return LLZ_OK;
}

} // namespace

extern "C" int llzs_pfb_analysis_f32(const float *x, const float *hist, float *re, float *im, const float *w, const float *cs,
                                     int channels, int frames, int M, int D, int L, int rot0, int rstep, long x_pitch,
                                     void *stream)
{
    int log2m;
    if (!x || !hist || !re || !im || !w || !cs || x_pitch < (long)frames * D) {
        llzs_set_error("pfb_analysis_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = pfb_shape("pfb_analysis_f32", channels, frames, M, D, L, &log2m);
    if (rc != LLZ_OK) return rc;
    const pfb_plan pl = pfb_analysis_plan(channels, frames, M, D, L);
    if ((long)channels * pl.runs >= (1L << 24)) {
        llzs_set_error("pfb_analysis_f32: %d channels x %d runs of %d frames exceed the grid; split the call", channels, pl.runs,
                       pl.n);
        return LLZ_ERR_RANGE;
    }
    const dim3 grid((unsigned)((long)channels * pl.runs));
    fft_pick(pl.form == 0, [&](auto staged) {
        hipLaunchKernelGGL(k_pfb_analysis_f32<staged()>, grid, dim3(FFT_THREADS), pl.lds, as_stream(stream), x, hist, re, im, w,
                           frames, M, log2m, D, L / M, cs, pl.tpw, fft_groups(log2m), x_pitch, pl.n, pl.runs, (unsigned)rot0,
                           (unsigned)rstep);
    });
    LLZ_LAUNCH_CHECK("k_pfb_analysis_f32");
    return LLZ_OK;
}

extern "C" int llzs_pfb_inverse_f32(const float *re, const float *im, float *u, const float *cs, int channels, int frames,
                                    int f0, int count, int M, int D, int rot0, int rstep, void *stream)
{
    int log2m;
    if (!re || !im || !u || !cs || f0 < 0 || count < 1 || f0 > frames - count) {
        llzs_set_error("pfb_inverse_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = pfb_shape("pfb_inverse_f32", channels, frames, M, D, M, &log2m);
    if (rc != LLZ_OK) return rc;
    const long total_tr = (long)channels * count;
    const fft_plan pl = fft_make_plan<arith_f32>(M, total_tr);
    hipLaunchKernelGGL(k_pfb_inverse_f32, dim3((unsigned)pl.blocks), dim3(FFT_THREADS), pl.lds, as_stream(stream), re, im, u,
                       frames, f0, count, M, log2m, cs, pl.tpw, fft_groups(log2m), total_tr, (unsigned)rot0, (unsigned)rstep);
    LLZ_LAUNCH_CHECK("k_pfb_inverse_f32");
    return LLZ_OK;
}

extern "C" int llzs_pfb_ola_f32(const float *u, float *x, const float *tail_old, float *tail_new, const float *g, int channels,
                                int count, int M, int D, int L, long x_pitch, void *stream)
{
    int log2m;
    if (!u || !x || !tail_old || !tail_new || tail_old == tail_new || !g || x_pitch < (long)count * D) {
        llzs_set_error("pfb_ola_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = pfb_shape("pfb_ola_f32", channels, count, M, D, L, &log2m);
    if (rc != LLZ_OK) return rc;
    const long total = (long)count * D + (L - D);
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)channels);
    hipLaunchKernelGGL(k_pfb_ola_f32, grid, dim3(256), 0, as_stream(stream), u, x, tail_old, tail_new, g, count, M, D, L,
                       x_pitch);
    LLZ_LAUNCH_CHECK("k_pfb_ola_f32");
    return LLZ_OK;
}

extern "C" int llzs_pfb_plan(int channels, int frames, int chunk, int M, int D, int L, int *out)
{
    int log2m;
    if (!out || chunk < 1 || chunk > frames) {
        llzs_set_error("pfb_plan: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = pfb_shape("pfb_plan", channels, frames, M, D, L, &log2m);
    if (rc != LLZ_OK) return rc;
    const pfb_plan a = pfb_analysis_plan(channels, frames, M, D, L);
    const fft_plan s = fft_make_plan<arith_f32>(M, (long)channels * chunk);
    out[0] = a.form; out[1] = a.n; out[2] = (int)((long)channels * a.runs); out[3] = (int)a.lds;
    out[4] = 1; out[5] = s.tpw; out[6] = (int)s.blocks; out[7] = (int)s.lds;
    return LLZ_OK;
}
