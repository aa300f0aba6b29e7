// stft.hip -- windowed-FFT analysis / synthesis frames (reference libllzfilter/llz_asmodel.c:180-310)
// for fft_len up to 4096, float32, many channels and frames per launch (above 4096: stft_large.hip).
//
//   k_stft_analysis_f32 / k_stft_synthesis_f32           any fft_len 8..4096 on the staged passes of fft_core.hpp
//   k_stft_analysis_reg_f32 / k_stft_synthesis_reg_f32   fft_len 256, 512, 2048 on square_core (fft_square.hpp)
//   k_stft_analysis1024_f32 / k_stft_synthesis1024_f32   fft_len 1024 on the half-wave machinery of fft32.hpp
// The two register synthesis kernels share their overlap-add walk (stft_ola_walk, fft_square.hpp).
#include "fft_square.hpp"

namespace {

// size = R * frame_len with R = 4 (3/4 overlap) or 2 (1/2 overlap).
//
// analysis: frame f of channel c is samples [(f+1)F - size, (f+1)F) of concat(hist, x) times the window; bins 0..size/2
// of its transform go to re/im[(c*frames + f)*bins + b] (llz_asmodel.c:188-204).  tpw frames share a workgroup.
__global__ void __launch_bounds__(FFT_THREADS)
k_stft_analysis_f32(const float *__restrict__ x, const float *__restrict__ hist, float *__restrict__ re,
                    float *__restrict__ im, const float *__restrict__ w, int frames, int F, int size, int log2n,
                    const float *__restrict__ cs, int tpw, unsigned groups, long x_pitch, long total_tr)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    const int tid = threadIdx.x;
    const long tr0 = (long)blockIdx.x * tpw;
    const int ntr = (int)min((long)tpw, total_tr - tr0);
    const int tstride = fft_tstride(size);
    const int total = ntr << log2n;
    const int keep = size - F;                                         // history samples in front of a call
    cpx<float> *tw = s + (size_t)tpw * tstride;
    fft_load_twiddles(tw, cs, size, tid);
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2n, i = e & (size - 1);
        const long g = tr0 + tr;
        const int c = (int)(g / frames), f = (int)(g - (long)c * frames);
        const long t = (long)(f + 1) * F - size + i;                   // sample index inside this call
        const float v = t >= 0 ? x[(size_t)c * x_pitch + t] : hist[(size_t)c * keep + (keep + t)];
        cpx<float> z;
        z.re = v * w[i];
        z.im = 0.f;
        s[tr * tstride + fft_phys(i)] = z;
    }
    __syncthreads();
    fft_run<arith_f32, false>(s, ntr, size, log2n, tstride, tw, groups, tid);
    const int bins = (size >> 1) + 1;                                  // position j holds bin brev(j)
    for (int tr = 0; tr < ntr; tr++) {
        const size_t o = (size_t)(tr0 + tr) * bins;
        for (int b = tid; b < bins; b += FFT_THREADS) {
            const cpx<float> v = s[tr * tstride + fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))];
            re[o + b] = v.re;
            im[o + b] = v.im;
        }
    }
}

// fft_len = 1024 analysis frames on the half-wave machinery of k_fft1024_f32: the windowed samples go from HBM straight
// into registers (imaginary parts zero), bins 0..512 straight back; 8 frames per workgroup.
__global__ void __launch_bounds__(256)
k_stft_analysis1024_f32(const float *__restrict__ x, const float *__restrict__ hist, float *__restrict__ re,
                        float *__restrict__ im, const float *__restrict__ w, int frames, int F,
                        const float *__restrict__ cs, long x_pitch, long total_tr)
{
    __shared__ float2 s_tw[1024];
    __shared__ float bufs[8][OLS_XBUF];
    const int tid = threadIdx.x, hw = tid >> 5, l5 = tid & 31;
    load_tw1024(s_tw, cs, tid);
    __syncthreads();
    const long g = (long)blockIdx.x * 8 + hw;
    if (g >= total_tr) return;
    const int c = (int)(g / frames), f = (int)(g - (long)c * frames);
    const int keep = 1024 - F;
    const long t0 = (long)(f + 1) * F - 1024;
    const float *row = x + (size_t)c * x_pitch;
    const float *hrow = hist + (size_t)c * keep;
    cf v[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int i = l5 + 32 * j;
        const long t = t0 + i;
        const float smp = t >= 0 ? row[t] : hrow[keep + t];
        v[j] = cf{smp * w[i], 0.f};
    }
    fft32<false>(v);
    transpose_twiddle<false>(v, bufs[hw], s_tw, l5);
    fft32<false>(v);
    const size_t o = (size_t)g * 513;
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const int bin = l5 + 32 * brev5(q);                         // v[q] = X[l5 + 32 brev5(q)]
        if (bin <= 512) {
            re[o + bin] = v[q].x;
            im[o + bin] = v[q].y;
        }
    }
}

// synthesis: a workgroup owns output blocks [b0, b1) of one channel.  Block t (frame_len samples) is the sum of the
// windowed inverse transforms of frames t-R+1 .. t (llz_asmodel.c:279-304), so the workgroup walks frames
// max(0, b0-R+1) .. b1-1 in groups of tpw, keeps the running overlap-add tail (size - F samples) in LDS and drops the
// blocks in front of b0 (their sums are incomplete; the first run of a channel starts from the handle's tail instead).
// Accumulation order per sample is the reference's: oldest frame first.  ACC = FFT_THREADS-sample slices of a group's
// span: 8 up to fft_len 2048 (tpw frames in 2048 points), 16 for the one-frame groups of fft_len 4096.
template <int ACC>
__global__ void __launch_bounds__(FFT_THREADS)
k_stft_synthesis_f32(const float *__restrict__ re, const float *__restrict__ im, float *__restrict__ x,
                     const float *__restrict__ ola_old, float *__restrict__ ola_new, const float *__restrict__ w,
                     int frames, int F, int size, int log2n, const float *__restrict__ cs, int tpw, unsigned groups,
                     long x_pitch, int run_len, int runs, float magic)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tstride = fft_tstride(size);
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    cpx<float> *tw = s + (size_t)tpw * tstride;
    float *carry = reinterpret_cast<float *>(tw + tw_entries(size));      // size - F floats
    const int tid = threadIdx.x;
    const int c = blockIdx.x / runs, run = blockIdx.x - c * runs;
    const int b0 = run * run_len, b1 = min(frames, b0 + run_len);
    const int R = size / F, keep = size - F, bins = (size >> 1) + 1;
    const int fs = max(0, b0 - (R - 1));
    fft_load_twiddles(tw, cs, size, tid);
    for (int q = tid; q < keep; q += FFT_THREADS) carry[q] = fs == 0 ? ola_old[(size_t)c * keep + q] : 0.f;
    const float inv = 1.0f / (float)size;                                  // llz_ifft divides by N (llz_fft.c:187-195)
    for (int g0 = fs; g0 < b1; g0 += tpw) {
        const int ng = min(tpw, b1 - g0);
        __syncthreads();                                                   // carry written, s free
        // spectra into bit-reversed positions: bins 0..size/2 as given, the upper half by Hermitian symmetry
        for (int tr = 0; tr < ng; tr++) {
            const size_t o = ((size_t)c * frames + g0 + tr) * bins;
            for (int b = tid; b < bins; b += FFT_THREADS) {
                cpx<float> v;
                v.re = re[o + b] * inv;
                v.im = im[o + b] * inv;
                s[tr * tstride + fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))] = v;
                if (b > 0 && b < (size >> 1)) {
                    v.im = -v.im;
                    s[tr * tstride + fft_phys((int)(__brev((unsigned)(size - b)) >> (32 - log2n)))] = v;
                }
            }
        }
        __syncthreads();
        fft_run<arith_f32, true>(s, ng, size, log2n, tstride, tw, groups, tid);
        // overlap-add over the group's span: position p counts from the group's first block
        const int span = (ng - 1) * F + size;                              // <= ACC * FFT_THREADS
        float acc[ACC];
#pragma unroll
        for (int m = 0; m < ACC; m++) {
            const int p = tid + m * FFT_THREADS;
            float a = 0.f;
            if (p < span) {
                a = p < keep ? carry[p] : 0.f;
                const int k_hi = min(ng - 1, p / F);                       // frames k with 0 <= p - kF < size
                const int k_lo = p < size ? 0 : (p - size) / F + 1;
                for (int k = k_lo; k <= k_hi; k++) {
                    const int i = p - k * F;
                    a += s[k * tstride + fft_phys(i)].re * w[i];
                }
            }
            acc[m] = a;
        }
        __syncthreads();                                                   // every read of carry and s is done
#pragma unroll
        for (int m = 0; m < ACC; m++) {
            const int p = tid + m * FFT_THREADS;
            if (p < span) {
                if (p < ng * F) {
                    if (g0 + p / F >= b0) x[(size_t)c * x_pitch + (size_t)g0 * F + p] = magic * acc[m];
                } else {
                    carry[p - ng * F] = acc[m];
                }
            }
        }
    }
    __syncthreads();
    if (b1 == frames)
        for (int q = tid; q < keep; q += FFT_THREADS) ola_new[(size_t)c * keep + q] = carry[q];
}

// fft_len = 1024 synthesis: as k_stft_synthesis_f32, with the inverse transforms on the half-wave machinery (8 frames per
// group, one per half-wave): bins from HBM straight into registers with the Hermitian upper half taken from the mirrored
// bin, windowed real output written to an LDS segment image, then the same overlap-add walk.
__global__ void __launch_bounds__(256)
k_stft_synthesis1024_f32(const float *__restrict__ re, const float *__restrict__ im, float *__restrict__ x,
                         const float *__restrict__ ola_old, float *__restrict__ ola_new, const float *__restrict__ w,
                         int frames, int F, const float *__restrict__ cs, long x_pitch, int run_len, int runs, float magic)
{
    constexpr int N = 1024, TPW = 8;
    __shared__ float2 s_tw[1024];
    __shared__ float bufs[TPW][OLS_XBUF];
    __shared__ float seg[TPW][N];
    __shared__ float carry[N];                                         // N - F used
    const int tid = threadIdx.x, hw = tid >> 5, l5 = tid & 31;
    load_tw1024(s_tw, cs, tid);
    stft_ola_walk(seg, carry, x, ola_old, ola_new, frames, F, x_pitch, run_len, runs, magic, tid,
                  [&](int c, int g0, int ng) {
        if (hw < ng) {
            const size_t o = ((size_t)c * frames + g0 + hw) * 513;
            cf v[32];
#pragma unroll
            for (int j = 0; j < 32; j++) {
                const int k = l5 + 32 * j;
                const int kk = k <= 512 ? k : N - k;                   // upper half: conjugate of the mirrored bin
                const float a = re[o + kk] * (1.0f / 1024.0f), b = im[o + kk] * (1.0f / 1024.0f);
                v[j] = cf{a, k <= 512 ? b : -b};
            }
            fft32<true>(v);
            transpose_twiddle<true>(v, bufs[hw], s_tw, l5);
            fft32<true>(v);
#pragma unroll
            for (int q = 0; q < 32; q++) {
                const int n = l5 + 32 * brev5(q);                      // v[q].x = real part of sample n
                seg[hw][n] = v[q].x * w[n];
            }
        }
    });
}

// Analysis frames for fft_len = E^2 (E = 16: 256) or 2 E^2 (TWO; E = 16: 512, E = 32: 2048) on a group of E lanes per
// frame: k_stft_analysis1024_f32's scheme on square_core -- windowed samples from HBM straight into the registers of the
// lane that transforms them, bins 0..size/2 straight back.
// (fft_len 2048 needs 273 VGPRs: two waves per SIMD asked for, 0.68 -> 0.63 ms)
template <int E, bool TWO>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((E == 32 && TWO) ? 2 : 1)))
k_stft_analysis_reg_f32(const float *__restrict__ x, const float *__restrict__ hist, float *__restrict__ re,
                        float *__restrict__ im, const float *__restrict__ w, int frames, int F,
                        const float2 *__restrict__ tw2d, const float2 *__restrict__ tw1, long x_pitch, long total_tr)
{
    constexpr int H = E * E, SIZE = TWO ? 2 * H : H, GROUPS = 256 / E, PITCH = E + 1, BINS = SIZE / 2 + 1;
    __shared__ float bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    const long g = (long)blockIdx.x * GROUPS + grp;
    if (g >= total_tr) return;
    const int c = (int)(g / frames), f = (int)(g - (long)c * frames);
    const int keep = SIZE - F;
    const long t0 = (long)(f + 1) * F - SIZE;
    const float *row = x + (size_t)c * x_pitch;
    const float *hrow = hist + (size_t)c * keep;
    float *buf = bufs[grp];
    auto sample = [&](int i) {
        const long t = t0 + i;
        return (t >= 0 ? row[t] : hrow[keep + t]) * w[i];
    };
    const size_t o = (size_t)g * BINS;
    if (!TWO) {
        cf v[E];
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = cf{sample(lg + E * j), 0.f};
        square_core<E, false>(v, buf, tw2d, lg);                    // v[q] = X[lg + E brevE(q)]
#pragma unroll
        for (int q = 0; q < E; q++) {
            const int bin = lg + E * brevE<E>(q);
            if (bin < BINS) { re[o + bin] = v[q].x; im[o + bin] = v[q].y; }
        }
    } else {
        cf s[E], d[E];
#pragma unroll
        for (int j = 0; j < E; j++) {                               // real input: s, d before the twist are real
            const float a = sample(lg + E * j), b = sample(lg + E * j + H);
            const float2 t = tw1[j * E + lg];
            s[j] = cf{a + b, 0.f};
            d[j] = cf{(a - b) * t.x, (a - b) * t.y};
        }
        square_core<E, false>(s, buf, tw2d, lg);                    // s[q] = X[2 kq], d[q] = X[2 kq + 1], kq = lg + E brevE(q)
        square_core<E, false>(d, buf, tw2d, lg);
#pragma unroll
        for (int q = 0; q < E; q++) {
            const int bin = 2 * (lg + E * brevE<E>(q));
            if (bin < BINS) { re[o + bin] = s[q].x; im[o + bin] = s[q].y; }
            if (bin + 1 < BINS) { re[o + bin + 1] = d[q].x; im[o + bin + 1] = d[q].y; }
        }
    }
}

// Synthesis frames for the same sizes: k_stft_synthesis1024_f32's walk (bins from HBM into registers with the Hermitian
// upper half taken from the mirrored bin, inverse transform, windowed real output into an LDS segment image, overlap-add
// in the reference's order, oldest frame first) with 256 / E frames per group on square_core.
// HALF (fft_len = 2 E^2): the spectrum of a REAL frame of N = 2H samples needs ONE H-point complex inverse transform, not two:
// with E[k] = (X[k] + conj(X[H-k])) / 2 and O[k] = (X[k] - conj(X[H-k])) W_N^-k / 2 (the spectra of the even and the odd samples),
// z = IDFT_H(E + j O) is x[2n] + j x[2n+1].  Both bins come from HBM (the mirrored one by its own index: no lane exchange), the
// results leave as (even, odd) pairs: half the transform work of the TWO form (1024 ch x 128 frames at 3/4 overlap, fft_len 2048:
// 1.89 -> 1.15 ms; fft_len 512, 256 frames at 1/2 overlap: 0.48 -> 0.33 ms).  cs: cos, then sin of 2 pi i / N.
// (At fft_len 2048 eight frame images are 64 KB and allow ONE workgroup per CU; letting the frames enter a four-frame image in
//  two parts -- 75 KB, two workgroups per CU, two more barriers per group -- measured slower, 1.15 -> 1.32 ms.)
template <int E, bool TWO, bool HALF>
__global__ void __launch_bounds__(256)
k_stft_synthesis_reg_f32(const float *__restrict__ re, const float *__restrict__ im, float *__restrict__ x,
                         const float *__restrict__ ola_old, float *__restrict__ ola_new, const float *__restrict__ w,
                         int frames, int F, const float2 *__restrict__ tw2d, const float2 *__restrict__ tw1, long x_pitch,
                         int run_len, int runs, float magic, const float *__restrict__ cs)
{
    static_assert(!(TWO && HALF), "the half-size form runs one square transform");
    constexpr int H = E * E, N = (TWO || HALF) ? 2 * H : H, TPW = 256 / E, PITCH = E + 1, BINS = N / 2 + 1;
    __shared__ float bufs[TPW][E * PITCH];
    __shared__ float seg[TPW][N];
    __shared__ float carry[N];                                         // N - F used
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    constexpr float sc = 1.0f / (float)N;
    stft_ola_walk(seg, carry, x, ola_old, ola_new, frames, F, x_pitch, run_len, runs, magic, tid,
                  [&](int c, int g0, int ng) {
        if (grp < ng) {
            const size_t o = ((size_t)c * frames + g0 + grp) * BINS;
            auto bin = [&](int k) {                                    // upper half: conjugate of the mirrored bin
                const int kk = k <= N / 2 ? k : N - k;
                const float a = re[o + kk] * sc, b = im[o + kk] * sc;
                return cf{a, k <= N / 2 ? b : -b};
            };
            float *buf = bufs[grp];
            if constexpr (HALF) {
                cf v[E];
#pragma unroll
                for (int j = 0; j < E; j++) {
                    const int k = lg + E * j;                          // 0 .. H-1; its partner H - k is in 1 .. H
                    // (bins 0 and H are real in the spectrum of a real frame; whatever their imaginary parts hold reaches only the
                    //  imaginary output of the full-size transform, which is dropped: the same here)
                    const float xr = re[o + k], xi = k == 0 ? 0.f : im[o + k], mr = re[o + H - k], mi = k == 0 ? 0.f : -im[o + H - k];
                    const float sr = xr + mr, si = xi + mi, dr = xr - mr, di = xi - mi;
                    const float cw = cs[k], sn = cs[N + k];            // W_N^-k = cw + j sn
                    const float orr = dr * cw - di * sn, oi = dr * sn + di * cw;     // (X[k] - conj X[H-k]) W_N^-k
                    v[j] = cf{(sr - oi) * sc, (si + orr) * sc};        // (E + j O) / H = (S + j D W) / N
                }
                square_core<E, true>(v, buf, tw2d, lg);                // v[q] = x[2n] + j x[2n+1], n = lg + E brevE(q)
#pragma unroll
                for (int q = 0; q < E; q++) {
                    const int n = lg + E * brevE<E>(q);
                    const float2 ww = *reinterpret_cast<const float2 *>(w + 2 * n);
                    *reinterpret_cast<float2 *>(&seg[grp][2 * n]) = make_float2(v[q].x * ww.x, v[q].y * ww.y);
                }
            } else if (!TWO) {
                cf v[E];
#pragma unroll
                for (int j = 0; j < E; j++) v[j] = bin(lg + E * j);
                square_core<E, true>(v, buf, tw2d, lg);                // v[q].x = sample lg + E brevE(q)
#pragma unroll
                for (int q = 0; q < E; q++) {
                    const int n = lg + E * brevE<E>(q);
                    seg[grp][n] = v[q].x * w[n];
                }
            } else {
                cf s[E], d[E];
#pragma unroll
                for (int j = 0; j < E; j++) {
                    s[j] = bin(2 * (lg + E * j));
                    d[j] = bin(2 * (lg + E * j) + 1);
                }
                square_core<E, true>(s, buf, tw2d, lg);
                square_core<E, true>(d, buf, tw2d, lg);
#pragma unroll
                for (int q = 0; q < E; q++) {                          // n = lg + E brevE(q): x[n], x[n + H] = s +- d conj(W_N^n)
                    const int n = lg + E * brevE<E>(q);
                    const float2 t = tw1[brevE<E>(q) * E + lg];
                    const float wdx = __builtin_fmaf(d[q].y, t.y, d[q].x * t.x);   // Re(d * conj(t))
                    seg[grp][n] = (s[q].x + wdx) * w[n];
                    seg[grp][n + H] = (s[q].x - wdx) * w[n + H];
                }
            }
        }
    });
}

} // namespace

static int stft_check(int channels, int frames, int F, int size, int *log2n, const char *who)
{
    *log2n = 0;
    while ((1 << *log2n) < size) (*log2n)++;
    if (channels < 1 || frames < 1 || F < 1 || size < 8 || size > 4096 || (1 << *log2n) != size ||
        (size != 2 * F && size != 4 * F)) {
        llzs_set_error("%s: bad shape (channels=%d frames=%d frame_len=%d fft_len=%d; fft_len a power of two in 8..4096)",
                       who, channels, frames, F, size);
        return LLZ_ERR_ARG;
    }
    return LLZ_OK;
}

// twiddle tables of the lane-group kernels for fft_len 256 (E = 16), 512 (2 x 16^2), 2048 (2 x 32^2), derived once per
// device from the handle's table cs
static int stft_reg_tables(int size, const float *cs, void *stream, const float2 **tw2d, const float2 **tw1)
{
    const bool two = size != 256;
    return fft_derived_tables(5, size, size == 2048 ? 32 : 16, two ? 2 : 1, two, cs, stream, "stft twiddle tables", tw2d, tw1);
}

extern "C" int llzs_stft_analysis_f32(const float *x, const float *hist, float *re, float *im, const float *w,
                                      const float *cs, int channels, int frames, int F, int size, long x_pitch,
                                      void *stream)
{
    int log2n;
    if (!x || !hist || !re || !im || !w || !cs || x_pitch < (long)frames * F) {
        llzs_set_error("stft_analysis_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = stft_check(channels, frames, F, size, &log2n, "stft_analysis_f32");
    if (rc != LLZ_OK) return rc;
    const long total_tr = (long)channels * frames;
    if ((size == 256 || size == 512 || size == 2048) && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        const float2 *tw2d = nullptr, *tw1 = nullptr;
        const int trc = stft_reg_tables(size, cs, stream, &tw2d, &tw1);
        if (trc != LLZ_OK) return trc;
        const int E = size == 2048 ? 32 : 16;
        const unsigned blocks = (unsigned)((total_tr + (256 / E) - 1) / (256 / E));
        if (size == 256)
            hipLaunchKernelGGL((k_stft_analysis_reg_f32<16, false>), dim3(blocks), dim3(256), 0, as_stream(stream), x, hist,
                               re, im, w, frames, F, tw2d, tw1, x_pitch, total_tr);
        else if (size == 512)
            hipLaunchKernelGGL((k_stft_analysis_reg_f32<16, true>), dim3(blocks), dim3(256), 0, as_stream(stream), x, hist, re,
                               im, w, frames, F, tw2d, tw1, x_pitch, total_tr);
        else
            hipLaunchKernelGGL((k_stft_analysis_reg_f32<32, true>), dim3(blocks), dim3(256), 0, as_stream(stream), x, hist, re,
                               im, w, frames, F, tw2d, tw1, x_pitch, total_tr);
        LLZ_LAUNCH_CHECK("k_stft_analysis_reg_f32");
        return LLZ_OK;
    }
    if (size == 1024 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        hipLaunchKernelGGL(k_stft_analysis1024_f32, dim3((unsigned)((total_tr + 7) / 8)), dim3(256), 0, as_stream(stream),
                           x, hist, re, im, w, frames, F, cs, x_pitch, total_tr);
        LLZ_LAUNCH_CHECK("k_stft_analysis1024_f32");
        return LLZ_OK;
    }
    const fft_plan pl = fft_make_plan<arith_f32>(size, total_tr);       // 4096: one frame per workgroup, 50 KB of LDS
    hipLaunchKernelGGL(k_stft_analysis_f32, dim3((unsigned)pl.blocks), dim3(FFT_THREADS), pl.lds, as_stream(stream), x, hist,
                       re, im, w, frames, F, size, log2n, cs, pl.tpw, fft_groups(log2n), x_pitch, total_tr);
    LLZ_LAUNCH_CHECK("k_stft_analysis_f32");
    return LLZ_OK;
}

extern "C" int llzs_stft_synthesis_f32(const float *re, const float *im, float *x, const float *ola_old, float *ola_new,
                                       const float *w, const float *cs, int channels, int frames, int F, int size,
                                       long x_pitch, float magic, void *stream)
{
    int log2n;
    if (!re || !im || !x || !ola_old || !ola_new || ola_old == ola_new || !w || !cs || x_pitch < (long)frames * F) {
        llzs_set_error("stft_synthesis_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const int rc = stft_check(channels, frames, F, size, &log2n, "stft_synthesis_f32");
    if (rc != LLZ_OK) return rc;
    const int R = size / F;
    const fft_plan pl = fft_make_plan<arith_f32>(size, frames, (size_t)(size - F) * sizeof(float));   // + the carry
    const int tpw = pl.tpw;
    // blocks per workgroup: enough workgroups to fill the chip, long enough that the R-1 warm-up frames stay cheap
    long want = ((long)frames * channels + 2047) / 2048;
    if (want > frames) want = frames;                                   // (clamped before the int: no overflow)
    int run_len = (int)(want < 8 * R ? 8 * R : want);
    if (run_len < tpw) run_len = tpw;
    if (run_len > frames) run_len = frames;
    if ((size == 256 || size == 512 || size == 2048) && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        const float2 *tw2d = nullptr, *tw1 = nullptr;
        const int trc = stft_reg_tables(size, cs, stream, &tw2d, &tw1);
        if (trc != LLZ_OK) return trc;
        const int gt = size == 2048 ? 8 : 16;                           // frames per group
        if (run_len < gt * R) run_len = gt * R;
        if (run_len > frames) run_len = frames;
        const int runsr = (frames + run_len - 1) / run_len;
        const dim3 grid((unsigned)((long)channels * runsr));
        // (fft_len 512 and 2048: the half-size form; tw2d of those sizes IS the E^2-point table derived from the 2 E^2-point one)
        const bool full = llzs_tune(LLZS_TUNE_STFT_FULL) == 1;
        if (size == 256)
            hipLaunchKernelGGL((k_stft_synthesis_reg_f32<16, false, false>), grid, dim3(256), 0, as_stream(stream), re, im, x,
                               ola_old, ola_new, w, frames, F, tw2d, tw1, x_pitch, run_len, runsr, magic, cs);
        else if (size == 512 && full)
            hipLaunchKernelGGL((k_stft_synthesis_reg_f32<16, true, false>), grid, dim3(256), 0, as_stream(stream), re, im, x,
                               ola_old, ola_new, w, frames, F, tw2d, tw1, x_pitch, run_len, runsr, magic, cs);
        else if (size == 512)
            hipLaunchKernelGGL((k_stft_synthesis_reg_f32<16, false, true>), grid, dim3(256), 0, as_stream(stream), re, im, x,
                               ola_old, ola_new, w, frames, F, tw2d, tw1, x_pitch, run_len, runsr, magic, cs);
        else if (full)
            hipLaunchKernelGGL((k_stft_synthesis_reg_f32<32, true, false>), grid, dim3(256), 0, as_stream(stream), re, im, x,
                               ola_old, ola_new, w, frames, F, tw2d, tw1, x_pitch, run_len, runsr, magic, cs);
        else
            hipLaunchKernelGGL((k_stft_synthesis_reg_f32<32, false, true>), grid, dim3(256), 0, as_stream(stream), re, im, x,
                               ola_old, ola_new, w, frames, F, tw2d, tw1, x_pitch, run_len, runsr, magic, cs);
        LLZ_LAUNCH_CHECK("k_stft_synthesis_reg_f32");
        return LLZ_OK;
    }
    if (size == 1024 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        if (run_len < 8 * R) run_len = 8 * R;
        if (run_len > frames) run_len = frames;
        const int runs1k = (frames + run_len - 1) / run_len;
        hipLaunchKernelGGL(k_stft_synthesis1024_f32, dim3((unsigned)((long)channels * runs1k)), dim3(256), 0,
                           as_stream(stream), re, im, x, ola_old, ola_new, w, frames, F, cs, x_pitch, run_len, runs1k,
                           magic);
        LLZ_LAUNCH_CHECK("k_stft_synthesis1024_f32");
        return LLZ_OK;
    }
    const int runs = (frames + run_len - 1) / run_len;
    const dim3 grid((unsigned)((long)channels * runs));
    fft_pick(size <= 2048, [&](auto small) {                            // 4096: one frame per group, <= 62 KB of LDS
        hipLaunchKernelGGL(k_stft_synthesis_f32<small() ? 8 : 16>, grid, dim3(FFT_THREADS), pl.lds, as_stream(stream), re, im,
                           x, ola_old, ola_new, w, frames, F, size, log2n, cs, tpw, fft_groups(log2n), x_pitch, run_len, runs,
                           magic);
    });
    LLZ_LAUNCH_CHECK("k_stft_synthesis_f32");
    return LLZ_OK;
}
