// tde.hip -- streaming time-delay estimator of many channel pairs (include/llz_tde.h, host layer llz_tde_host.c): generalised
// cross-correlation with CC, PHAT or SCOT weighting on recursively averaged cross-spectra, float32 transforms on the staged
// passes of fft_core.hpp, fft_len 64..4096, hop fft_len, fft_len / 2 or fft_len / 4.
//
//   k_tde_staged_f32        a workgroup per pair, one launch per call.  The workgroup walks the call's frames in order: the
//                           recursion S_f = lam S_{f-1} + g P_f is serial in f, and its state (Re S, Im S, Gx, Gy of the bins a
//                           thread owns) stays in registers from the call's first frame to its last.
//
// Per frame: the windowed x frame into the LDS image, forward transform, this thread's bins into registers; the same for y
// (never both in one complex transform, as in csd.hip: z = x + i y would put the loud row's rounding error into the quiet row's
// spectrum; skipped when the pair names one channel twice); the recursion, every product and sum rounded on its own (contraction
// off: (a, a) then has Im P == xr xi - xi xr == 0 exactly); the weighted spectrum W / N with its Hermitian half back into the
// image at the bit-reversed positions the inverse passes start from; the inverse transform; the peak over lags -L .. L with the
// first maximum kept (greater value, or equal value and lower lag -- the same rule in a thread's scan, across a wave's lanes with
// __shfl_xor and across the four waves through LDS), a NaN flag reduced next to it; one thread interpolates and stores.
#include "fft_core.hpp"

namespace {

struct tde_args {
    const float *x, *hist, *w;      // x: [channels][x_pitch], hist: [channels][keep], w: [N]
    const int *pair_xy;             // [pairs][2]
    float *state;                   // [pairs][bins][4] = Re S, Im S, Gx, Gy: read when f_lo > 0, written at the end
    float *curve;                   // [pairs][2 L + 1]: the last frame's curve
    float *delay, *peak;            // [pairs][delay_pitch], [pairs][peak_pitch]; peak may be nullptr
    long x_pitch, hops0;            // hops0: hops taken before this call (frame f starts at sample (f - hops0) D of x)
    long f_lo, f_hi;                // the call's frames, counted from the last reset
    long delay_pitch, peak_pitch;
    int N, D, keep, L, weight, k_lo, k_hi;
    float lam, g, delta;
};

struct tde_best {
    float v;
    int lag, nan;
};
// "greater value, or equal value and lower lag"
__device__ __forceinline__ void tde_take(tde_best &a, float v, int lag, int nan)
{
    if (v > a.v || (v == a.v && lag < a.lag)) {
        a.v = v;
        a.lag = lag;
    }
    a.nan |= nan;
}

// one bin of the recursion
__device__ __forceinline__ void tde_update(float (&s)[4], float xr, float xi, float yr, float yi, bool first, float lam, float g)
{
#pragma clang fp contract(off)
    const float p0 = xr * yr, p1 = xi * yi, p2 = xr * yi, p3 = xi * yr;
    const float q0 = xr * xr, q1 = xi * xi, q2 = yr * yr, q3 = yi * yi;
    const float term[4] = {p0 + p1, p2 - p3, q0 + q1, q2 + q3};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (first) {
            s[k] = term[k];                                            // frame 0, or lam == 0: no product by zero
        } else {
            const float a = lam * s[k], b = g * term[k];
            s[k] = a + b;
        }
    }
}

// W of one bin; the denominator 0 gives 0
__device__ __forceinline__ cpx<float> tde_weigh(const float (&s)[4], int weight, float delta)
{
#pragma clang fp contract(off)
    cpx<float> w;
    w.re = s[0];
    w.im = s[1];
    if (weight != 0) {
        const float mag = weight == 1 ? hypotf(s[0], s[1]) : sqrtf(s[2]) * sqrtf(s[3]);
        const float den = mag + delta;
        if (den == 0.f) {
            w.re = 0.f;
            w.im = 0.f;
        } else {
            w.re = s[0] / den;
            w.im = s[1] / den;
        }
    }
    return w;
}

__global__ void __launch_bounds__(FFT_THREADS)
k_tde_staged_f32(tde_args a, const float *__restrict__ cs, int log2n, unsigned groups)
{
    constexpr int MAXB = 4096 / 2 / FFT_THREADS + 1;                   // bins per thread at fft_len 4096: 2049 over 256 lanes
    constexpr int WAVES = FFT_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    const int tid = threadIdx.x, N = a.N, half = N >> 1, bins = half + 1, L = a.L, lags = 2 * L + 1;
    const int tstride = fft_tstride(N);
    cpx<float> *tw = s + tstride;
    tde_best *red = reinterpret_cast<tde_best *>(tw + tw_entries(N));  // [WAVES]
    fft_load_twiddles(tw, cs, N, tid);
    const int pair = blockIdx.x;
    const int cx = a.pair_xy[2 * pair], cy = a.pair_xy[2 * pair + 1];
    float *state = a.state + (size_t)pair * bins * 4;
    float *curve = a.curve + (size_t)pair * lags;
    const float inv_n = 1.0f / (float)N;                               // a power of two: the scaling is exact

    float st[MAXB][4];
#pragma unroll
    for (int m = 0; m < MAXB; m++) {
        const int b = tid + m * FFT_THREADS;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.f_lo > 0 && b < bins) v = *reinterpret_cast<const float4 *>(state + (size_t)b * 4);
        st[m][0] = v.x; st[m][1] = v.y; st[m][2] = v.z; st[m][3] = v.w;
    }
    auto load = [&](int c, long t0) {                                  // the windowed frame of channel c into the image
        const float *row = a.x + (size_t)c * a.x_pitch;
        const float *hrow = a.hist + (size_t)c * a.keep;
        for (int i = tid; i < N; i += FFT_THREADS) {
            const long t = t0 + i;
            cpx<float> z;
            z.re = (t >= 0 ? row[t] : hrow[a.keep + t]) * a.w[i];
            z.im = 0.f;
            s[fft_phys(i)] = z;
        }
        __syncthreads();
        fft_run<arith_f32, false>(s, 1, N, log2n, tstride, tw, groups, tid);
    };
    for (long f = a.f_lo; f < a.f_hi; f++) {
        const long t0 = (f - a.hops0) * a.D;
        cpx<float> X[MAXB], Y[MAXB];
        load(cx, t0);
#pragma unroll
        for (int m = 0; m < MAXB; m++) {                               // position j holds bin brev(j)
            const int b = tid + m * FFT_THREADS;
            if (b < bins) X[m] = s[fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))];
        }
        __syncthreads();                                               // every read of the image is done
        if (cy != cx) {                                                // (the same for the whole workgroup)
            load(cy, t0);
#pragma unroll
            for (int m = 0; m < MAXB; m++) {
                const int b = tid + m * FFT_THREADS;
                if (b < bins) Y[m] = s[fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))];
            }
            __syncthreads();
        }
        // the recursion, and W / N with its Hermitian half into the image: bins 0 .. N/2 from their owners, bin N - k from k's
        const bool first = f == 0 || a.lam == 0.f;
#pragma unroll
        for (int m = 0; m < MAXB; m++) {
            const int b = tid + m * FFT_THREADS;
            if (b < bins) {
                const cpx<float> y = cy != cx ? Y[m] : X[m];
                tde_update(st[m], X[m].re, X[m].im, y.re, y.im, first, a.lam, a.g);
                cpx<float> w;
                w.re = 0.f;
                w.im = 0.f;
                if (b >= a.k_lo && b <= a.k_hi) w = tde_weigh(st[m], a.weight, a.delta);
                w.re *= inv_n;
                w.im *= inv_n;
                if (b == 0 || b == half) w.im = 0.f;                   // the real bins: their imaginary parts are dropped
                s[fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))] = w;
                if (b > 0 && b < half) {
                    w.im = -w.im;
                    s[fft_phys((int)(__brev((unsigned)(N - b)) >> (32 - log2n)))] = w;
                }
            }
        }
        __syncthreads();
        fft_run<arith_f32, true>(s, 1, N, log2n, tstride, tw, groups, tid);      // r[tau] = Re s[tau mod N], barrier behind it
        // the peak over lags -L .. L: a thread's lags in rising order, the first maximum kept
        tde_best best;
        best.v = -__builtin_inff();
        best.lag = 0x7fffffff;
        best.nan = 0;
        const bool last = f + 1 == a.f_hi;
        for (int j = tid; j < lags; j += FFT_THREADS) {
            const int lag = j - L;
            const float r = s[fft_phys(lag & (N - 1))].re;
            tde_take(best, r, lag, r != r);
            if (last) curve[j] = r;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float v = __shfl_xor(best.v, d, 64);
            const int lag = __shfl_xor(best.lag, d, 64), nan = __shfl_xor(best.nan, d, 64);
            tde_take(best, v, lag, nan);
        }
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
#pragma clang fp contract(off)
#pragma unroll
            for (int wv = 1; wv < WAVES; wv++) tde_take(best, red[wv].v, red[wv].lag, red[wv].nan);
            const float nanv = __builtin_nanf("");
            float delay = nanv, peak = nanv;
            if (!best.nan) {
                const float p = s[fft_phys((best.lag - 1) & (N - 1))].re, q = s[fft_phys(best.lag & (N - 1))].re;
                const float r = s[fft_phys((best.lag + 1) & (N - 1))].re;
                const float two_q = 2.f * q, pq = p - two_q, den = pq + r;
                float frac = 0.f;
                if (den < 0.f) {
                    const float num = p - r, h = 0.5f * num;
                    frac = h / den;
                    frac = frac < -0.5f ? -0.5f : (frac > 0.5f ? 0.5f : frac);
                }
                delay = (float)best.lag + frac;
                peak = q;
            }
            a.delay[(size_t)pair * a.delay_pitch + (size_t)(f - a.f_lo)] = delay;
            if (a.peak) a.peak[(size_t)pair * a.peak_pitch + (size_t)(f - a.f_lo)] = peak;
        }
        __syncthreads();                                               // the image and red[] are free for the next frame
    }
#pragma unroll
    for (int m = 0; m < MAXB; m++) {
        const int b = tid + m * FFT_THREADS;
        if (b < bins) *reinterpret_cast<float4 *>(state + (size_t)b * 4) = make_float4(st[m][0], st[m][1], st[m][2], st[m][3]);
    }
}

} // namespace

static int tde_log2(int n)
{
    int k = 0;
    while ((1 << k) < n) k++;
    return (1 << k) == n ? k : -1;
}

extern "C" int llzs_tde_frames_f32(const float *x, const float *hist, const float *w, const float *cs, const int *pair_xy,
                                   float *state, float *curve, float *delay, float *peak, int pairs, int fft_len, int hop,
                                   long x_pitch, long hops0, long f_lo, long f_hi, long delay_pitch, long peak_pitch, int max_lag, int weight,
                                   int k_lo, int k_hi, float lam, float g, float delta, void *stream)
{
    const int log2n = tde_log2(fft_len);
    if (!x || !w || !cs || !pair_xy || !state || !curve || !delay || pairs < 1 || log2n < 6 || log2n > 12 ||
        (hop != fft_len && 2 * hop != fft_len && 4 * hop != fft_len) || (hop != fft_len && !hist) ||
        f_lo < 0 || f_hi <= f_lo || delay_pitch < f_hi - f_lo || (peak && peak_pitch < f_hi - f_lo) || f_lo < hops0 - (fft_len / hop - 1) ||
        (f_hi - 1 - hops0) * hop + fft_len > x_pitch || max_lag < 1 || max_lag > fft_len / 2 - 1 || weight < 0 || weight > 2 ||
        k_lo < 0 || k_hi < k_lo || k_hi > fft_len / 2 || !(lam >= 0.f && lam < 1.f) || !(delta >= 0.f)) {
        llzs_set_error("tde_frames_f32: bad arguments (pairs %d fft_len %d hop %d frames %ld..%ld pitches %ld, %ld max_lag %d "
                       "weight %d bins %d..%d)", pairs, fft_len, hop, f_lo, f_hi, delay_pitch, peak_pitch, max_lag, weight, k_lo, k_hi);
        return LLZ_ERR_ARG;
    }
    tde_args a;
    a.x = x; a.hist = hist; a.w = w; a.pair_xy = pair_xy; a.state = state; a.curve = curve; a.delay = delay; a.peak = peak;
    a.x_pitch = x_pitch; a.hops0 = hops0; a.f_lo = f_lo; a.f_hi = f_hi; a.delay_pitch = delay_pitch; a.peak_pitch = peak_pitch;
    a.N = fft_len; a.D = hop; a.keep = fft_len - hop; a.L = max_lag; a.weight = weight; a.k_lo = k_lo; a.k_hi = k_hi;
    a.lam = lam; a.g = g; a.delta = delta;
    // one image, the twiddle table and the four waves' partial peaks: 50 KB at 4096
    const fft_plan pl = fft_make_plan<arith_f32>(fft_len, 1, (FFT_THREADS / 64) * sizeof(tde_best));
    hipLaunchKernelGGL(k_tde_staged_f32, dim3((unsigned)pairs), dim3(FFT_THREADS), pl.lds, as_stream(stream), a, cs, log2n,
                       fft_groups(log2n));
    LLZ_LAUNCH_CHECK("k_tde_staged_f32");
    return LLZ_OK;
}
