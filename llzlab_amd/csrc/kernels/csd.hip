// csd.hip -- Welch cross-spectra of many channel pairs (include/llz_spectral.h, host layer llz_spectral_host.c), float32
// transforms, fft_len 64..4096, hop fft_len, fft_len / 2 or fft_len / 4.
//
//   k_csd_reg_f32<E, TWO>   fft_len 256 (E = 16), 512 (2 x 16^2, TWO), 1024 (E = 32): a group of E lanes per (pair, run) on
//                           square_core (fft_square.hpp), windowed samples from HBM straight into the registers of the lane
//                           that transforms them, as k_stft_analysis_reg_f32 does
//   k_csd_staged_f32        any fft_len on the staged passes of fft_core.hpp, a workgroup per (pair, run): 64, 128, 2048, 4096,
//                           and every size under the fft_generic tune
//                           (2048 = 2 x 32^2 does not fit the register file with the sums of a run and their compensation
//                           terms: on groups of 32 lanes the compiler's report showed 780 to 1500 bytes of scratch per lane,
//                           on a whole wave with a 32 x 32 transform per half-wave 360 bytes: that size is staged)
//   k_csd_fold_f64          finished float32 run partials into the double accumulators, in run order
//   k_csd_read_f64          the read-outs, in double from accumulators + the carried partial, rounded once
//
// A work item is (pair, run): run r = frames [32 r, 32 r + 32) of the stream counted from the last reset, of which the call
// holds [f_lo, f_hi).  The item walks its frames in order; for each it transforms the x frame, keeps the bins it owns in
// registers, transforms the y frame (never both in one complex transform: z = x + i y would put the loud row's rounding error
// into the quiet row's spectrum) and adds |X|^2, |Y|^2, conj(X) Y into float32 accumulators that stay in registers for the run.
// A run that began in an earlier call starts from the handle's carried partial (carry_in); a run the call does not finish
// goes to carry_out, both with the compensation terms of its sums (csd_add) -- two buffers, because one launch may hold the
// item that continues the open run and the item that leaves a later run open, and nothing orders the items of a launch; a
// finished run's sums go to the scratch slot (run - r0, pair) for the fold.  Products and sums are separately rounded
// (contraction off): (a, a) then has Sxy == Sxx and an imaginary part of exactly 0, and (b, a) is the exact conjugate of (a, b).
#include "fft_square.hpp"

namespace {

constexpr int CSD_RUN = 32;

struct csd_args {
    const float *x, *hist, *w;      // x: [channels][x_pitch], hist: [channels][keep], w: [N]
    const int *pair_xy;             // [pairs][2]
    float *scratch;                 // [runs of the walk][pairs][bins][4]
    const float *carry_in;          // [2][pairs][bins][4]: the run that was open before the call: its sums, then their
    float *carry_out;               // compensation terms; and where the run the call leaves open goes: another buffer
    long x_pitch, hops0;            // hops0: hops taken before this call (frame f starts at sample (f - hops0) D of x)
    long f_lo, f_hi, r0;            // the call's frames, the walk's first run
    int N, D, keep, pairs;
};

// Sxx, Syy, Re Sxy, Im Sxy of one bin of one frame onto a[0..3], every product and sum rounded on its own.  The run's sums are
// COMPENSATED float32 sums in frame order (Kahan: a[4..7] holds what the additions so far lost): a plain 32-term float32 sum is
// off by several u, independently in Sxx, Syy and Sxy, and a coherent pair (two tones) then read a coherence of up to 1 + 12 u;
// compensated, a run's sum is within about 1 u of the exact sum of its terms and the coherence stays within 1 + 2 u.  Every
// step commutes with a power of two and with a change of sign, so the exact ties hold as for plain sums.
__device__ __forceinline__ void csd_add(float (&a)[8], float xr, float xi, float yr, float yi)
{
#pragma clang fp contract(off)
    const float p0 = xr * xr, p1 = xi * xi, p2 = yr * yr, p3 = yi * yi;
    const float p4 = xr * yr, p5 = xi * yi, p6 = xr * yi, p7 = xi * yr;
    const float term[4] = {p0 + p1, p2 + p3, p4 + p5, p6 - p7};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float y = term[k] - a[4 + k];
        const float t = a[k] + y;
        a[4 + k] = (t - a[k]) - y;
        a[k] = t;
    }
}

// a partial's sums from s (and its compensation terms from c, where the partial is an open run's: c != nullptr) and back
__device__ __forceinline__ void csd_load(float (&a)[8], bool from, const float *s, const float *c)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = v;
    if (from) {
        v = *reinterpret_cast<const float4 *>(s);
        w = *reinterpret_cast<const float4 *>(c);
    }
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    a[4] = w.x; a[5] = w.y; a[6] = w.z; a[7] = w.w;
}
__device__ __forceinline__ void csd_store(const float (&a)[8], float *s, float *c)
{
    *reinterpret_cast<float4 *>(s) = make_float4(a[0], a[1], a[2], a[3]);
    if (c) *reinterpret_cast<float4 *>(c) = make_float4(a[4], a[5], a[6], a[7]);
}

// where the item's partial starts and ends: the frames [fa, fb) of its run inside the call, the carried partial in front
// (cont) and the destination behind
struct csd_item {
    long fa, fb;
    bool cont;
    const float *src, *src_c;        // the carried partial and its compensation terms (read when cont)
    float *dst, *dst_c;              // dst_c: nullptr for a finished run (its compensation terms end with it)
    int cx, cy;
};
__device__ __forceinline__ csd_item csd_make_item(const csd_args &a, long item, int bins)
{
    const int run_local = (int)(item / a.pairs), pair = (int)(item - (long)run_local * a.pairs);
    const long run = a.r0 + run_local, f0 = run * CSD_RUN;
    csd_item it;
    it.fa = f0 > a.f_lo ? f0 : a.f_lo;
    it.fb = f0 + CSD_RUN < a.f_hi ? f0 + CSD_RUN : a.f_hi;
    it.cont = f0 < a.f_lo;
    const bool finished = f0 + CSD_RUN <= a.f_hi;
    // (the item that continues the open run and the item that leaves a later run open may be in one launch, unordered: they
    //  read and write different buffers)
    const size_t cell = (size_t)pair * bins * 4, comp = (size_t)a.pairs * bins * 4;
    it.src = a.carry_in + cell;
    it.src_c = a.carry_in + comp + cell;
    it.dst = finished ? a.scratch + ((size_t)run_local * a.pairs + pair) * bins * 4 : a.carry_out + cell;
    it.dst_c = finished ? nullptr : a.carry_out + comp + cell;
    it.cx = a.pair_xy[2 * pair];
    it.cy = a.pair_xy[2 * pair + 1];
    return it;
}

// ---- the staged form: a workgroup per item, one transform image in LDS; X's bins wait in registers while Y is transformed
__global__ void __launch_bounds__(FFT_THREADS)
k_csd_staged_f32(csd_args a, const float *__restrict__ cs, int log2n, unsigned groups)
{
    constexpr int MAXB = 4096 / 2 / FFT_THREADS + 1;                   // bins per thread at fft_len 4096: 2049 over 256 lanes
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    const int tid = threadIdx.x, N = a.N, bins = (N >> 1) + 1;
    const int tstride = fft_tstride(N);
    cpx<float> *tw = s + tstride;
    fft_load_twiddles(tw, cs, N, tid);
    const csd_item it = csd_make_item(a, blockIdx.x, bins);
    float acc[MAXB][8];
#pragma unroll
    for (int m = 0; m < MAXB; m++) {
        const int b = tid + m * FFT_THREADS;
        csd_load(acc[m], it.cont && b < bins, it.src + (size_t)b * 4, it.src_c + (size_t)b * 4);
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
    for (long f = it.fa; f < it.fb; f++) {
        const long t0 = (f - a.hops0) * a.D;
        cpx<float> X[MAXB], Y[MAXB];
        load(it.cx, t0);
#pragma unroll
        for (int m = 0; m < MAXB; m++) {                               // position j holds bin brev(j)
            const int b = tid + m * FFT_THREADS;
            if (b < bins) X[m] = s[fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))];
        }
        if (it.cy != it.cx) {                                          // (the same for the whole workgroup)
            __syncthreads();
            load(it.cy, t0);
#pragma unroll
            for (int m = 0; m < MAXB; m++) {
                const int b = tid + m * FFT_THREADS;
                if (b < bins) Y[m] = s[fft_phys((int)(__brev((unsigned)b) >> (32 - log2n)))];
            }
        }
#pragma unroll
        for (int m = 0; m < MAXB; m++) {
            const int b = tid + m * FFT_THREADS;
            if (b < bins) {
                const cpx<float> y = it.cy != it.cx ? Y[m] : X[m];
                csd_add(acc[m], X[m].re, X[m].im, y.re, y.im);
            }
        }
        __syncthreads();                                               // every read of the image is done
    }
#pragma unroll
    for (int m = 0; m < MAXB; m++) {
        const int b = tid + m * FFT_THREADS;
        if (b < bins) csd_store(acc[m], it.dst + (size_t)b * 4, it.dst_c ? it.dst_c + (size_t)b * 4 : nullptr);
    }
}

// ---- the register form.  Of the E (2 E with TWO) values a lane holds after the transform, those with a bin in 0 .. N/2 are
// kept: slot j < E/2 = register 2 j (bin lg + E brevE(2 j)), and register 1 (bin N/2 in lane 0 only) in the last slot; with TWO
// the even bin 2 k of s and the odd bin 2 k + 1 of d side by side, and s's register 1 (bin N/2 in lane 0) last.
template <int E, bool TWO>
struct csd_geom {
    static constexpr int H = E * E, N = TWO ? 2 * H : H, BINS = N / 2 + 1, NK = TWO ? E + 1 : E / 2 + 1;
    static __device__ __forceinline__ int bin(int slot, int lg)        // the last slot: lane 0 only
    {
        if (!TWO) return slot < E / 2 ? lg + E * brevE<E>(2 * slot) : H / 2;
        return slot < E ? 2 * (lg + E * brevE<E>(2 * (slot >> 1))) + (slot & 1) : H;
    }
};

template <int E, bool TWO, int NK, typename Sample>
__device__ __forceinline__ void csd_transform(cf (&out)[NK], Sample sample, float *buf, const float2 *__restrict__ tw2d,
                                              const float2 *__restrict__ tw1, int lg)
{
    static_assert(NK == csd_geom<E, TWO>::NK, "one slot per kept value");
    constexpr int H = E * E;
    if constexpr (!TWO) {
        cf v[E];
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = cf{sample(lg + E * j), 0.f};
        square_core<E, false>(v, buf, tw2d, lg);                       // v[q] = X[lg + E brevE(q)]
#pragma unroll
        for (int j = 0; j < E / 2; j++) out[j] = v[2 * j];
        out[E / 2] = v[1];
    } else {
        cf s[E], d[E];
#pragma unroll
        for (int j = 0; j < E; j++) {                                  // real input: s, d before the twist are real
            const float p = sample(lg + E * j), q = sample(lg + E * j + H);
            const float2 t = tw1[j * E + lg];
            s[j] = cf{p + q, 0.f};
            d[j] = cf{(p - q) * t.x, (p - q) * t.y};
        }
        square_core<E, false>(s, buf, tw2d, lg);                       // s[q] = X[2 kq], d[q] = X[2 kq + 1], kq = lg + E brevE(q)
        square_core<E, false>(d, buf, tw2d, lg);
#pragma unroll
        for (int j = 0; j < E / 2; j++) {
            out[2 * j] = s[2 * j];
            out[2 * j + 1] = d[2 * j];
        }
        out[E] = s[1];
    }
}

template <int E, bool TWO>
__global__ void __launch_bounds__(256)
k_csd_reg_f32(csd_args a, const float2 *__restrict__ tw2d, const float2 *__restrict__ tw1, long items)
{
    typedef csd_geom<E, TWO> G;
    constexpr int GROUPS = 256 / E, PITCH = E + 1, NK = G::NK;
    __shared__ float bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    const bool last = lg == 0;                                         // the lane that owns bin N/2
    const long item = (long)blockIdx.x * GROUPS + grp;
    if (item >= items) return;                                         // (no workgroup barrier below: lane groups are on their own)
    const csd_item it = csd_make_item(a, item, G::BINS);
    float *buf = bufs[grp];
    float acc[NK][8];
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const size_t o = (size_t)G::bin(k, lg) * 4;
        csd_load(acc[k], it.cont && (k < NK - 1 || last), it.src + o, it.src_c + o);
    }
    const float *xrow = a.x + (size_t)it.cx * a.x_pitch, *xh = a.hist + (size_t)it.cx * a.keep;
    const float *yrow = a.x + (size_t)it.cy * a.x_pitch, *yh = a.hist + (size_t)it.cy * a.keep;
    for (long f = it.fa; f < it.fb; f++) {
        const long t0 = (f - a.hops0) * a.D;
        cf X[NK];
        csd_transform<E, TWO>(X, [&](int i) {
            const long t = t0 + i;
            return (t >= 0 ? xrow[t] : xh[a.keep + t]) * a.w[i];
        }, buf, tw2d, tw1, lg);
        if (it.cy != it.cx) {
            cf Y[NK];
            csd_transform<E, TWO>(Y, [&](int i) {
                const long t = t0 + i;
                return (t >= 0 ? yrow[t] : yh[a.keep + t]) * a.w[i];
            }, buf, tw2d, tw1, lg);
#pragma unroll
            for (int k = 0; k < NK; k++) csd_add(acc[k], X[k].x, X[k].y, Y[k].x, Y[k].y);
        } else {
#pragma unroll
            for (int k = 0; k < NK; k++) csd_add(acc[k], X[k].x, X[k].y, X[k].x, X[k].y);
        }
    }
#pragma unroll
    for (int k = 0; k < NK; k++)
        if (k < NK - 1 || last) {
            const size_t o = (size_t)G::bin(k, lg) * 4;
            csd_store(acc[k], it.dst + o, it.dst_c ? it.dst_c + o : nullptr);
        }
}

// acc[i] += the partials of the walk's nfin finished runs, in run order; i over [pairs][bins][4]
__global__ void __launch_bounds__(256)
k_csd_fold_f64(const float *__restrict__ scratch, double *__restrict__ acc, long per, int nfin)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    double v = acc[i];
    for (int r = 0; r < nfin; r++) v += (double)scratch[(size_t)r * per + i];
    acc[i] = v;
}

// what: LLZ_SPEC_PXX .. LLZ_SPEC_TF of llz_spectral.h, 5 = the raw sums (double)
__global__ void __launch_bounds__(256)
k_csd_read_f64(const double *__restrict__ acc, const float *__restrict__ carry, long cells, int what, double ku,
               float *__restrict__ out, double *__restrict__ raw)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = acc[(size_t)i * 4 + k] + (carry ? (double)carry[(size_t)i * 4 + k] : 0.0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    switch (what) {
    case 0: out[i] = (float)(s[0] / ku); break;
    case 1: out[i] = (float)(s[1] / ku); break;
    case 2:
        out[(size_t)i * 2] = (float)(s[2] / ku);
        out[(size_t)i * 2 + 1] = (float)(s[3] / ku);
        break;
    case 3: {
        const double den = s[0] * s[1];
        out[i] = (float)(den == 0.0 ? nan : (s[2] * s[2] + s[3] * s[3]) / den);
        break;
    }
    case 4:
        out[(size_t)i * 2] = (float)(s[0] == 0.0 ? nan : s[2] / s[0]);
        out[(size_t)i * 2 + 1] = (float)(s[0] == 0.0 ? nan : s[3] / s[0]);
        break;
    default:
#pragma unroll
        for (int k = 0; k < 4; k++) raw[(size_t)i * 4 + k] = s[k];
        break;
    }
}

} // namespace

static int csd_log2(int n)
{
    int k = 0;
    while ((1 << k) < n) k++;
    return (1 << k) == n ? k : -1;
}

extern "C" int llzs_csd_form(int fft_len)
{
    const bool reg = fft_len == 256 || fft_len == 512 || fft_len == 1024;
    return reg && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1 ? 1 : 0;
}

extern "C" int llzs_csd_runs_f32(const float *x, const float *hist, const float *w, const float *cs, const int *pair_xy,
                                 float *scratch, const float *carry_in, float *carry_out, int pairs, int fft_len, int hop,
                                 long x_pitch, long hops0,
                                 long f_lo, long f_hi, long r0, int nruns, void *stream)
{
    const int log2n = csd_log2(fft_len);
    if (!x || !w || !cs || !pair_xy || !scratch || !carry_in || !carry_out || carry_in == carry_out || pairs < 1 ||
        log2n < 6 || log2n > 12 ||
        (hop != fft_len && 2 * hop != fft_len && 4 * hop != fft_len) || (hop != fft_len && !hist) || nruns < 1 ||
        f_lo < 0 || f_hi <= f_lo || r0 * CSD_RUN >= f_hi || (r0 + 1) * CSD_RUN <= f_lo ||
        (r0 + nruns - 1) * CSD_RUN >= f_hi || f_lo < hops0 - (fft_len / hop - 1) ||
        (f_hi - 1 - hops0) * hop + fft_len > x_pitch || (long)pairs * nruns > 0x7fffffffL) {
        llzs_set_error("csd_runs_f32: bad arguments (pairs %d fft_len %d hop %d frames %ld..%ld runs %ld+%d)", pairs, fft_len,
                       hop, f_lo, f_hi, r0, nruns);
        return LLZ_ERR_ARG;
    }
    csd_args a;
    a.x = x; a.hist = hist; a.w = w; a.pair_xy = pair_xy; a.scratch = scratch; a.carry_in = carry_in; a.carry_out = carry_out;
    a.x_pitch = x_pitch; a.hops0 = hops0; a.f_lo = f_lo; a.f_hi = f_hi; a.r0 = r0;
    a.N = fft_len; a.D = hop; a.keep = fft_len - hop; a.pairs = pairs;
    const long items = (long)pairs * nruns;
    if (llzs_csd_form(fft_len)) {
        const int E = fft_len == 1024 ? 32 : 16;
        const bool two = fft_len == 512;
        const float2 *tw2d = nullptr, *tw1 = nullptr;
        const int trc = fft_derived_tables(7, fft_len, E, two ? 2 : 1, two, cs, stream, "csd twiddle tables", &tw2d, &tw1);
        if (trc != LLZ_OK) return trc;
        const unsigned blocks = (unsigned)((items + (256 / E) - 1) / (256 / E));
        if (fft_len == 256)
            hipLaunchKernelGGL((k_csd_reg_f32<16, false>), dim3(blocks), dim3(256), 0, as_stream(stream), a, tw2d, tw1, items);
        else if (fft_len == 512)
            hipLaunchKernelGGL((k_csd_reg_f32<16, true>), dim3(blocks), dim3(256), 0, as_stream(stream), a, tw2d, tw1, items);
        else
            hipLaunchKernelGGL((k_csd_reg_f32<32, false>), dim3(blocks), dim3(256), 0, as_stream(stream), a, tw2d, tw1, items);
        LLZ_LAUNCH_CHECK("k_csd_reg_f32");
        return LLZ_OK;
    }
    const fft_plan pl = fft_make_plan<arith_f32>(fft_len, 1);          // one image and the twiddle table: 50 KB at 4096
    hipLaunchKernelGGL(k_csd_staged_f32, dim3((unsigned)items), dim3(FFT_THREADS), pl.lds, as_stream(stream), a, cs, log2n,
                       fft_groups(log2n));
    LLZ_LAUNCH_CHECK("k_csd_staged_f32");
    return LLZ_OK;
}

extern "C" int llzs_csd_fold_f64(const float *scratch, double *acc, int pairs, int bins, int nfin, void *stream)
{
    if (!scratch || !acc || pairs < 1 || bins < 1 || nfin < 1) {
        llzs_set_error("csd_fold_f64: bad arguments");
        return LLZ_ERR_ARG;
    }
    const long per = (long)pairs * bins * 4;
    hipLaunchKernelGGL(k_csd_fold_f64, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, as_stream(stream), scratch, acc, per,
                       nfin);
    LLZ_LAUNCH_CHECK("k_csd_fold_f64");
    return LLZ_OK;
}

extern "C" int llzs_csd_read_f64(const double *acc, const float *carry, int pairs, int bins, int what, double ku, float *out,
                                 double *raw, void *stream)
{
    if (!acc || pairs < 1 || bins < 1 || what < 0 || what > 5 || (what == 5 ? !raw : !out) || !(ku > 0.0)) {
        llzs_set_error("csd_read_f64: bad arguments");
        return LLZ_ERR_ARG;
    }
    const long cells = (long)pairs * bins;
    hipLaunchKernelGGL(k_csd_read_f64, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, as_stream(stream), acc, carry, cells,
                       what, ku, out, raw);
    LLZ_LAUNCH_CHECK("k_csd_read_f64");
    return LLZ_OK;
}
