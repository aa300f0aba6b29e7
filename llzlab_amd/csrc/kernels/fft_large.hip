// fft_large.hip -- radix-2 transforms above 4096 points: llz_fft / llz_ifft (double, bit-identical to the reference) up to
// 2^24 points and the float32 batch from 8192 up to 2^24 points.  Same dataflow as fft.hip (reference
// libllzfilter/llz_fft.c:61-198); only the grouping of butterflies into memory passes differs.
//
// Let N = 2^n and B = 2^b the largest transform a flavour holds in one workgroup's LDS (FLAVOURS below).
//   n <= b (float32 8192, 16384): one launch per transform, the whole transform in LDS (k_fft_block, FULL).
//   n >  b, forward: the first n - b DIF stages (half-spans N/2 .. B) pair elements more than B apart: they run as outer
//            passes over HBM in place (k_fft_outer, up to four stages fused in registers per pass).  The remaining b stages
//            are independent B-point DIF transforms of contiguous blocks with twiddle index q * (N / span): the N table
//            sampled at stride N/B, which for powers of two is bit for bit the B table (2 pi i and / size scale exactly).
//            Last, the bit reversal as an in-place swap of tile pairs (k_fft_bitrev: rev_N is an involution).
//   n >  b, inverse: the mirror image -- the swap pass with the division by N of llz_fft.c:187-195, the DIT blocks in LDS,
//            then the outer DIT passes for half-spans B .. N/2.
// Every double butterfly is the reference's butterfly on the reference's operands with its table entry (arith_f64,
// contraction off), so llz_fft / llz_ifft stay exact.  The float32 flavour uses the factored passes of fft_core.hpp.
#include "fft_core.hpp"

namespace {

// ---- outer pass: G stages over HBM, in place.  Item `it` of transform tr holds the E = 2^G elements
// blk * (E * step) + j * step + r; lanes take consecutive r, so every one of the E loads is one coalesced run per wave.
template <typename A, int G, bool INV>
__global__ void __launch_bounds__(256)
k_fft_outer(typename A::data_t *__restrict__ data, size_t items, int log2n, int log2step,
            const typename A::tw_t *__restrict__ cs /* N cos, then N sin */)
{
    typedef typename A::data_t T;
    typedef typename A::tw_t W;
    constexpr int E = 1 << G;
    const int N = 1 << log2n, log2items = log2n - G, step = 1 << log2step;
    cpx<T> *g = reinterpret_cast<cpx<T> *>(data);
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t tr = it >> log2items;
        const int rem = (int)(it & (((size_t)1 << log2items) - 1));
        const int r = rem & (step - 1), blk = rem >> log2step;
        cpx<T> *base = g + (tr << log2n) + ((size_t)blk << (G + log2step)) + r;
        cpx<T> v[E];
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = base[(size_t)j << log2step];
        if constexpr (std::is_same<A, arith_f32>::value) {
            // fft_pass_f32's factored form; k * m < N, so the full N table needs no half-turn wrap
            const int m = r << (log2n - G - log2step);
            auto twiddle = [&](int p) {
                const int idx = (int)(__brev((unsigned)p) >> (32 - G)) * m;
                const float c = cs[idx], sn = cs[N + idx];
                const float wi = INV ? sn : -sn;
                const cpx<float> d = v[p];
                v[p].re = __builtin_fmaf(d.re, c, -(d.im * wi));
                v[p].im = __builtin_fmaf(d.re, wi, d.im * c);
            };
            if (INV) {
#pragma unroll
                for (int p = 1; p < E; p++) twiddle(p);
            }
            small_fft<E, INV>(v, std::make_integer_sequence<int, G>{});
            if (!INV) {
#pragma unroll
                for (int p = 1; p < E; p++) twiddle(p);
            }
        } else {
            // fft_pass's butterflies, table entries read from memory
#pragma unroll
            for (int gq = 0; gq < G; gq++) {
                const int hj = INV ? (1 << gq) : (E >> (gq + 1));
                const int log2hj = INV ? gq : (G - 1 - gq);
                const int tshift = (log2n - 1) - (log2step + log2hj);
#pragma unroll
                for (int j = 0; j < E; j++) {
                    if (j & hj) continue;
                    const int idx = (((j & (hj - 1)) << log2step) + r) << tshift;
                    const W wr = cs[idx], ws = cs[N + idx];
                    const cpx<T> u = v[j], w = v[j + hj];
                    if (!INV) {
                        cpx<T> x, y;
                        x.re = A::add(u.re, w.re); x.im = A::add(u.im, w.im);
                        A::rot(A::sub(u.re, w.re), A::sub(u.im, w.im), wr, A::neg(ws), y.re, y.im);
                        v[j] = x; v[j + hj] = y;
                    } else {
                        T dr, di;
                        A::rot(w.re, w.im, wr, ws, dr, di);
                        cpx<T> x, y;
                        x.re = A::add(u.re, dr); x.im = A::add(u.im, di);
                        y.re = A::sub(u.re, dr); y.im = A::sub(u.im, di);
                        v[j] = x; v[j + hj] = y;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < E; j++) base[(size_t)j << log2step] = v[j];
    }
}

template <typename A, int G, bool INV, int NT>
__device__ __forceinline__ void lds_pass(cpx<typename A::data_t> *s, int size, int log2n, int log2step, int tstride,
                                         const cpx<typename A::tw_t> *tw, int tid)
{
    if constexpr (std::is_same<A, arith_f32>::value) {
        fft_pass_f32<G, INV, NT>(s, 1, size, log2n, log2step, tstride, tw, tid);
    } else {
        static_assert(NT == FFT_THREADS, "the exact passes stride by FFT_THREADS");
        fft_pass<A, G, INV>(s, 1, size, log2n, log2step, tstride, tw, tid);
    }
}

// ---- B-point transforms of contiguous blocks in LDS, one block per workgroup at a time (grid-stride over nblk blocks).
// FULL: the block is the whole transform -- the inverse loads through the bit reversal dividing by N, the forward stores
// through it (done on the LDS side, so both HBM directions stay coalesced).  Otherwise natural order in and out.
// TWL: the half-turn table goes into LDS, sampled from the N table cs at stride N/B; else twg is that table, padded
// (tw_phys), in memory: the float32 flavour, where at 16384 points the data alone fill 135 KB of LDS and at 8192 points
// the table would keep a second workgroup off the CU.
template <typename A, bool INV, int NT, bool FULL, bool TWL>
__global__ void __launch_bounds__(NT)
k_fft_block(typename A::data_t *__restrict__ data, size_t nblk, int log2b, int log2n,
            const typename A::tw_t *__restrict__ cs, const cpx<typename A::tw_t> *__restrict__ twg, unsigned groups)
{
    typedef typename A::data_t T;
    typedef typename A::tw_t W;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<T> *s = reinterpret_cast<cpx<T> *>(smem_raw);
    const int tid = threadIdx.x, B = 1 << log2b, N = 1 << log2n;
    const int tstride = fft_phys(B) + 1;
    const cpx<W> *tw = twg;
    if (TWL) {
        cpx<W> *twl = reinterpret_cast<cpx<W> *>(s + tstride);
        const int sh = log2n - log2b;
        for (int e = tid; e < (B >> 1); e += NT) {
            cpx<W> t;
            t.re = cs[e << sh];
            t.im = cs[N + (e << sh)];
            twl[tw_phys(e)] = t;
        }
        tw = twl;                                          // published by the barrier after the first load
    }
    cpx<T> *g0 = reinterpret_cast<cpx<T> *>(data);
    for (size_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        cpx<T> *g = g0 + (b << log2b);
        for (int i = tid; i < B; i += NT) {
            cpx<T> v = g[i];
            int at = i;
            if (FULL && INV) {
                at = (int)(__brev((unsigned)i) >> (32 - log2b));
                v.re = A::scale_in(v.re, B, log2b);
                v.im = A::scale_in(v.im, B, log2b);
            }
            s[fft_phys(at)] = v;
        }
        __syncthreads();
        int done = 0;
#pragma unroll 1
        for (int p = 0; p < 4; p++) {
            const int G = (groups >> (4 * p)) & 15;
            if (G == 0) break;
            const int log2step = INV ? done : (log2b - done - G);
            switch (G) {
            case 1: lds_pass<A, 1, INV, NT>(s, B, log2b, log2step, tstride, tw, tid); break;
            case 2: lds_pass<A, 2, INV, NT>(s, B, log2b, log2step, tstride, tw, tid); break;
            case 3: lds_pass<A, 3, INV, NT>(s, B, log2b, log2step, tstride, tw, tid); break;
            default: lds_pass<A, 4, INV, NT>(s, B, log2b, log2step, tstride, tw, tid); break;
            }
            done += G;
        }
        for (int i = tid; i < B; i += NT) {
            const int at = (FULL && !INV) ? (int)(__brev((unsigned)i) >> (32 - log2b)) : i;
            g[i] = s[fft_phys(at)];
        }
        __syncthreads();                                   // every read of s done before the next block's loads
    }
}

// ---- bit reversal of N = 2^n points (n >= 10) in place, optionally dividing by N (the inverse's gather, llz_fft.c:187-195).
// Index i = (a, m, c): a the top five bits, c the bottom five, m the n - 10 bits between; rev_N(a, m, c) =
// (rev5(c), rev(m), rev5(a)).  Tile m (1024 points, 32 runs of 32) and tile rev(m) swap through LDS; the workgroup of the
// smaller index does both, a tile with m = rev(m) is permuted on its own.  Every point is read once and written once.
template <typename A, bool SCALE>
__global__ void __launch_bounds__(256)
k_fft_bitrev(typename A::data_t *__restrict__ data, size_t tiles, int log2n)
{
    typedef typename A::data_t T;
    __shared__ cpx<T> ta[32][33], tb[32][33];
    const int tid = threadIdx.x, mbits = log2n - 10, N = 1 << log2n;
    cpx<T> *g0 = reinterpret_cast<cpx<T> *>(data);
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t tr = t >> mbits;
        const int m = (int)(t & (((size_t)1 << mbits) - 1));
        const int mr = mbits ? (int)(__brev((unsigned)m) >> (32 - mbits)) : 0;
        if (mr < m) continue;                              // uniform over the workgroup
        cpx<T> *g = g0 + (tr << log2n);
        const size_t om = (size_t)m << 5, omr = (size_t)mr << 5;
        for (int e = tid; e < 1024; e += 256) {
            const int a = e >> 5, c = e & 31;
            const size_t row = (size_t)a << (log2n - 5);
            ta[a][c] = g[row + om + c];
            if (mr != m) tb[a][c] = g[row + omr + c];
        }
        __syncthreads();
        for (int e = tid; e < 1024; e += 256) {
            const int a = e >> 5, c = e & 31;
            const int ra = (int)(__brev((unsigned)a) >> 27), rc = (int)(__brev((unsigned)c) >> 27);
            const size_t row = (size_t)a << (log2n - 5);
            cpx<T> v = mr != m ? tb[rc][ra] : ta[rc][ra];
            if (SCALE) { v.re = A::scale_in(v.re, N, log2n); v.im = A::scale_in(v.im, N, log2n); }
            g[row + om + c] = v;
            if (mr != m) {
                cpx<T> u = ta[rc][ra];
                if (SCALE) { u.re = A::scale_in(u.re, N, log2n); u.im = A::scale_in(u.im, N, log2n); }
                g[row + omr + c] = u;
            }
        }
        __syncthreads();
    }
}

// the half-turn table of B points in tw_phys layout, in memory, sampled from the N table cs (float32, B = 16384); the pad
// slots are never read
__global__ void k_fft_large_twb(cpx<float> *__restrict__ twb, const float *__restrict__ cs, int log2b, int log2n)
{
    const int i = blockIdx.x * 256 + threadIdx.x, N = 1 << log2n, sh = log2n - log2b;
    if (i >= (1 << (log2b - 1))) return;
    cpx<float> t;
    t.re = cs[i << sh];
    t.im = cs[N + (i << sh)];
    twb[tw_phys(i)] = t;
}

// ---- plan: flavour -> largest LDS block, its workgroup shape; N -> outer stage groups and passes over HBM.
struct fft_flavour {
    int max_log2b;      // largest transform held in one workgroup's LDS
    int max_g;          // stages per outer pass (registers per item: 2^max_g complex values)
};
constexpr fft_flavour FLAVOURS[2] = {
    {12, 4},            // double: 4096 points, 101 KB of LDS with the table (k_fft_radix2's layout)
    {14, 4},            // float32: 16384 points, 135 KB of LDS, table in memory
};

struct fft_large_plan {
    int log2n, log2b;
    int outer;          // outer passes over HBM
    int g[8];           // stages of each outer pass, in forward order
    unsigned groups;    // the LDS block's passes (fft_groups)
    int passes;         // passes over HBM in all: outer + block + bit reversal
};

static fft_large_plan fft_large_plan_of(int f32, int log2n)
{
    const fft_flavour fl = FLAVOURS[f32 ? 1 : 0];
    fft_large_plan p = {};
    p.log2n = log2n;
    p.log2b = log2n < fl.max_log2b ? log2n : fl.max_log2b;
    const int left = log2n - p.log2b;
    p.outer = (left + fl.max_g - 1) / fl.max_g;
    for (int q = 0, l = left; q < p.outer; q++) {
        p.g[q] = (l + (p.outer - q) - 1) / (p.outer - q);
        l -= p.g[q];
    }
    p.groups = fft_groups(p.log2b);
    p.passes = p.outer + 1 + (p.outer ? 1 : 0);
    return p;
}

static unsigned grid_of(size_t units)
{
    const size_t cap = (size_t)1 << 20;                     // grid-stride loops take the rest
    return (unsigned)(units < cap ? (units ? units : 1) : cap);
}

template <typename A, int G>
static void launch_outer(typename A::data_t *data, size_t count, int log2n, int log2step, const typename A::tw_t *cs,
                         int inverse, hipStream_t st)
{
    const size_t items = count << (log2n - G);
    const unsigned grid = grid_of((items + 255) / 256);
    if (inverse) hipLaunchKernelGGL((k_fft_outer<A, G, true>), dim3(grid), dim3(256), 0, st, data, items, log2n, log2step, cs);
    else hipLaunchKernelGGL((k_fft_outer<A, G, false>), dim3(grid), dim3(256), 0, st, data, items, log2n, log2step, cs);
}

template <typename A, int NT, bool FULL, bool TWL>
static int launch_block(typename A::data_t *data, size_t nblk, const fft_large_plan &p, const typename A::tw_t *cs,
                        const cpx<typename A::tw_t> *twg, int inverse, hipStream_t st)
{
    const int B = 1 << p.log2b;
    const size_t lds = ((size_t)(B + (B >> 5)) + 1) * sizeof(cpx<typename A::data_t>) +
                       (TWL ? (size_t)tw_entries(B) * sizeof(cpx<typename A::tw_t>) : 0);
    const void *kf = inverse ? reinterpret_cast<const void *>(k_fft_block<A, true, NT, FULL, TWL>)
                             : reinterpret_cast<const void *>(k_fft_block<A, false, NT, FULL, TWL>);
    LLZ_HIP_CHECK(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = grid_of(nblk);
    if (inverse)
        hipLaunchKernelGGL((k_fft_block<A, true, NT, FULL, TWL>), dim3(grid), dim3(NT), lds, st, data, nblk, p.log2b,
                           p.log2n, cs, twg, p.groups);
    else
        hipLaunchKernelGGL((k_fft_block<A, false, NT, FULL, TWL>), dim3(grid), dim3(NT), lds, st, data, nblk, p.log2b,
                           p.log2n, cs, twg, p.groups);
    return LLZ_OK;
}

template <typename A>
static void launch_bitrev(typename A::data_t *data, size_t count, int log2n, int scale, hipStream_t st)
{
    const size_t tiles = count << (log2n - 10);
    if (scale) hipLaunchKernelGGL((k_fft_bitrev<A, true>), dim3(grid_of(tiles)), dim3(256), 0, st, data, tiles, log2n);
    else hipLaunchKernelGGL((k_fft_bitrev<A, false>), dim3(grid_of(tiles)), dim3(256), 0, st, data, tiles, log2n);
}

// the one launcher: outer passes, LDS blocks and the bit reversal in the order of the plan
template <typename A>
static int run_large(typename A::data_t *data, size_t count, const fft_large_plan &p, const typename A::tw_t *cs,
                     const cpx<typename A::tw_t> *twg, int inverse, hipStream_t st, const char *name)
{
    constexpr bool F32 = std::is_same<A, arith_f32>::value;
    const size_t nblk = count << (p.log2n - p.log2b);
    auto block = [&]() -> int {
        if constexpr (F32) {
            // table in memory: 8192 points then take 68 KB of LDS, two workgroups per CU (load and compute overlap)
            if (p.outer == 0 && p.log2b <= 13) return launch_block<A, 512, true, false>(data, nblk, p, cs, twg, inverse, st);
            if (p.outer == 0) return launch_block<A, 1024, true, false>(data, nblk, p, cs, twg, inverse, st);
            return launch_block<A, 1024, false, false>(data, nblk, p, cs, twg, inverse, st);
        } else {
            return launch_block<A, FFT_THREADS, false, true>(data, nblk, p, cs, twg, inverse, st);
        }
    };
    auto outer = [&](int G, int log2step) {
        switch (G) {
        case 1: launch_outer<A, 1>(data, count, p.log2n, log2step, cs, inverse, st); break;
        case 2: launch_outer<A, 2>(data, count, p.log2n, log2step, cs, inverse, st); break;
        case 3: launch_outer<A, 3>(data, count, p.log2n, log2step, cs, inverse, st); break;
        default: launch_outer<A, 4>(data, count, p.log2n, log2step, cs, inverse, st); break;
        }
    };
    int rc;
    if (!inverse) {
        for (int q = 0, done = 0; q < p.outer; q++) {              // half-spans N/2 .. B
            outer(p.g[q], p.log2n - done - p.g[q]);
            done += p.g[q];
        }
        if ((rc = block()) != LLZ_OK) return rc;
        if (p.outer) launch_bitrev<A>(data, count, p.log2n, 0, st);
    } else {
        if (p.outer) launch_bitrev<A>(data, count, p.log2n, 1, st);
        if ((rc = block()) != LLZ_OK) return rc;
        for (int q = p.outer - 1, done = p.log2b; q >= 0; q--) {   // half-spans B .. N/2
            outer(p.g[q], done);
            done += p.g[q];
        }
    }
    LLZ_LAUNCH_CHECK(name);
    return LLZ_OK;
}

static int large_log2(int size, const char *name)
{
    int log2n = 0;
    while (log2n < 30 && (1 << log2n) < size) log2n++;
    if (size < 8192 || size > LLZS_FFT_MAX || (1 << log2n) != size) {
        llzs_set_error("%s: size %d must be a power of two in 8192..%d", name, size, LLZS_FFT_MAX);
        return -1;
    }
    return log2n;
}

} // namespace

extern "C" int llzs_fft_large_twb_bytes(int size)          // <= 68 KB: an int, like the other shim entries
{
    const int log2n = large_log2(size, "llzs_fft_large_twb_bytes");
    if (log2n < 0) return 0;
    const fft_large_plan p = fft_large_plan_of(1, log2n);
    return tw_entries(1 << p.log2b) * (int)sizeof(cpx<float>);
}

extern "C" int llzs_fft_large_twb(float *twb, int size, const float *cs, void *stream)
{
    const int log2n = large_log2(size, "llzs_fft_large_twb");
    if (log2n < 0 || !twb || !cs) return LLZ_ERR_ARG;
    const fft_large_plan p = fft_large_plan_of(1, log2n);
    const int half = 1 << (p.log2b - 1);
    hipLaunchKernelGGL(k_fft_large_twb, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<cpx<float> *>(twb), cs, p.log2b, log2n);
    LLZ_LAUNCH_CHECK("k_fft_large_twb");
    return LLZ_OK;
}

extern "C" int llzs_fft_large_passes(int size, int f32)
{
    const int log2n = large_log2(size, "llzs_fft_large_passes");
    return log2n < 0 ? LLZ_ERR_ARG : fft_large_plan_of(f32, log2n).passes;
}

extern "C" int llzs_fft_large_f32(float *data, int count, int size, const float *cs, const float *twb, int inverse,
                                  void *stream)
{
    const int log2n = large_log2(size, "llzs_fft_large_f32");
    if (log2n < 0) return LLZ_ERR_ARG;
    const fft_large_plan p = fft_large_plan_of(1, log2n);
    if (!data || !cs || !twb || count < 1) {
        llzs_set_error("llzs_fft_large_f32: NULL data or table, or count %d", count);
        return LLZ_ERR_ARG;
    }
    return run_large<arith_f32>(data, (size_t)count, p, cs, reinterpret_cast<const cpx<float> *>(twb), inverse,
                                as_stream(stream), "llzs_fft_large_f32");
}

extern "C" int llzs_fft_large_f64(double *data, int size, const double *cs, int inverse, void *stream)
{
    const int log2n = large_log2(size, "llzs_fft_large_f64");
    if (log2n < 0) return LLZ_ERR_ARG;
    if (!data || !cs) {
        llzs_set_error("llzs_fft_large_f64: NULL data or table");
        return LLZ_ERR_ARG;
    }
    const fft_large_plan p = fft_large_plan_of(0, log2n);
    return run_large<arith_f64>(data, 1, p, cs, nullptr, inverse, as_stream(stream), "llzs_fft_large_f64");
}
