// asrc.hip -- kernel K3r: llz_asrc_mc, the arbitrary-ratio resampler (include/llz_asrc.h states the definition).
//
// A channel's integer state (llz_asrc_time.h: position of its next output in the call's buffer, step, glide) lives on the device and
// is mirrored by the host layer, which runs the same code on it: the host knows every count without asking the device, and a
// call on device pointers is two or three launches ordered by the stream and no copy in either direction.
//
//   k_asrc_f32      grid (tile groups, channels), 1024 lanes, one output per lane and tile.  A tile of 1024 consecutive outputs
//                   takes its first and last time from the closed form, stages that span of [history | input] into LDS (16 steps
//                   of 16 samples per output at the most: 16497 floats), and each lane whose own time lies inside the call runs
//                   the T taps: c_k = fma(a, G[p+1][k] - G[p][k], G[p][k]), y = fma(x[n + T/2 - k], c_k, y), k ascending from
//                   y = 0.  A tile whose first output lies beyond the call leaves at once; no lane stores at or beyond its
//                   channel's count.  A workgroup walks `tiles_per_wg` consecutive tiles (32 on long calls): the LDS table form loads
//                   its table once per walk (74 KB against 8 B of signal per output), and while a tile computes, the next tile's
//                   span is already on its way into two registers per lane (spans up to 2048 samples, steps up to 2; a longer
//                   span is staged when its turn comes).  With the table a CU holds one workgroup, so without that prefetch all
//                   16 waves wait out every span's load: 14.3 -> 9.6 ms for 1024 channels x 2^20 samples at step 1.000023.
//   table forms     LDS: the whole table image, rows of llz_asrc_time.h's pitch, read 16 bytes at a time (two rows of four taps per
//                   four input samples: 3 LDS dwords per tap and output, the rows in two 16-byte reads, the samples in dword reads);
//                   global: the same image and the same reads through the caches, for tables beyond the LDS budget (up to 2.1 MB).
//                   Both forms compute the same bits.
//   k_asrc_advance  a lane per channel: the count of the call by llz_asrc_time.h's bisection, then the state behind the call.
// The history behind a call is llzs_fir_tail_f32's (T - 1 samples, ping-pong buffers).
#include <atomic>
#include "common.hpp"
#include "../llz_asrc_time.h"

#define ASRC_THREADS 1024
#define ASRC_TILE 1024
#define ASRC_SPAN (ASRC_TILE * 16 + LLZ_ASRC_MAX_TAPS + 16)        // floats of LDS for a tile's input span

// the span of [history | input] that the tile of outputs j0 .. j0 + 1023 reads: false when the tile lies beyond the count
__device__ static inline bool asrc_span(const llz_asrc_state *s, unsigned long long j0, unsigned long long bound, long avail, int half,
                                        long *first, long *len)
{
    const unsigned long long t0 = llz_asrc_time(s, j0);
    if (t0 >= bound) return false;
    long lo = (long)(t0 >> 32) - half + 1;                          // >= 0: an output not yet delivered has n + T/2 >= H
    if (lo < 0) lo = 0;
    long hi = (long)(llz_asrc_time(s, j0 + ASRC_TILE - 1) >> 32) + half;
    if (hi > avail - 1) hi = avail - 1;
    *first = lo;
    *len = hi - lo + 1 > ASRC_SPAN ? ASRC_SPAN : hi - lo + 1;       // (steps within 1/16 .. 16 never reach the cap)
    return true;
}

template <bool TABLE_LDS>
__global__ void __launch_bounds__(ASRC_THREADS)
k_asrc_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist, const float *__restrict__ table,
           const llz_asrc_state *__restrict__ state, long n_in, long in_pitch, long out_pitch, int T, int logphi, int pitch,
           int tiles_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds, *gs = lds + ASRC_SPAN;
    const int c = blockIdx.y, tid = threadIdx.x, H = T - 1, half = T / 2;
    const llz_asrc_state s = state[c];
    const long avail = H + n_in;                                    // samples of [history | input]
    const unsigned long long bound = (unsigned long long)(avail - half) << 32;
    unsigned long long j0 = (unsigned long long)blockIdx.x * (unsigned)tiles_per_wg * ASRC_TILE;
    long first, len;
    if (!asrc_span(&s, j0, bound, avail, half, &first, &len)) return;      // the whole group lies beyond this channel's count
    if (TABLE_LDS) {
        const int quads = ((1 << logphi) + 1) * (pitch / 4);
        for (int i = tid; i < quads; i += ASRC_THREADS)
            reinterpret_cast<float4 *>(gs)[i] = reinterpret_cast<const float4 *>(table)[i];
    }
    const float *x_c = in + (size_t)c * in_pitch, *h_c = hist + (size_t)c * H;
    const float ascale = __uint_as_float((unsigned)(127 - (32 - logphi)) << 23);       // 2^-(32 - log2 phases)
    float r0 = 0.f, r1 = 0.f;                                       // the next tile's span, two samples per lane, while it fits
    bool fetched = false;
    for (int tile = 0;; tile++) {
        if (tile) __syncthreads();                                  // the tile before has read its span
        if (fetched) {
            if (tid < len) xs[tid] = r0;
            if (tid + ASRC_THREADS < len) xs[tid + ASRC_THREADS] = r1;
        } else {
            for (long i = tid; i < len; i += ASRC_THREADS) {
                const long idx = first + i;
                xs[i] = idx < H ? h_c[idx] : x_c[idx - H];
            }
        }
        __syncthreads();
        // the loads of the next tile's span fly while this tile computes (steps up to 2: 2048 samples; longer spans are staged
        // when their turn comes)
        long nfirst = 0, nlen = 0;
        const bool more = tile + 1 < tiles_per_wg && asrc_span(&s, j0 + ASRC_TILE, bound, avail, half, &nfirst, &nlen);
        fetched = more && nlen <= 2 * ASRC_THREADS;
        if (fetched) {
            const long i0 = nfirst + tid, i1 = i0 + ASRC_THREADS;
            if (tid < nlen) r0 = i0 < H ? h_c[i0] : x_c[i0 - H];
            if (tid + ASRC_THREADS < nlen) r1 = i1 < H ? h_c[i1] : x_c[i1 - H];
        }
        const unsigned long long tj = llz_asrc_time(&s, j0 + tid);
        if (tj < bound) {
            const long n = (long)(tj >> 32);
            const unsigned frac = (unsigned)tj, p = frac >> (32 - logphi);
            const float a = (float)(frac & ((1u << (32 - logphi)) - 1u)) * ascale;      // at most 24 bits: exact
            const float *g0 = (TABLE_LDS ? gs : table) + (size_t)p * pitch, *g1 = g0 + pitch;
            const float *x = xs + (n - first) + half;               // x[-k] = sample n + T/2 - k
            float y = 0.f;
            const int T4 = T & ~3;
            for (int k = 0; k < T4; k += 4) {
                const float4 u = *reinterpret_cast<const float4 *>(g0 + k), v = *reinterpret_cast<const float4 *>(g1 + k);
                y = fmaf(x[-k], fmaf(a, v.x - u.x, u.x), y);
                y = fmaf(x[-k - 1], fmaf(a, v.y - u.y, u.y), y);
                y = fmaf(x[-k - 2], fmaf(a, v.z - u.z, u.z), y);
                y = fmaf(x[-k - 3], fmaf(a, v.w - u.w, u.w), y);
            }
            if (T4 < T) {                                           // T is even: two taps are left
                const float2 u = *reinterpret_cast<const float2 *>(g0 + T4), v = *reinterpret_cast<const float2 *>(g1 + T4);
                y = fmaf(x[-T4], fmaf(a, v.x - u.x, u.x), y);
                y = fmaf(x[-T4 - 1], fmaf(a, v.y - u.y, u.y), y);
            }
            out[(size_t)c * out_pitch + j0 + tid] = y;
        }
        if (!more) break;
        first = nfirst; len = nlen; j0 += ASRC_TILE;
    }
}

__global__ void __launch_bounds__(256)
k_asrc_advance(llz_asrc_state *__restrict__ state, int channels, long n_in, int T)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= channels) return;
    llz_asrc_state s = state[c];
    const unsigned long long bound = (unsigned long long)(T - 1 + n_in - T / 2) << 32;
    llz_asrc_advance(&s, llz_asrc_count(&s, bound), (unsigned long long)n_in);
    state[c] = s;
}

// the dynamic-LDS ceiling of a table form, raised once per device: the largest a launch of that form can ask for
static int asrc_allow_lds(bool table_lds)
{
    static std::atomic<unsigned long long> done[2];
    int device = 0;
    LLZ_HIP_CHECK(hipGetDevice(&device));
    const unsigned long long bit = 1ull << (device & 63);
    if (device < 64 && (done[table_lds].load(std::memory_order_acquire) & bit)) return LLZ_OK;
    const size_t most = sizeof(float) * ASRC_SPAN + (table_lds ? LLZ_ASRC_LDS_TABLE_BYTES : 0);
    const void *kernel = table_lds ? reinterpret_cast<const void *>(k_asrc_f32<true>) : reinterpret_cast<const void *>(k_asrc_f32<false>);
    LLZ_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
    done[table_lds].fetch_or(bit, std::memory_order_release);
    return LLZ_OK;
}

static int asrc_log2(int v)
{
    int l = 0;
    while ((1 << l) < v) l++;
    return (1 << l) == v ? l : -1;
}

extern "C" int llzs_asrc_f32(const float *in, float *out, const float *hist, const float *table, const void *state, int channels,
                             long n_in, long in_pitch, long out_pitch, int T, int phases, int table_lds, long max_count,
                             void *stream)
{
    const int logphi = asrc_log2(phases), pitch = LLZ_ASRC_PITCH(T);
    if (!in || !out || !hist || !table || !state || channels < 1 || channels > 65535 || n_in < 1 || n_in > LLZ_ASRC_MAX_FRAME ||
        in_pitch < n_in || max_count < 1 || out_pitch < max_count || T < LLZ_ASRC_MIN_TAPS || T > LLZ_ASRC_MAX_TAPS || (T & 1) ||
        logphi < 0 || phases < LLZ_ASRC_MIN_PHASES || phases > LLZ_ASRC_MAX_PHASES) {
        llzs_set_error("asrc_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const size_t tbytes = sizeof(float) * (size_t)(phases + 1) * pitch;
    if (table_lds && tbytes > LLZ_ASRC_LDS_TABLE_BYTES) {
        llzs_set_error("asrc_f32: a table of %zu B does not fit the LDS form (%d B)", tbytes, LLZ_ASRC_LDS_TABLE_BYTES);
        return LLZ_ERR_RANGE;
    }
    const long tiles = (max_count + ASRC_TILE - 1) / ASRC_TILE;
    const int tpw = tiles >= 128 ? 32 : tiles >= 32 ? 8 : tiles >= 8 ? 2 : 1;
    const size_t lds = sizeof(float) * ASRC_SPAN + (table_lds ? tbytes : 0);
    const dim3 grid((unsigned)((tiles + tpw - 1) / tpw), (unsigned)channels);
    const auto kernel = table_lds ? k_asrc_f32<true> : k_asrc_f32<false>;
    const int rc = asrc_allow_lds(table_lds != 0);
    if (rc != LLZ_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(ASRC_THREADS), lds, as_stream(stream), in, out, hist, table,
                       static_cast<const llz_asrc_state *>(state), n_in, in_pitch, out_pitch, T, logphi, pitch, tpw);
    LLZ_LAUNCH_CHECK("k_asrc_f32");
    return LLZ_OK;
}

extern "C" int llzs_asrc_advance(void *state, int channels, long n_in, int T, void *stream)
{
    if (!state || channels < 1 || n_in < 1 || n_in > LLZ_ASRC_MAX_FRAME || T < LLZ_ASRC_MIN_TAPS || T > LLZ_ASRC_MAX_TAPS) {
        llzs_set_error("asrc_advance: bad arguments");
        return LLZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_asrc_advance, dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<llz_asrc_state *>(state), channels, n_in, T);
    LLZ_LAUNCH_CHECK("k_asrc_advance");
    return LLZ_OK;
}
