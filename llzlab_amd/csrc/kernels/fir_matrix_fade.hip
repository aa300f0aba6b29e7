// fir_matrix_fade.hip -- K4g while paths fade (llz_fir_xfade_matrix_mc, include/llz_fir.h part 6): the product and the inverse of
// fir_matrix.hip with a second table of spectra (the NEW taps of the paths in the fade) beside the handle's.  For the span of
// the fade a fading OUTPUT -- one with at least one path in the fade -- runs both matrices' rows on the same delay lines and
// blends the two outputs sample by sample in the time domain, after the sum over inputs:
//     y_o[n] = fmaf(w[n], y_new_o[n] - y_old_o[n], y_old_o[n]),   w[n] = (float)n / (float)(F B), n from the fade's first sample.
// The delay lines hold INPUT spectra, so k_fir_matrix_fwd (fir_matrix.hip) serves a fade unchanged.  Calls with no fade pending
// or in flight run k_fir_matrix_mac / _inv; the files share stream_bins.hpp (the fade's position, fade_pos, with K4f's fade too) and
// the geometry of fir_matrix.hpp.  The inverse stays written out in both files: as one function of fir_matrix.hpp it kept every
// register limit, but a fading call at 2 -> 64, block 2048 took 0.4 % longer ("Shared code").
//
//   1. k_fir_matrix_mac_fade: k_fir_matrix_mac's grid, thread-to-bin ownership and U = 8 / V partitions in flight.  The block of
//      the fade, fb = fade_done + j0 + j, is the same for a whole workgroup, and so is each of its three cases:
//        * the output does not fade: the plain chain on H / conn into Y -- bin_mac over the group's inputs ascending and p
//          ascending from a zero accumulator, explicit fmas: k_fir_matrix_mac's bits;
//        * it fades and fb >= fade_blocks (a block past the end inside a call): one chain into Y that takes Hn / conn_new for
//          the paths in the fade and H / conn for the others: the bits k_fir_matrix_mac gives after set_taps(new);
//        * it fades and fb < fade_blocks: ONE walk over the group's inputs and partitions with two accumulator sets, Y (old)
//          and Yn (new).  Every ring bin is loaded once.  A path not in the fade loads its H bins once and feeds both chains
//          from the same registers; a path in the fade loads H and Hn; a path connected under one tap set only feeds that
//          chain only.  Each accumulator sees, term for term, the plain chain of its tap set.
//      The walk takes U partitions at a time: all their loads, then all their fmas (p ascending).  The accumulators pass through
//      an empty asm statement between the two, which the loads are ordered against and the fmas depend on: without it the
//      compiler issued the last loads of a group behind the first fmas, two memory latencies per group where one will do.
//   2. k_fir_matrix_inv_fade, grid (output, block): a block that does not blend is k_fir_matrix_inv's code; a blending one adds
//      the G partials of Y (g ascending), inverts, keeps the thread's B / T old samples in registers, does the same for Yn and
//      stores fade_blend(w, y_old, y_new) non-temporally, w by one correctly rounded division of two exact floats.
// The fade's position comes by value with each launch: no device-side counter, no atomics.  All index arithmetic over outputs x
// inputs x partitions x bins is size_t.
#include <type_traits>
#include "common.hpp"
#include "part_fft.hpp"
#include "stream_bins.hpp"
#include "fir_matrix.hpp"

namespace {

struct matrix_fade_geom : matrix_geom, fade_pos {};     // block j of this launch is block fade_done + j0 + j of the fade

// workgroup (o, j, tile + tiles g).  H / conn: the handle's spectra and connection table; Hn / conn_new: the new taps' (same
// layouts; read only where fade[o][i] is set); ofade[o]: 1 = output o has a path in the fade; Y / Yn: the old and the new
// partial spectra (Yn is written by blending blocks only)
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_matrix_mac_fade(const float2 *__restrict__ H, const float2 *__restrict__ Hn, const float2 *__restrict__ ring,
                      const unsigned char *__restrict__ conn, const unsigned char *__restrict__ conn_new,
                      const unsigned char *__restrict__ fade, const unsigned char *__restrict__ ofade, float2 *__restrict__ Y,
                      float2 *__restrict__ Yn, matrix_fade_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), V = mac_v(LOG2B), TILES = mac_tiles(LOG2B);
    constexpr int U = 8 / V;                                // partitions in flight
    const int tid = threadIdx.x, o = blockIdx.x, j = blockIdx.y;
    const int tile = (int)blockIdx.z % TILES, g = (int)blockIdx.z / TILES;
    const int pos = (tile * T + tid) * V;
    const bool first = pos == 0;                            // owner of position 0, the packed bin
    const int jj = G.j0 + j;                                // the block's place behind `head`: only a flush starts past 0
    const int cur = (G.head + jj) % G.R, p0 = G.flush ? jj : 0;
    const int i0 = g * G.gsize, i1 = i0 + G.gsize < G.inputs ? i0 + G.gsize : G.inputs;
    const bool of = ofade[o] != 0;                          // the same for the whole workgroup, as everything derived from it
    const bool blend = of && G.fade_done + jj < G.fade_blocks;
    const size_t row = (size_t)o * (size_t)G.inputs;
    float2 acc[V], accn[V];
#pragma unroll
    for (int v = 0; v < V; v++) acc[v] = accn[v] = float2{0.f, 0.f};

    // one path's partitions p0 .. P - 1, slot of X_{j-p} = (cur - p) mod R.  MODE 0: xv ha into a; 1: xv ha into a and b (one
    // load of ha); 2: xv ha into a, xv hb into b.  N steps at a time: all their loads first, then their fmas, p ascending
    auto walk = [&](auto mode, const float2 *rc, const float2 *ha, const float2 *hb, float2 *a, float2 *b) {
        constexpr int MODE = decltype(mode)::value;
        auto steps = [&](auto count, int pp) {
            constexpr int N = decltype(count)::value;
            float2 xv[N][V], h[N][V], hn[N][V];
#pragma unroll
            for (int u = 0; u < N; u++) {
                int s = cur - (pp + u);
                if (s < 0) s += G.R;
                load_bins<V>(rc + (size_t)s * B, xv[u]);
                load_bins<V>(ha + (size_t)(pp + u) * B, h[u]);
                if constexpr (MODE == 2) load_bins<V>(hb + (size_t)(pp + u) * B, hn[u]);
            }
            // the group's loads all issue before its first fma: the loads are ordered against these (empty) statements, and every
            // fma of the group takes its accumulator from one of them
#pragma unroll
            for (int v = 0; v < V; v++) {
                asm volatile("" : "+v"(a[v].x), "+v"(a[v].y) : : "memory");
                if constexpr (MODE != 0) asm volatile("" : "+v"(b[v].x), "+v"(b[v].y) : : "memory");
            }
#pragma unroll
            for (int u = 0; u < N; u++) {
#pragma unroll
                for (int v = 0; v < V; v++) {
                    bin_mac(a[v], xv[u][v], h[u][v], v == 0 && first);
                    if constexpr (MODE == 1) bin_mac(b[v], xv[u][v], h[u][v], v == 0 && first);
                    if constexpr (MODE == 2) bin_mac(b[v], xv[u][v], hn[u][v], v == 0 && first);
                }
            }
        };
        int p = p0;
#pragma unroll 1
        for (; p + U <= G.P; p += U) steps(std::integral_constant<int, U>{}, p);
#pragma unroll 1
        for (; p < G.P; p++) steps(std::integral_constant<int, 1>{}, p);
    };
    const std::integral_constant<int, 0> ONE{};
    const std::integral_constant<int, 1> SHARED{};
    const std::integral_constant<int, 2> BOTH{};

    for (int i = i0; i < i1; i++) {
        const size_t path = row + (size_t)i;
        const bool fd = of && fade[path] != 0;              // without a fading output no path of the row is in the fade
        const bool co = conn[path] != 0;                    // under the old taps
        const bool cn = fd ? conn_new[path] != 0 : co;      // under the new ones: a path not in the fade keeps its taps
        const float2 *rc = ring + (size_t)i * (size_t)G.R * B + pos;
        const float2 *ho = H + path * (size_t)G.P * B + pos, *hn = Hn + path * (size_t)G.P * B + pos;
        if (!blend) {
            // the plain chain: the old taps, or past the fade's end the row as set_taps(new) would have left it (fd is set
            // only for a fading output, and cn is co where it is not)
            if (cn) walk(ONE, rc, fd ? hn : ho, nullptr, acc, nullptr);
        } else if (!fd) {
            if (co) walk(SHARED, rc, ho, nullptr, acc, accn);
        } else if (co && cn) {
            walk(BOTH, rc, ho, hn, acc, accn);
        } else if (co) {
            walk(ONE, rc, ho, nullptr, acc, nullptr);        // fading out: the old sum alone
        } else if (cn) {
            walk(ONE, rc, hn, nullptr, accn, nullptr);       // fading in: the new sum alone
        }
    }
    const size_t at = (((size_t)g * (size_t)G.outputs + (size_t)o) * (size_t)G.nblk + (size_t)j) * B + pos;
    store_bins<V>(Y + at, acc);
    if (blend) store_bins<V>(Yn + at, accn);
}

// workgroup (o, j): the partials added, g ascending; inverse split and transform; the last B samples out, blended while output
// o fades
template <int LOG2B>
__global__ void __launch_bounds__(stream_threads(LOG2B))
k_fir_matrix_inv_fade(const float2 *__restrict__ Y, const float2 *__restrict__ Yn, const unsigned char *__restrict__ ofade,
                      const float2 *__restrict__ tw, float *__restrict__ out, matrix_fade_geom G)
{
    constexpr int B = 1 << LOG2B, T = stream_threads(LOG2B), M = B / T, V = M >= 2 ? 2 : 1, NG = M / V;
    __shared__ __align__(16) float2 lds[B];
    float *lf = reinterpret_cast<float *>(lds);
    const int tid = threadIdx.x, o = blockIdx.x, j = blockIdx.y;
    const float2 *spl = tw + B / 2;
    const size_t gstride = (size_t)G.outputs * (size_t)G.nblk * B;
    const size_t yoff = ((size_t)o * (size_t)G.nblk + (size_t)j) * B;
    const int fb = G.fade_done + G.j0 + j;                  // this block's place in the fade
    const bool blend = ofade[o] != 0 && fb < G.fade_blocks; // the same for the whole workgroup

    // k_fir_matrix_inv's steps on one scratch: the block's B output samples are lf[B ..) afterwards
    auto inverse = [&](const float2 *y0) {
        float2 acc[M];
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int pos = (tid + g * T) * V;
            load_bins<V>(y0 + pos, &acc[g * V]);
            for (int gg = 1; gg < G.G; gg++) {
                float2 part[V];
                load_bins<V>(y0 + (size_t)gg * gstride + pos, part);
#pragma unroll
                for (int v = 0; v < V; v++) acc[g * V + v] = c_add(acc[g * V + v], part[v]);
            }
            store_bins<V>(lds + pos, &acc[g * V]);
        }
        __syncthreads();
        float2 zz[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int q = (tid + (m / V) * T) * V + m % V;
            zz[m] = split_inv(acc[m], lds[mirror<LOG2B>(q)], spl[q]);
            if (q == 0) zz[m] = split_inv0(acc[m]);
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NG; g++) store_bins<V>(lds + (tid + g * T) * V, &zz[g * V]);
        part_fft_dit_inv<LOG2B, T>(lds, tw, tid);
    };

    float *orow = out + (size_t)o * (size_t)G.out_pitch;
    if (!blend) {
        inverse(Y + yoff);
        for (int t = tid; t < B; t += T) {
            const long n = (long)j * B + t;
            if (n < G.n_out) __builtin_nontemporal_store(lf[B + t], &orow[n]);
        }
    } else {
        float yo[M];                                        // the old matrix's samples of this thread: t = tid + m T
        inverse(Y + yoff);
#pragma unroll
        for (int m = 0; m < M; m++) yo[m] = lf[B + tid + m * T];
        __syncthreads();                                    // every read of the old output is done before the image is reused
        inverse(Yn + yoff);
        const float den = (float)((long)G.fade_blocks * B); // F B <= 2^24: exact
#pragma unroll
        for (int m = 0; m < M; m++) {
            const int t = tid + m * T;
            const long n = (long)j * B + t;
            const float w = __fdiv_rn((float)((long)fb * B + t), den);
            if (n < G.n_out) __builtin_nontemporal_store(fade_blend(w, yo[m], lf[B + t]), &orow[n]);
        }
    }
}

template <int LOG2B>
int mac_fade_launch(const float2 *H, const float2 *Hn, const float2 *ring, const unsigned char *conn,
                    const unsigned char *conn_new, const unsigned char *fade, const unsigned char *ofade, float2 *Y, float2 *Yn,
                    const matrix_fade_geom &G, hipStream_t st)
{
    const dim3 grid((unsigned)G.outputs, (unsigned)G.nblk, (unsigned)(mac_tiles(LOG2B) * G.G)), wg(stream_threads(LOG2B));
    hipLaunchKernelGGL((k_fir_matrix_mac_fade<LOG2B>), grid, wg, 0, st, H, Hn, ring, conn, conn_new, fade, ofade, Y, Yn, G);
    LLZ_LAUNCH_CHECK("k_fir_matrix_mac_fade");
    return LLZ_OK;
}

template <int LOG2B>
int inv_fade_launch(const float2 *Y, const float2 *Yn, const unsigned char *ofade, const float2 *tw, float *out,
                    const matrix_fade_geom &G, hipStream_t st)
{
    const dim3 grid((unsigned)G.outputs, (unsigned)G.nblk), wg(stream_threads(LOG2B));
    hipLaunchKernelGGL((k_fir_matrix_inv_fade<LOG2B>), grid, wg, 0, st, Y, Yn, ofade, tw, out, G);
    LLZ_LAUNCH_CHECK("k_fir_matrix_inv_fade");
    return LLZ_OK;
}

} // namespace

// llzs_fir_matrix_mac_f32's launch with a fade pending or in flight.  hspec_new, conn_new: the new taps' spectra and connection
// table, laid out as hspec and conn (read only where fade[o][i] != 0); fade: [outputs][inputs] bytes, the paths in the fade;
// ofade: [outputs] bytes, the outputs with such a path; ypart_new: a second scratch laid out as ypart.  Block j of this launch
// is block fade_done + j0 + j of the fade's fade_blocks.
extern "C" int llzs_fir_matrix_mac_fade_f32(int block, const float *hspec, const float *hspec_new, const float *ring,
                                            const unsigned char *conn, const unsigned char *conn_new, const unsigned char *fade,
                                            const unsigned char *ofade, float *ypart, float *ypart_new, int inputs, int outputs,
                                            int nblk, int flush, int j0, int P, int R, int head, int groups, int group_size,
                                            int fade_done, int fade_blocks, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    if (!matrix_shape_ok(ok, inputs, outputs, nblk, P, R, head) || !hspec || !hspec_new || !ring || !conn || !conn_new || !fade ||
        !ofade || !ypart || !ypart_new || ypart == ypart_new ||
        !matrix_groups_ok(block, inputs, nblk, flush, j0, P, groups, group_size) || !fade_pos_ok({fade_done, fade_blocks})) {
        llzs_set_error("fir_matrix_mac_fade_f32: bad arguments (block=%d inputs=%d outputs=%d nblk=%d j0=%d P=%d R=%d head=%d "
                       "groups=%d x %d fade %d of %d)", block, inputs, outputs, nblk, j0, P, R, head, groups, group_size, fade_done,
                       fade_blocks);
        return LLZ_ERR_ARG;
    }
    matrix_fade_geom G = {};
    G.inputs = inputs; G.outputs = outputs; G.P = P; G.R = R; G.head = head; G.nblk = nblk; G.flush = flush ? 1 : 0;
    G.j0 = j0; G.G = groups; G.gsize = group_size; G.fade_done = fade_done; G.fade_blocks = fade_blocks;
    const float2 *H = reinterpret_cast<const float2 *>(hspec), *Hn = reinterpret_cast<const float2 *>(hspec_new);
    const float2 *rg = reinterpret_cast<const float2 *>(ring);
    float2 *Y = reinterpret_cast<float2 *>(ypart), *Yn = reinterpret_cast<float2 *>(ypart_new);
    hipStream_t st = as_stream(stream);
#define MACF(L) mac_fade_launch<L>(H, Hn, rg, conn, conn_new, fade, ofade, Y, Yn, G, st)
    STREAM_DISPATCH(log2b, MACF)
#undef MACF
}

// llzs_fir_matrix_inv_f32's launch with a fade pending or in flight: an output marked in ofade whose block fade_done + j0 + j
// lies inside the fade is fade_blend(w, inverse of ypart, inverse of ypart_new), every other block the inverse of ypart
extern "C" int llzs_fir_matrix_inv_fade_f32(int block, const float *ypart, const float *ypart_new, const unsigned char *ofade,
                                            const float *tw, float *out, int outputs, int nblk, int j0, int groups, long n_out,
                                            long out_pitch, int fade_done, int fade_blocks, void *stream)
{
    int log2b;
    const bool ok = stream_log2(block, &log2b);
    if (!matrix_shape_ok(ok, 1, outputs, nblk, 1, 1, 0) || !ypart || !ypart_new || !ofade || !tw || !out || groups < 1 || j0 < 0 ||
        n_out < 1 || n_out > (long)nblk * block || out_pitch < n_out || !fade_pos_ok({fade_done, fade_blocks})) {
        llzs_set_error("fir_matrix_inv_fade_f32: bad arguments (block=%d outputs=%d nblk=%d j0=%d groups=%d n_out=%ld out_pitch=%ld "
                       "fade %d of %d)", block, outputs, nblk, j0, groups, n_out, out_pitch, fade_done, fade_blocks);
        return LLZ_ERR_ARG;
    }
    matrix_fade_geom G = {};
    G.outputs = outputs; G.nblk = nblk; G.j0 = j0; G.G = groups; G.n_out = n_out; G.out_pitch = out_pitch;
    G.fade_done = fade_done; G.fade_blocks = fade_blocks;
    const float2 *Y = reinterpret_cast<const float2 *>(ypart), *Yn = reinterpret_cast<const float2 *>(ypart_new);
    const float2 *W = reinterpret_cast<const float2 *>(tw);
    hipStream_t st = as_stream(stream);
#define INVF(L) inv_fade_launch<L>(Y, Yn, ofade, W, out, G, st)
    STREAM_DISPATCH(log2b, INVF)
#undef INVF
}
