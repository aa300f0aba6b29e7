// stream_bins.hpp -- what the frequency-domain delay lines share: fir_stream.hip (K4f), fir_stream_fade.hip (K4f while taps
// fade) and fir_matrix.hip (K4g).  The packed half-spectrum of a real block pair (B bins by position, position i holds bin
// bitrev(i), position 0 packs DC and Nyquist), its product step, the loads and stores of neighbouring bins, the two split
// steps between the B-point complex transform (part_fft.hpp) and that half-spectrum -- called by all three files, so that a
// block of the fade kernel that does not fade, and one path of the matrix form, give the stream convolver's values -- and
// the launch preamble of their launchers: block size, dispatch over the seven sizes, K4f's geometry and argument check, and the
// position of a launch within a fade (fade_pos and its check, the one place that holds the limit of 4096 blocks on the device
// side) for fir_stream_fade.hip and fir_matrix_fade.hip.
#pragma once
#include "common.hpp"
#include "part_fft.hpp"

namespace {

constexpr int stream_threads(int log2b) { return (1 << log2b) < 256 ? (1 << log2b) : 256; }

__device__ __forceinline__ float2 c_conj(float2 a) { return {a.x, -a.y}; }

// acc += x h; PACKED0: bin 0 holds DC and Nyquist, two real values: each half by its own
__device__ __forceinline__ void bin_mac(float2 &acc, float2 x, float2 h, bool packed0)
{
    const float xr = packed0 ? 0.f : x.x, xi = packed0 ? 0.f : x.y, hh = packed0 ? h.y : h.x;
    acc.x = __builtin_fmaf(-xi, h.y, __builtin_fmaf(x.x, h.x, acc.x));
    acc.y = __builtin_fmaf(x.y, hh, __builtin_fmaf(xr, h.y, acc.y));
}

// position of bin B - k for the position i > 0 of bin k = bitrev(i) (position 0, the packed bin, has no mirror: itself)
template <int LOG2B>
__device__ __forceinline__ int mirror(int i)
{
    const unsigned k = __brev((unsigned)i) >> (32 - LOG2B);
    return i ? (int)(__brev((1u << LOG2B) - k) >> (32 - LOG2B)) : 0;
}

// V neighbouring bins in one load (V = 2: 16 bytes; every row of ring and H starts on a multiple of 512 bytes)
template <int V>
__device__ __forceinline__ void load_bins(const float2 *p, float2 *dst)
{
    if (V == 2) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        dst[0] = float2{q.x, q.y};
        dst[1] = float2{q.z, q.w};
    } else {
        dst[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void store_bins(float2 *p, const float2 *src)
{
    if (V == 2) *reinterpret_cast<float4 *>(p) = float4{src[0].x, src[0].y, src[1].x, src[1].y};
    else *p = src[0];
}

// forward split: bin k of the real transform (doubled) = (Z_k + conj Z_{B-k}) + W_N^k (-j) (Z_k - conj Z_{B-k}); a = Z_k, zm =
// Z_{B-k}, w = W_N^k.  The packed bin: (DC, Nyquist) from Z_0 alone
__device__ __forceinline__ float2 split_fwd(float2 a, float2 zm, float2 w)
{
    const float2 b = c_conj(zm);
    const float2 e = c_add(a, b), d = c_sub(a, b);
    return c_add(e, c_mul<false>(float2{d.y, -d.x}, w));
}
__device__ __forceinline__ float2 split_fwd0(float2 a) { return float2{2.f * (a.x + a.y), 2.f * (a.x - a.y)}; }

// inverse split: Z''_k = (Y_k + conj Y_{B-k}) + j conj(W_N^k) (Y_k - conj Y_{B-k}); a = Y_k, ym = Y_{B-k}
__device__ __forceinline__ float2 split_inv(float2 a, float2 ym, float2 w)
{
    const float2 b = c_conj(ym);
    const float2 e = c_add(a, b), d = c_sub(a, b);
    return c_add(e, c_mul<true>(float2{-d.y, d.x}, w));
}
__device__ __forceinline__ float2 split_inv0(float2 a) { return float2{a.x + a.y, a.x - a.y}; }

// one sample of a crossfade between two filters' outputs (fir_stream_fade.hip): w = 0 gives y_old to the bit, equal outputs give
// that output to the bit at any w
__device__ __forceinline__ float fade_blend(float w, float y_old, float y_new) { return __builtin_fmaf(w, y_new - y_old, y_old); }

// ------------------------------------------------------------------------------------------------ the launch preamble
// block = 2^*log2b, 64 .. 4096
bool stream_log2(int block, int *log2b)
{
    int l = 0;
    while ((1 << l) < block) l++;
    *log2b = l;
    return l >= 6 && l <= 12 && (1 << l) == block;
}

// `return call(LOG2B);` for the block size; call: a macro of one argument
#define STREAM_DISPATCH(log2b, call)                                                                                             \
    switch (log2b) {                                                                                                             \
    case 6: return call(6);                                                                                                      \
    case 7: return call(7);                                                                                                      \
    case 8: return call(8);                                                                                                      \
    case 9: return call(9);                                                                                                      \
    case 10: return call(10);                                                                                                    \
    case 11: return call(11);                                                                                                    \
    default: return call(12);                                                                                                    \
    }

// one K4f launch, plain or fading (fir_stream_fade.hip derives its own from it)
struct stream_geom {
    int P, R, head;             // partitions, ring slots, the slot block 0 of this launch writes
    int nblk;                   // blocks of this launch (a flush: zero blocks, one per workgroup)
    int flush;
    long n_out;                 // samples per channel to store: <= nblk B
    long in_pitch, out_pitch;
};

// where a launch of a fade kernel stands in the fade (fir_stream_fade.hip, fir_matrix_fade.hip derive their geometries from
// it): the launch's block 0 is block fade_done of the fade's fade_blocks; blocks from fade_blocks on run the new taps alone
struct fade_pos {
    int fade_done, fade_blocks;
};

// fade_blocks B <= 2^24, so that a sample's index within the fade is exact in float; a launch starts inside the fade
bool fade_pos_ok(const fade_pos &F)
{
    return F.fade_blocks >= 1 && F.fade_blocks <= 4096 && F.fade_done >= 0 && F.fade_done < F.fade_blocks;
}

// G and the buffers of a K4f launch within the kernels' index ranges and the grid limits; in: null only for a flush
bool stream_launch_ok(const stream_geom &G, bool log2ok, int block, int channels, bool buffers, const float *in)
{
    const long n = (long)G.nblk * block;
    return log2ok && buffers && channels >= 1 && channels <= 65535 && G.nblk >= 1 && G.P >= 1 && G.R >= G.P && G.head >= 0 &&
           G.head < G.R && G.n_out >= 1 && G.n_out <= n && G.out_pitch >= G.n_out && (G.flush || (in && G.in_pitch >= n)) &&
           (!G.flush || (G.nblk <= 65535 && G.nblk <= G.P));
}

} // namespace
