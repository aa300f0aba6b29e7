// stft_large.hip -- the framing half of the composed float32 STFT batch (llz_stft_mc_*) for frames the one-launch kernels
// of stft.hip do not take: fft_len above 4096 (up to LLZS_FFT_MAX), and 4096 under the fft_generic tune.  The host
// (llz_asmodel_host.c) walks a call's frames in chunks of at most LLZS_STFT_CHUNK_POINTS points and, per chunk, runs
//
//   analysis  : k_stft_frames_large (windowed frames -> complex scratch), the float32 batch transform of llz_fft_batch on
//               the scratch (fft.hip up to 4096 points, fft_large.hip above), k_stft_bins_large (bins 0..N/2 -> re / im);
//   synthesis : k_stft_mirror_large (bins -> Hermitian-extended scratch), the inverse batch transform (which divides by N,
//               as llz_ifft does), k_stft_ola_large (windowed overlap-add, oldest frame first, tail carried per channel).
//
// A chunk is a run of consecutive transforms g = c * frames + f in the layout of re / im ([channels][frames][bins]), so it
// may start or end inside a channel.  Every offset into x, re, im and the scratch is 64-bit.
#include "common.hpp"

namespace {

// windowed frame g0 + blockIdx.y of concat(hist, x): samples [(f+1)F - N, (f+1)F) times the window, imaginary part zero
// (the values k_stft_analysis_f32 puts into LDS)
__global__ void __launch_bounds__(256)
k_stft_frames_large(const float *__restrict__ x, const float *__restrict__ hist, float2 *__restrict__ z,
                    const float *__restrict__ w, int frames, int F, int N, long x_pitch, long g0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long g = g0 + blockIdx.y;
    const long c = g / frames, f = g - c * frames;
    const long keep = N - F;
    const long t = (f + 1) * F - N + i;                                // sample index inside this call
    const float v = t >= 0 ? x[c * x_pitch + t] : hist[c * keep + (keep + t)];
    z[(size_t)blockIdx.y * N + i] = make_float2(v * w[i], 0.f);
}

// bins 0..N/2 of transform g0 + blockIdx.y (natural order after the batch transform's bit reversal)
__global__ void __launch_bounds__(256)
k_stft_bins_large(const float2 *__restrict__ z, float *__restrict__ re, float *__restrict__ im, int N, long g0)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int bins = (N >> 1) + 1;
    if (b >= bins) return;
    const float2 v = z[(size_t)blockIdx.y * N + b];
    const size_t o = (size_t)(g0 + blockIdx.y) * bins + b;
    re[o] = v.x;
    im[o] = v.y;
}

// the full spectrum of frame g0 + blockIdx.y: bins 0..N/2 as given, the upper half by Hermitian symmetry
// (llz_asmodel.c:279-288)
__global__ void __launch_bounds__(256)
k_stft_mirror_large(const float *__restrict__ re, const float *__restrict__ im, float2 *__restrict__ z, int N, long g0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int bins = (N >> 1) + 1;
    const size_t o = (size_t)(g0 + blockIdx.y) * bins;
    const float2 v = i < bins ? make_float2(re[o + i], im[o + i]) : make_float2(re[o + N - i], -im[o + N - i]);
    z[(size_t)blockIdx.y * N + i] = v;
}

// overlap-add of the chunk's inverse transforms, channel c = c0 + blockIdx.y.  The channel's frames in the chunk are
// fa .. fb-1; position p counts from sample fa * F of the channel's output.  acc = tail (positions < keep) + the windowed
// frames in ascending order (the reference's oldest-first sum); positions < nf * F leave scaled, the rest are the new tail,
// written to tail_out (the chunk's channels, [blockIdx.y][keep]) so that no workgroup reads a tail value another has
// already replaced.  tail_in: the handle's tail (ola_old) where the chunk holds the channel's first frame, else ola_new.
__global__ void __launch_bounds__(256)
k_stft_ola_large(const float2 *__restrict__ z, float *__restrict__ x, const float *__restrict__ ola_old,
                 const float *__restrict__ ola_new, float *__restrict__ tail_out, const float *__restrict__ w, int frames,
                 int F, int N, long x_pitch, long g0, long g1, long c0, float magic)
{
    const long c = c0 + blockIdx.y;
    const long fa = max(g0, c * frames) - c * frames, fb = min(g1, (c + 1) * frames) - c * frames;
    const int nf = (int)(fb - fa), keep = N - F;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nf * F + keep) return;
    const float *tail_in = (fa == 0 ? ola_old : ola_new) + c * keep;
    const float2 *zc = z + (size_t)(c * frames + fa - g0) * N;         // the channel's first frame in the chunk
    float a = p < keep ? tail_in[p] : 0.f;
    const int k_hi = min(nf - 1, p / F);                               // frames k with 0 <= p - kF < N
    const int k_lo = p < N ? 0 : (p - N) / F + 1;
    for (int k = k_lo; k <= k_hi; k++) {
        const int i = p - k * F;
        a += zc[(size_t)k * N + i].x * w[i];
    }
    if (p < nf * F) x[c * x_pitch + fa * F + p] = magic * a;
    else tail_out[(size_t)blockIdx.y * keep + (p - nf * F)] = a;
}

int large_shape(int frames, int F, int N, long g0, int count, const char *who)
{
    if (frames < 1 || F < 1 || N < 8 || N > LLZS_FFT_MAX || (N & (N - 1)) || (N != 2 * F && N != 4 * F) || g0 < 0 ||
        count < 1 || count > 32768) {
        llzs_set_error("%s: bad shape (frames=%d frame_len=%d fft_len=%d first=%ld count=%d)", who, frames, F, N, g0, count);
        return LLZ_ERR_ARG;
    }
    return LLZ_OK;
}

inline dim3 grid_of(int n, int count) { return dim3((unsigned)((n + 255) / 256), (unsigned)count); }

} // namespace

extern "C" int llzs_stft_frames_large_f32(const float *x, const float *hist, float *z, const float *w, int frames, int F,
                                          int N, long x_pitch, long g0, int count, void *stream)
{
    const int rc = large_shape(frames, F, N, g0, count, "stft_frames_large_f32");
    if (rc != LLZ_OK) return rc;
    if (!x || !hist || !z || !w || x_pitch < (long)frames * F) {
        llzs_set_error("stft_frames_large_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_stft_frames_large, grid_of(N, count), dim3(256), 0, as_stream(stream), x, hist,
                       reinterpret_cast<float2 *>(z), w, frames, F, N, x_pitch, g0);
    LLZ_LAUNCH_CHECK("k_stft_frames_large");
    return LLZ_OK;
}

extern "C" int llzs_stft_bins_large_f32(const float *z, float *re, float *im, int N, long g0, int count, void *stream)
{
    const int rc = large_shape(1, N / 2, N, g0, count, "stft_bins_large_f32");
    if (rc != LLZ_OK) return rc;
    if (!z || !re || !im) {
        llzs_set_error("stft_bins_large_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_stft_bins_large, grid_of((N >> 1) + 1, count), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2 *>(z), re, im, N, g0);
    LLZ_LAUNCH_CHECK("k_stft_bins_large");
    return LLZ_OK;
}

extern "C" int llzs_stft_mirror_large_f32(const float *re, const float *im, float *z, int N, long g0, int count,
                                          void *stream)
{
    const int rc = large_shape(1, N / 2, N, g0, count, "stft_mirror_large_f32");
    if (rc != LLZ_OK) return rc;
    if (!z || !re || !im) {
        llzs_set_error("stft_mirror_large_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_stft_mirror_large, grid_of(N, count), dim3(256), 0, as_stream(stream), re, im,
                       reinterpret_cast<float2 *>(z), N, g0);
    LLZ_LAUNCH_CHECK("k_stft_mirror_large");
    return LLZ_OK;
}

// tail: scratch of (channels in the chunk) * (N - F) floats; copied into ola_new after the overlap-add
extern "C" int llzs_stft_ola_large_f32(const float *z, float *x, const float *ola_old, float *ola_new, float *tail,
                                       const float *w, int frames, int F, int N, long x_pitch, long g0, int count,
                                       float magic, void *stream)
{
    const int rc = large_shape(frames, F, N, g0, count, "stft_ola_large_f32");
    if (rc != LLZ_OK) return rc;
    if (!z || !x || !ola_old || !ola_new || ola_old == ola_new || !tail || !w || x_pitch < (long)frames * F) {
        llzs_set_error("stft_ola_large_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    const long g1 = g0 + count, c0 = g0 / frames, c1 = (g1 - 1) / frames;
    const int span = (int)(count < frames ? count : frames) * F + (N - F);   // the longest channel run of the chunk
    const size_t keep = (size_t)(N - F);
    hipLaunchKernelGGL(k_stft_ola_large, grid_of(span, (int)(c1 - c0 + 1)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2 *>(z), x, ola_old, ola_new, tail, w, frames, F, N, x_pitch, g0, g1, c0,
                       magic);
    LLZ_LAUNCH_CHECK("k_stft_ola_large");
    return llzs_d2d(ola_new + (size_t)c0 * keep, tail, sizeof(float) * keep * (size_t)(c1 - c0 + 1), stream);
}
