/*
 * include/llz_pfb.h -- uniform DFT polyphase filter bank for many channels (weighted overlap-add), analysis and synthesis, C ABI
 * of libllzfilter_hip.so: llz_pfb_mc.  It is what llz_stft_mc (llz_asmodel.h) cannot be: a prototype filter several transform
 * lengths long folded into the transform, a free prototype for each direction, and a hop that gives critically sampled or 2x, 4x
 * or 8x oversampled bands -- the front end of subband echo cancellation around the adaptive filters and the arbitrary-ratio
 * resampler, of channelisers, of codec and analyser front ends next to the MDCT.  The reference has no counterpart; the checker
 * is a float64 model written from the definition below (tests/pfb_checks.py).
 *
 * THE DEFINITION
 *
 * M bands, a power of two in 8..4096.  D the hop, M / D in {1, 2, 4, 8}.  P taps per band, 1..16.  L = P M the prototype length,
 * at most 32768.  R = L / D, at most 128.  The analysis window w[0..L) and the synthesis window g[0..L) are the caller's float32
 * arrays; index 0 weighs the OLDEST sample of a frame (as a filter the analysis prototype is h[n] = w[L - 1 - n]).
 *
 * Streams start at t = 0 with zero history.  Frames are counted m = 0, 1, ... from init or reset, separately per direction.
 * Frame m starts at s_m = (m + 1) D - L.
 *
 * Analysis.  v_m[i] = w[i] x[s_m + i].  The fold u_m[r] = sum_{p < P} v_m[r + p M] is summed in float32 with p ascending: every
 * product is rounded to float32, the sum starts with the product of p = 0 and every addition is rounded.  (The order is part of
 * the contract: the bitwise properties below rest on it.)
 *   LLZ_PFB_PHASE_FRAME   X_m[k] = sum_r u_m[r] e^{-j 2 pi k r / M}: llz_stft_mc's convention; P = 1 is an STFT with a free window.
 *   LLZ_PFB_PHASE_TIME    X_m[k] = sum_i v_m[i] e^{-j 2 pi k (s_m + i) / M}: every band is a proper baseband signal at rate
 *                         fs / D.  Since M divides L this is the same transform of u_m placed at (r + (m + 1) D) mod M: an index
 *                         rotation, no extra arithmetic.
 * Bins 0..M/2 go to re / im, [channels][frames][M/2 + 1], llz_stft_mc's layout.
 *
 * Synthesis.  u_m = the real part of the 1/M-scaled inverse transform of the Hermitian extension of bins 0..M/2 (the imaginary
 * parts of bins 0 and M/2 belong to no real frame: their effect is unspecified); in TIME phase the rotation is undone.  v_m[i] =
 * g[i] u_m[i mod M], one rounded product.  The running sum is y[t] += v_m[t - s_m], for every sample added oldest frame first,
 * from +0, every addition rounded.  A call of `frames` frames emits frames D samples: block m is the running sum over [s_m,
 * s_m + D), complete once frame m is added; while that lies before t = 0 (the first R - 1 blocks) it is what the frames so far put
 * on top of the zeros of the initial tail.  Analysis followed by synthesis therefore has a delay of L - D samples.  There is
 * no built-in scale: g carries it.
 *
 * One handle serves both directions.  Per channel it keeps the last L - D input samples (analysis) and the overlap-add tail of
 * L - D partial sums (synthesis), so consecutive calls continue the streams: the tail holds exactly the partial sums the same
 * frames would have produced inside one call.
 *
 * BITWISE PROPERTIES.  No bit of any output depends on how frames are grouped into calls (down to calls of one frame), on which
 * frames share a workgroup, on the analysis form (llz_pfb_mc_plan), or on what the other channels hold.
 */
#ifndef LLZ_PFB_H
#define LLZ_PFB_H

#ifdef __cplusplus
extern "C" {
#endif

enum { LLZ_PFB_PHASE_FRAME = 0, LLZ_PFB_PHASE_TIME = 1 };

#define LLZ_PFB_MAX_TAPS 16             /* P */
#define LLZ_PFB_MAX_LENGTH 32768        /* L = P M */

/* channels 1..65535; bands = M, hop = D, taps_per_band = P as above; w: HOST [P M] floats; g: HOST [P M] floats, NULL means
 * g = w; both are copied.  Every refusal leaves a message of its own (llz_hip_last_error).  Returns the handle or
 * (unsigned long)-1. */
unsigned long llz_pfb_mc_init(int channels, int bands, int hop, int taps_per_band, const float *w, const float *g, int phase);
void llz_pfb_mc_uninit(unsigned long h);
/* M / 2 + 1 */
int  llz_pfb_mc_bins(unsigned long h);
/* L - D, the delay in samples of analysis followed by synthesis */
int  llz_pfb_mc_delay(unsigned long h);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_pfb_mc_set_stream(unsigned long h, void *stream);
/* x: planar [channels][frames D] float32; re, im: [channels][frames][M/2 + 1].  Host or device pointers; device memory is used
 * in place on the handle's stream.  frames = 0 returns 0 and touches nothing; frames D is at most 2^31 - 1.  Device output that
 * overlaps device input is refused with LLZ_ERR_ARG and the handle is left untouched.  Returns frames, or a negative LLZ_ERR_*. */
int  llz_pfb_mc_analysis(unsigned long h, const float *x, float *re, float *im, int frames);
int  llz_pfb_mc_synthesis(unsigned long h, const float *re, const float *im, float *x, int frames);
/* both histories to zeros, both frame counters to 0: the state of a fresh handle */
int  llz_pfb_mc_reset(unsigned long h);
/* frames taken per direction since init or reset (either pointer may be NULL) */
int  llz_pfb_mc_frames(unsigned long h, long long *analysis, long long *synthesis);
/* what a call of `frames` frames launches; nothing is launched.  out[0..3], analysis: form (0 = the span of a workgroup's frames
 * staged in LDS, 1 = samples read through the caches), frames per workgroup, workgroups, LDS bytes per workgroup.  out[4..7],
 * synthesis: form (1 = inverse transforms into the handle's scratch, then a gather per sample), frames per workgroup of the
 * inverse transforms, their workgroups in the first chunk of frames, their LDS bytes. */
int  llz_pfb_mc_plan(unsigned long h, int frames, int out[8]);

#ifdef __cplusplus
}
#endif
#endif
