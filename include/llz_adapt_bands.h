/*
 * include/llz_adapt_bands.h -- adaptive filters in the bands of a filter bank, C ABI of libllzfilter_hip.so: llz_adapt_bands_mc,
 * a normalised LMS filter of K complex taps for every (channel, bin) of a batch of band signals, updated frame by frame at the
 * band rate.  It is the step between the analysis and the synthesis of the polyphase filter bank (or of llz_stft_mc) in a subband
 * echo canceller: the bands of a loudspeaker signal x and of a microphone signal d go in, the bands of the error e come out, and
 * the synthesis of e is the microphone signal with the echo removed -- at the delay of the bank alone, where the full-band block
 * filters of llz_adapt.h add a block.  An oversampled bank (2x to 8x) feeds K taps per band, and each band converges on its own
 * power.  The reference has no counterpart; the checker is a float64 model written from the definition below
 * (tests/adapt_bands_checks.py).  One reference per band and no terms across bands.
 *
 * Signals are band signals in llz_stft_mc's layout, [channels][frames][bins] float32, re and im in arrays of their own.  bins is
 * a free parameter, 1..4097: M / 2 + 1 for a bank or a transform of M bands, but the handle knows nothing of a bank.  K = taps,
 * 1..64.
 *
 * The algorithm.  Every (channel c, bin k) is a stream of its own: weights w_q, q = 0 .. K - 1, complex, initially zero; a
 * history x[m - q], zero before frame 0; frames counted from the init or the last reset.  For frame m, in order:
 *   1. y = sum_{q < K} w_q x[m - q], a complex product, NO conjugate on w.
 *   2. e = d[m] - y, one float32 subtraction per component: e has the bits of float32(d) - y.  e is always stored, y when the
 *      caller passes buffers for it.
 *   3. If the channel's mu is not zero: p = sum_{q < K} |x[m - q]|^2, taken from the history anew in every frame (there is no
 *      running or smoothed power state); g = mu e / (p + delta); w_q += g conj(x[m - q]) for every q < K.
 *   4. A channel whose mu is 0 is FROZEN: step 3 is skipped, its weights keep their bits, y and e are still produced.
 * Taps q >= K do not exist: whatever tap ceiling the kernel instance was built for (llz_adapt_bands_mc_plan), it neither filters
 * with them nor updates them.
 *
 * Arithmetic: float32 throughout, and the order of every sum is fixed in terms of the AGE q, never of where a value sits in a
 * register or a loop.  With fma(a, b, c) = a b + c rounded once, every sum starts from 0 and runs over q ASCENDING:
 *   y_re = fma(-w_im, x_im, fma(w_re, x_re, y_re))         y_im = fma(w_im, x_re, fma(w_re, x_im, y_im))
 *   p    = fma(x_im, x_im, fma(x_re, x_re, p))
 *   g_re = (mu e_re) / (p + delta), g_im = (mu e_im) / (p + delta): a product, a sum and a correctly rounded quotient
 *   w_re = fma(g_im, x_im, fma(g_re, x_re, w_re))          w_im = fma(-g_re, x_im, fma(g_im, x_re, w_im))
 * with w = w_q and x = x[m - q].  On this order rest the bitwise properties:
 *   - no bit of e, y or the weights depends on how the frames are grouped into calls, down to calls of one frame and empty calls;
 *   - no bit depends on what any other (channel, bin) holds: a NaN in one bin of one channel stays there (llz_adapt_mc isolates
 *     channels; this isolates every bin of every channel);
 *   - no bit depends on whether the caller's pointers are host or device memory;
 *   - reset(1) followed by the same input repeats a fresh handle's bits.
 *
 * One kernel launch per call, whatever its frames: a lane owns one (channel, bin) and walks the call's frames with its weights and
 * history in registers.
 */
#ifndef LLZ_ADAPT_BANDS_H
#define LLZ_ADAPT_BANDS_H

#ifdef __cplusplus
extern "C" {
#endif

/* channels 1..65535; bins 1..4097; taps 1..64; mu in [0, 2], the step size of every channel (0 = frozen); delta > 0 and finite,
 * the regularisation of step 3 in units of |x|^2 (1e-3 x taps suits bands of unit variance).  Device memory: channels x taps x
 * bins x 8 bytes of weights, channels x max(taps - 1, 1) x bins x 8 of history, channels x 4 of step sizes; when an allocation
 * fails the message states the bytes asked for.  Every refusal leaves a message of its own.  Returns the handle or
 * (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_adapt_bands_mc_init(int channels, int bins, int taps, float mu, float delta);
void llz_adapt_bands_mc_uninit(unsigned long h);
/* x (reference), d (desired), e (error out), y (filter output; yre and yim both NULL or both set): [channels][frames][bins]
 * float32, device memory (used in place, asynchronous on the handle's stream) or host memory (staged, synchronous).  frames = 0
 * returns 0 and touches nothing.  Refused with LLZ_ERR_ARG, the handle left where it was: a device range of an output that
 * overlaps an input or another output, and frames x bins beyond 2^31 - 1.  Returns frames, or a negative LLZ_ERR_* code. */
int  llz_adapt_bands_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                        float *eim, float *yre, float *yim, int frames);
/* the step sizes of channels [first, first + count): mu = HOST [count], each in [0, 2], 0 = frozen; ordered on the handle's
 * stream behind the calls already issued */
int  llz_adapt_bands_mc_set_step(unsigned long h, int first, int count, const float *mu);
/* the weights of channels [first, first + count): wre, wim = HOST [count][taps][bins], row q the taps of age q; the history is
 * kept; ordered on the stream */
int  llz_adapt_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim);
/* the weights of channels [first, first + count) in the same layout, downloaded behind the calls already issued: the handle's
 * own float32 values, bit for bit */
int  llz_adapt_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim);
/* the history to zeros and the frame count to 0; clear_taps != 0: the weights to zero as well -- the state of a fresh handle but
 * for the step sizes --, else they are kept */
int  llz_adapt_bands_mc_reset(unsigned long h, int clear_taps);
/* *out = the frames taken since the init or the last reset */
int  llz_adapt_bands_mc_frames(unsigned long h, long long *out);
/* out = {tap ceiling of the kernel instance (4, 8, 16, 32 or 64), threads per workgroup, workgroups, launches per call}; nothing
 * is launched */
int  llz_adapt_bands_mc_plan(unsigned long h, int out[4]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_adapt_bands_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
