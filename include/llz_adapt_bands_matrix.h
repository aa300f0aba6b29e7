/*
 * include/llz_adapt_bands_matrix.h -- multi-reference adaptive filters in the bands of a filter bank, C ABI of
 * libllzfilter_hip.so: llz_adapt_bands_matrix_mc, a normalised LMS filter of I references x K complex taps for every (output,
 * bin) of a batch of band signals, updated frame by frame at the band rate.  It is to llz_adapt_bands_mc (llz_adapt_bands.h) what
 * llz_adapt_matrix_mc is to llz_adapt_mc: a microphone that hears several loudspeakers cannot be served by a bank of
 * single-reference filters, each of which takes the other references' echo for noise and normalises by the wrong power.  Here
 * every output's error drives all its paths at once, normalised by the JOINT power of the references: stereo and surround echo
 * cancellation in the bands, a noise canceller with several references, a sidelobe canceller behind a blocking matrix.  Frozen
 * (mu = 0) and loaded by set_taps, the same handle is a filter-and-sum beamformer or mixer with a weight per bin,
 * y_o[m][k] = sum_i sum_q w_{o,i,q}[k] x_i[m - q][k]; with K = 1 an instantaneous one.  The reference has no counterpart; the
 * checker is a float64 model written from the definition below (tests/adapt_bands_matrix_checks.py).  No terms across bands, no
 * decorrelation of the references, no step-size control.
 *
 * I = inputs, 1..8; O = outputs, 1..4096; bins 1..4097; K = taps, 1..64; I K <= 64.  Signals are band signals in llz_stft_mc's
 * layout, float32, re and im in arrays of their own: x is [inputs][frames][bins]; d, e, y are [outputs][frames][bins].
 *
 * The algorithm.  Every (output o, bin k) holds weights w_{i,q}, i < I, q < K, complex, initially zero.  Every (input i, bin k)
 * holds ONE history x_i[m - q], zero before frame 0, shared by all outputs; frames are counted from the init or the last reset.
 * For frame m, in order:
 *   1. y = sum_{q < K} sum_{i < I} w_{i,q} x_i[m - q], a complex product, NO conjugate on w.
 *   2. e = d[m] - y, one float32 subtraction per component.  e is always stored, y when the caller passes buffers for it.
 *   3. If the output's mu is not zero: p = sum_{q < K} sum_{i < I} |x_i[m - q]|^2, the joint power of all references, taken from
 *      the history anew in every frame; g = mu e / (p + delta); w_{i,q} += g conj(x_i[m - q]) for every i, q.
 *   4. An output whose mu is 0 is FROZEN: step 3 is skipped, its weights keep their bits, y and e are still produced.
 * Entries beyond I K do not exist: whatever entry ceiling the kernel instance was built for (llz_adapt_bands_matrix_mc_plan), it
 * neither filters with them nor updates them.
 *
 * Arithmetic: float32 throughout.  With fma(a, b, c) = a b + c rounded once, every sum starts from 0 and runs over q ASCENDING,
 * and within a q over i ASCENDING, in the four forms of llz_adapt_bands.h:
 *   y_re = fma(-w_im, x_im, fma(w_re, x_re, y_re))         y_im = fma(w_im, x_re, fma(w_re, x_im, y_im))
 *   p    = fma(x_im, x_im, fma(x_re, x_re, p))
 *   g_re = (mu e_re) / (p + delta), g_im = (mu e_im) / (p + delta): a product, a sum and a correctly rounded quotient
 *   w_re = fma(g_im, x_im, fma(g_re, x_re, w_re))          w_im = fma(-g_re, x_im, fma(g_im, x_re, w_im))
 * with w = w_{i,q} and x = x_i[m - q].  On this order rest the bitwise properties:
 *   - with inputs = 1 every bit of e, y and the weights is llz_adapt_bands_mc's for the same taps, mu and delta;
 *   - no bit of output o depends on how the frames are grouped into calls, down to calls of one frame and empty calls;
 *   - no bit of output o depends on the number of outputs, on any other output's d or mu, on what any other bin holds, or on
 *     whether the caller's pointers are host or device memory;
 *   - a NaN in bin k of any reference reaches bin k of every output (the power is joint) and no other bin;
 *   - a reference that is zero throughout, its weights zero, leaves every value of e, y and the other weights equal (==) to
 *     those of a handle without that input;
 *   - reset(1) followed by the same input repeats a fresh handle's bits.
 *
 * One kernel launch per call, whatever its frames: a lane owns one (output, bin) and walks the call's frames with its weights and
 * the regressor in registers.  The shared history is never updated in place: a launch reads one of two buffers and the lanes of
 * output 0 write the other, which the next launch reads.
 */
#ifndef LLZ_ADAPT_BANDS_MATRIX_H
#define LLZ_ADAPT_BANDS_MATRIX_H

#ifdef __cplusplus
extern "C" {
#endif

/* inputs 1..8; outputs 1..4096; bins 1..4097; taps 1..64 with inputs x taps <= 64; mu in [0, 2], the step size of every output
 * (0 = frozen); delta > 0 and finite, the regularisation of step 3 in units of |x|^2 (1e-3 x inputs x taps suits bands of unit
 * variance).  Device memory: outputs x inputs x taps x bins x 8 bytes of weights, twice inputs x max(taps - 1, 1) x bins x 8 of
 * history, outputs x 4 of step sizes; when an allocation fails the message states the bytes asked for.  Every refusal leaves a
 * message of its own.  Returns the handle or (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_adapt_bands_matrix_mc_init(int inputs, int outputs, int bins, int taps, float mu, float delta);
void llz_adapt_bands_matrix_mc_uninit(unsigned long h);
/* x (references): [inputs][frames][bins]; d (desired), e (error out), y (filter output; yre and yim both NULL or both set):
 * [outputs][frames][bins]; float32, device memory (used in place, asynchronous on the handle's stream) or host memory (staged,
 * synchronous), in any mix.  frames = 0 returns 0 and touches nothing.  Refused with LLZ_ERR_ARG, the handle left where it was: a
 * device range of an output that overlaps an input or another output, and frames x bins beyond 2^31 - 1.  Returns frames, or a
 * negative LLZ_ERR_* code. */
int  llz_adapt_bands_matrix_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim,
                               float *ere, float *eim, float *yre, float *yim, int frames);
/* the step sizes of outputs [out_first, out_first + out_count): mu = HOST [out_count], each in [0, 2], 0 = frozen; ordered on
 * the handle's stream behind the calls already issued */
int  llz_adapt_bands_matrix_mc_set_step(unsigned long h, int out_first, int out_count, const float *mu);
/* the weights of the paths (out_first .. , in_first ..): wre, wim = HOST [out_count][in_count][taps][bins], row q the taps of
 * age q; the history is kept; ordered on the stream */
int  llz_adapt_bands_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                        const float *wre, const float *wim);
/* the weights of those paths in the same layout, downloaded behind the calls already issued: the handle's own float32 values,
 * bit for bit */
int  llz_adapt_bands_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *wre,
                                        float *wim);
/* the history to zeros and the frame count to 0; clear_taps != 0: the weights to zero as well -- the state of a fresh handle but
 * for the step sizes --, else they are kept */
int  llz_adapt_bands_matrix_mc_reset(unsigned long h, int clear_taps);
/* *out = the frames taken since the init or the last reset */
int  llz_adapt_bands_matrix_mc_frames(unsigned long h, long long *out);
/* out = {inputs of the kernel instance, entry ceiling of the instance (8, 16, 32 or 64 >= inputs x taps), threads per workgroup,
 * workgroups, launches per call}; nothing is launched */
int  llz_adapt_bands_matrix_mc_plan(unsigned long h, int out[5]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_adapt_bands_matrix_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
