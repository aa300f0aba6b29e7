/*
 * include/llz_adapt.h -- adaptive FIR filters for many channels, C ABI of libllzfilter_hip.so: llz_adapt_mc, a partitioned-block
 * frequency-domain NLMS filter (PBFDAF, also called MDF) that TRACKS a response while the signals run -- echo, feedback and
 * crosstalk cancellation per microphone, online identification of a room or cabinet, keeping the taps of a llz_fir_stream_mc or
 * llz_fir_matrix_mc handle up to date from a reference x and a microphone signal d.  The reference has no counterpart; the
 * checker is a float64 model written from the definition below (tests/adapt_checks.py).  One reference per channel: where an
 * output hears several references at once, llz_adapt_matrix_mc (llz_adapt_matrix.h) is the form to use.
 *
 * It is the stream convolver of llz_fir.h part 5 -- the same block, partitions, ring of input spectra and kernel walk -- plus
 * an error, a normalised gradient and a constrained weight update on the same ring.
 *
 * The algorithm, per channel: block B, N = 2 B, P = ceil(flt_len / B) partitions.  X_q is the N-point DFT (unnormalised, e^-j)
 * of input blocks (q - 1, q) of x, kept in a ring of R = P + k - 1 slots, k the blocks per call of the init's frame_len.  W_p is
 * the spectrum of partition p of the weights; the initial weights are zero.  For block j, in order:
 *   1. X_j is computed and written into the ring.
 *   2. Y = sum_{p < P} X_{j-p} W_p, p ascending; y_j = the last B samples of IDFT_N(Y).
 *   3. e_j = d_j - y_j, a float32 subtraction per sample.  e is always stored, y when the caller passes a buffer for it.
 *   4. If the channel's mu is not zero: E = DFT_N([0_B, e_j]); D_k = sum_{p < P} |X_{j-p,k}|^2, taken in the same walk of the
 *      ring as step 2 (there is no smoothed power state); G_k = mu E_k / (D_k + delta).
 *   5. For every p: dW_p = conj(X_{j-p}) G; THE GRADIENT CONSTRAINT: dw = IDFT_N(dW_p), every sample t >= min(B, flt_len - p B)
 *      set to zero -- the second half, and in the last partition also what lies beyond flt_len --, dW_p = DFT_N(dw); W_p += dW_p.
 * The filter therefore has exactly flt_len taps.  Only this constrained form exists: with this normalisation the unconstrained
 * one does not converge to the taps.  A channel whose mu is 0 is FROZEN: steps 4 and 5 are skipped, its weights keep their
 * bits, and for given weights its y has the bits of llz_fir_stream_mc with those taps.
 *
 * Arithmetic: float32 throughout, spectra in the stream convolver's packed layout (DC and Nyquist are two real bins in the
 * product, the power and the quotient); the summation orders are fixed, so the same calls give the same bits, and how calls
 * group the blocks of a stream does not change a bit.  A channel's values depend on that channel's x and d alone.
 *
 * Two kernel launches per block (filter, update) on the handle's stream, with the ring slot passed by value: a call CAPTURED
 * INTO A GRAPH would replay one and the same slot -- graph capture is not supported, as for llz_fir_stream_mc.
 */
#ifndef LLZ_ADAPT_H
#define LLZ_ADAPT_H

#ifdef __cplusplus
extern "C" {
#endif

/* channels 1..65535; block a power of two in 64..2048 (4096 is refused: the kernels would not fit their registers); frame_len =
 * k x block, k >= 1, the longest call; flt_len 1..131073; mu in [0, 2], the step size of every channel (0 = frozen);
 * delta > 0 and finite, the regularisation of step 4 in units of |X|^2 (1e-3 x block suits signals of unit variance).  Device
 * memory: channels x P x block x 8 bytes of weights, channels x R x block x 8 of ring, channels x block x 12 of last block and
 * gradient scratch; when an allocation fails the message states the bytes asked for.  Every refusal leaves a message of its own.
 * Returns the handle or (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_adapt_mc_init(int channels, int block, int frame_len, int flt_len, float mu, float delta);
void llz_adapt_mc_uninit(unsigned long h);
/* x (reference), d (desired), e (error out), y (filter output, may be NULL): planar [channels][frame_len] float32, device memory
 * (used in place, asynchronous on the handle's stream) or host memory (staged, synchronous); frame_len a multiple of block, at
 * most the init's.  Device ranges of e or y that overlap x, d or each other are refused (LLZ_ERR_ARG).  Returns frame_len, or a
 * negative LLZ_ERR_* code. */
int  llz_adapt_mc(unsigned long h, const float *x, const float *d, float *e, float *y, int frame_len);
/* the step sizes of channels [first, first + count): mu = HOST [count], each in [0, 2], 0 = frozen; ordered on the handle's
 * stream behind the calls already issued */
int  llz_adapt_mc_set_step(unsigned long h, int first, int count, const float *mu);
/* the weights of channels [first, first + count): taps = HOST [count][flt_len]; the delay line is kept; ordered on the stream */
int  llz_adapt_mc_set_taps(unsigned long h, int first, int count, const float *taps);
/* the weights of channels [first, first + count) as taps: HOST [count][flt_len].  The weights' spectra are downloaded behind the
 * calls already issued and each partition is inverted on the host in double; its first min(block, flt_len - p block) samples
 * are the taps, rounded to float once. */
int  llz_adapt_mc_get_taps(unsigned long h, int first, int count, float *taps);
/* the delay line (ring and last block) to zeros; clear_taps != 0: the weights to zero as well -- the state of a fresh handle
 * but for the step sizes --, else they are kept */
int  llz_adapt_mc_reset(unsigned long h, int clear_taps);
/* out = {N = 2 block, P = ceil(flt_len / block), ring slots R, blocks per call k of the init's frame_len}; nothing is launched */
int  llz_adapt_mc_plan(unsigned long h, int out[4]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_adapt_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
