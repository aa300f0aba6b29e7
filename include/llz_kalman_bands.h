/*
 * include/llz_kalman_bands.h -- adaptive filters in the bands of a filter bank that control their own step, C ABI of
 * libllzfilter_hip.so: llz_kalman_bands_mc, the diagonal state-space (Kalman) adaptive filter of K complex taps for every
 * (channel, bin) of a batch of band signals (Enzner and Vary's frequency-domain Kalman filter, 2006, in its subband form).  It
 * stands where llz_adapt_bands_mc (llz_adapt_bands.h) stands, between the analysis and the synthesis of a bank, and replaces that
 * filter's fixed step mu by a state variance P_q per tap and a tracked power psi of whatever in the error is not echo: the step
 * shrinks by itself while a near-end talker or noise dominates the error (double-talk) and opens again when the echo path moves,
 * so nobody has to detect double-talk and freeze the channel.  The reference has no counterpart; the checker is a float64 model
 * written from the definition below (tests/kalman_bands_checks.py).  One reference per band and no terms across bands.
 *
 * Signals are llz_adapt_bands_mc's: [channels][frames][bins] float32, re and im in arrays of their own; bins 1..4097.  K = taps,
 * 1..32 (a lane holds 5 K + 1 values of state; at 64 taps they no longer fit its registers).
 *
 * The state of a (channel c, bin k): weights w_q, q = 0 .. K - 1, complex, initially zero; a history x[m - q], zero before frame
 * 0; variances P_q >= 0, real, initially p0; a noise power psi >= 0, initially 0.  The parameters, all float32: a in (0, 1], the
 * state transition (0.999: how fast a forgotten path is assumed to drift); lam in [0, 1), the smoothing of psi (0.9); p0 > 0;
 * delta > 0.  Three constants are formed from them once, in float32: A2 = a a, omA2 = 1 - A2, oml = 1 - lam.  For frame m, in
 * order:
 *   1. y = sum_{q < K} w_q x[m - q], a complex product, NO conjugate on w; e = d[m] - y, one float32 subtraction per component.
 *      Both exactly as llz_adapt_bands_mc forms them.  e is always stored, y when the caller passes buffers for it.
 *   2. If the channel adapts (a flag per channel, on at init):
 *        psi <- lam psi + oml |e|^2
 *        u_q  = P_q |x[m - q]|^2                                  for every q < K
 *        s    = psi + delta + sum_{q < K} u_q,      r = 1 / s
 *        w_q <- w_q + (e r) P_q conj(x[m - q])
 *        c_q  = 1 - u_q r, and c_q = 0 where that is below 0
 *        P_q <- A2 c_q P_q + omA2 |w_q|^2                         with the NEW w_q
 *   3. A channel that does not adapt is FROZEN: step 2 is skipped, w, P and psi keep their bits, y and e are still produced -- with
 *      the bits llz_adapt_bands_mc gives at mu = 0 for the same taps.
 * Taps q >= K do not exist, whatever tap ceiling the kernel instance was built for (llz_kalman_bands_mc_plan).
 *
 * Arithmetic: float32 throughout, and the order of every sum is fixed in terms of the AGE q.  With fma(a, b, c) = a b + c rounded
 * once and every other operation rounded on its own, q ASCENDING:
 *   y_re = fma(-w_im, x_im, fma(w_re, x_re, y_re))         y_im = fma(w_im, x_re, fma(w_re, x_im, y_im))         from 0
 *   psi  = fma(lam, psi, oml * fma(e_im, e_im, e_re * e_re))
 *   u_q  = P_q * fma(x_im, x_im, x_re * x_re)
 *   s    = (psi + delta), then s = s + u_q for q = 0, 1, ..     r = 1 / s, the frame's one correctly rounded quotient
 *   g_re = e_re * r, g_im = e_im * r;  k_re = g_re * P_q, k_im = g_im * P_q               (P_q before its update)
 *   w_re = fma(k_im, x_im, fma(k_re, x_re, w_re))          w_im = fma(-k_re, x_im, fma(k_im, x_re, w_im))
 *   c_q  = 1 - u_q * r;  if (c_q < 0) c_q = 0              (a NaN stays a NaN)
 *   P_q  = fma(omA2, fma(w_im, w_im, w_re * w_re), (A2 * c_q) * P_q)
 * with w = w_q and x = x[m - q].  One reciprocal and products, not K + 2 quotients: a correctly rounded float32 quotient costs
 * about ten instructions, the clamp one (has both forms' times).
 *
 * P_q >= 0 and psi >= 0 always hold (as long as nothing overflows: inf 0 is a NaN, and a NaN stays one).  psi: lam >= 0, oml >= 0
 * (lam < 1), |e|^2 >= 0 as a sum of squares, and a rounded product or fma of non-negative values is never negative.  s >= delta
 * > 0 and s >= u_q, a monotone sum of non-negative terms.  P_q: u_q r <= s r, and with r = (1 / s)(1 + eps), |eps| <= 2^-24, the
 * exact s r = 1 + eps rounds to 1 at the most (the next float above 1 is 1 + 2^-23, and a tie goes to the even 1).  So c_q >= 0
 * wherever r is a normal number; where it is subnormal (s above 2^126) eps is larger, and there the clamp holds the invariant.  It
 * is part of the definition (and of the models).  With c_q >= 0, A2 >= 0, omA2 >= 0 (a <= 1, so A2 <= 1 after rounding) and
 * |w_q|^2 >= 0, P_q is an fma of non-negative values.  set_variance refuses anything else.
 *
 * On the fixed order rest the bitwise properties, llz_adapt_bands.h's: no bit of e, y, w, P or psi depends
 *   - on how the frames are grouped into calls, down to calls of one frame and empty calls;
 *   - on what any other (channel, bin) holds: a NaN in one bin of one channel stays there;
 *   - on whether the caller's pointers are host or device memory;
 * and reset(1) followed by the same input repeats a fresh handle's bits.
 *
 * One kernel launch per call, whatever its frames: a lane owns one (channel, bin) and walks the call's frames with its weights,
 * history and variances in registers.
 */
#ifndef LLZ_KALMAN_BANDS_H
#define LLZ_KALMAN_BANDS_H

#ifdef __cplusplus
extern "C" {
#endif

/* channels 1..65535; bins 1..4097; taps 1..32 (33..64, which llz_adapt_bands_mc takes, are refused with a message of their own);
 * a in (0, 1]; lam in [0, 1); p0 > 0 and finite; delta > 0 and finite, in units of |x|^2 like p0 |x|^2.  Suggested: 0.999, 0.9,
 * 1, 1e-3 for bands of unit variance.  Device memory: channels x taps x bins x 12 bytes of weights and variances, channels x
 * max(taps - 1, 1) x bins x 8 of history, channels x bins x 4 of noise powers, channels x 4 of flags; when an allocation fails
 * the message states the bytes asked for.  Every refusal leaves a message of its own.  Returns the handle or (unsigned long)-1
 * (llz_hip_last_error() says why). */
unsigned long llz_kalman_bands_mc_init(int channels, int bins, int taps, float a, float lam, float p0, float delta);
void llz_kalman_bands_mc_uninit(unsigned long h);
/* x (reference), d (desired), e (error out), y (filter output; yre and yim both NULL or both set): [channels][frames][bins]
 * float32, device memory (used in place, asynchronous on the handle's stream) or host memory (staged, synchronous).  frames = 0
 * returns 0 and touches nothing.  Refused with LLZ_ERR_ARG, the handle left where it was: a device range of an output that
 * overlaps an input or another output, and frames x bins beyond 2^31 - 1.  Returns frames, or a negative LLZ_ERR_* code. */
int  llz_kalman_bands_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim, float *ere,
                         float *eim, float *yre, float *yim, int frames);
/* whether channels [first, first + count) adapt: on = HOST [count], 0 = frozen, anything else = adapting; ordered on the
 * handle's stream behind the calls already issued */
int  llz_kalman_bands_mc_set_adapt(unsigned long h, int first, int count, const int *on);
/* the weights of channels [first, first + count): wre, wim = HOST [count][taps][bins], row q the taps of age q; the history, P
 * and psi are kept; ordered on the stream */
int  llz_kalman_bands_mc_set_taps(unsigned long h, int first, int count, const float *wre, const float *wim);
/* the weights of channels [first, first + count) in the same layout, downloaded behind the calls already issued: the handle's
 * own float32 values, bit for bit */
int  llz_kalman_bands_mc_get_taps(unsigned long h, int first, int count, float *wre, float *wim);
/* the variances of channels [first, first + count): p = HOST [count][taps][bins], every value finite and >= 0 (else refused,
 * nothing changed); everything else is kept; ordered on the stream.  Raising P is how a caller re-opens adaptation after a path
 * change it knows of */
int  llz_kalman_bands_mc_set_variance(unsigned long h, int first, int count, const float *p);
int  llz_kalman_bands_mc_get_variance(unsigned long h, int first, int count, float *p);
/* the noise powers psi of channels [first, first + count): psi = HOST [count][bins] */
int  llz_kalman_bands_mc_get_noise(unsigned long h, int first, int count, float *psi);
/* the history to zeros and the frame count to 0; clear != 0: w = 0, P = p0 and psi = 0 as well -- the state of a fresh handle but
 * for the adapt flags --, else they are kept */
int  llz_kalman_bands_mc_reset(unsigned long h, int clear);
/* *out = the frames taken since the init or the last reset */
int  llz_kalman_bands_mc_frames(unsigned long h, long long *out);
/* out = {tap ceiling of the kernel instance (4, 8, 16 or 32), threads per workgroup, workgroups, launches per call}; nothing is
 * launched */
int  llz_kalman_bands_mc_plan(unsigned long h, int out[4]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_kalman_bands_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
