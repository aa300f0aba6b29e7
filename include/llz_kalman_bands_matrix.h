/*
 * include/llz_kalman_bands_matrix.h -- multi-reference adaptive filters in the bands of a filter bank that control their own
 * step, C ABI of libllzfilter_hip.so: llz_kalman_bands_matrix_mc, the diagonal state-space (Kalman) adaptive filter of I
 * references x K complex taps for every (output, bin) of a batch of band signals.  It is to llz_kalman_bands_mc
 * (llz_kalman_bands.h) what llz_adapt_bands_matrix_mc (llz_adapt_bands_matrix.h) is to llz_adapt_bands_mc: a microphone that hears
 * several loudspeakers cannot be served by a bank of single-reference Kalman filters, each of which takes the other references'
 * echo for near-end noise -- its psi swallows that echo and its step closes.  Here every output's error drives all its paths at
 * once, with a state variance per path and tap and ONE tracked noise power per (output, bin): stereo and surround echo
 * cancellation in the bands that survives double-talk unattended, a noise canceller with several references.  Its e and y are
 * what llz_suppress_bands_mc (llz_suppress_bands.h) consumes.  The reference has no counterpart; the checker is a float64 model
 * written from the definition below (tests/kalman_bands_matrix_checks.py).  No terms across bands, no decorrelation of the
 * references, a DIAGONAL state covariance: the cross terms between paths are not tracked.
 *
 * I = inputs, 1..8; O = outputs, 1..4096; bins 1..4097; K = taps, 1..32; I K <= 32 (a lane holds 5 I K + 1 values of state, which
 * is llz_kalman_bands_mc's register argument; llz_adapt_bands_matrix_mc takes up to 64 entries).  Signals are band signals in
 * llz_stft_mc's layout, float32, re and im in arrays of their own: x is [inputs][frames][bins]; d, e, y are
 * [outputs][frames][bins].
 *
 * The state.  Every (output o, bin k) holds weights w_{i,q}, i < I, q < K, complex, initially zero; variances P_{i,q} >= 0, real,
 * initially p0; one noise power psi >= 0, initially 0.  Every (input i, bin k) holds ONE history x_i[m - q], zero before frame 0,
 * shared by all outputs; frames are counted from the init or the last reset.  The parameters, all float32, are
 * llz_kalman_bands_mc's: a in (0, 1], lam in [0, 1), p0 > 0, delta > 0.  Three constants are formed from them once, in float32:
 * A2 = a a, omA2 = 1 - A2, oml = 1 - lam; delta is the caller's delta as float32, added to psi when s is started.  For frame m, in
 * order:
 *   1. y = sum_{q < K} sum_{i < I} w_{i,q} x_i[m - q], a complex product, NO conjugate on w; e = d[m] - y, one float32
 *      subtraction per component.  e is always stored, y when the caller passes buffers for it.
 *   2. If the output adapts (a flag per output, on at init):
 *        psi     <- lam psi + oml |e|^2
 *        u_{i,q}  = P_{i,q} |x_i[m - q]|^2                        for every i < I, q < K
 *        s        = psi + delta + sum_{q < K} sum_{i < I} u_{i,q},      r = 1 / s
 *        w_{i,q} <- w_{i,q} + (e r) P_{i,q} conj(x_i[m - q])
 *        c_{i,q}  = 1 - u_{i,q} r, and c_{i,q} = 0 where that is below 0
 *        P_{i,q} <- A2 c_{i,q} P_{i,q} + omA2 |w_{i,q}|^2         with the NEW w_{i,q}
 *   3. An output that does not adapt is FROZEN: step 2 is skipped, w, P and psi keep their bits, y and e are still produced.  The
 *      shared history moves on whatever any output's flag says.
 * Entries beyond I K do not exist, whatever entry ceiling the kernel instance was built for (llz_kalman_bands_matrix_mc_plan).
 *
 * Arithmetic: llz_kalman_bands.h's, form for form, float32 throughout.  Every sum runs over the ENTRY j = q I + i: q ASCENDING,
 * and within a q, i ASCENDING.  With fma(a, b, c) = a b + c rounded once and every other operation rounded on its own:
 *   y_re = fma(-w_im, x_im, fma(w_re, x_re, y_re))         y_im = fma(w_im, x_re, fma(w_re, x_im, y_im))         from 0
 *   psi  = fma(lam, psi, oml * fma(e_im, e_im, e_re * e_re))
 *   u_j  = P_j * fma(x_im, x_im, x_re * x_re)
 *   s    = (psi + delta), then s = s + u_j for j = 0, 1, ..     r = 1 / s, the frame's one correctly rounded quotient
 *   g_re = e_re * r, g_im = e_im * r;  k_re = g_re * P_j, k_im = g_im * P_j               (P_j before its update)
 *   w_re = fma(k_im, x_im, fma(k_re, x_re, w_re))          w_im = fma(-k_re, x_im, fma(k_im, x_re, w_im))
 *   c_j  = 1 - u_j * r;  if (c_j < 0) c_j = 0              (a NaN stays a NaN)
 *   P_j  = fma(omA2, fma(w_im, w_im, w_re * w_re), (A2 * c_j) * P_j)
 * with w = w_{i,q}, P_j = P_{i,q} and x = x_i[m - q].  Contraction is off and every fma is written out.
 *
 * P_{i,q} >= 0 and psi >= 0 always hold (as long as nothing overflows), by llz_kalman_bands.h's argument with j in the place of
 * q: s is a monotone sum of non-negative terms from psi + delta > 0, so s >= u_j for every j and u_j r <= s r rounds to 1 at the
 * most wherever r is a normal number; elsewhere the clamp, which is part of the definition, holds c_j >= 0; and P_j is then an fma
 * of non-negative values.  set_variance refuses anything else.
 *
 * On the fixed order rest the bitwise properties:
 *   - with inputs = 1 every bit of e, y, w, P and psi is llz_kalman_bands_mc's for the same parameters;
 *   - a frozen output's e and y are llz_adapt_bands_matrix_mc's bits at mu = 0 for the same weights and history;
 *   - no bit of output o depends on how the frames are grouped into calls, down to calls of one frame and empty calls;
 *   - no bit of output o depends on the number of outputs, on any other output's d, flag or state, on what any other bin holds,
 *     or on whether the caller's pointers are host or device memory;
 *   - a NaN in bin k of any reference reaches bin k of every output (s is joint) and no other bin;
 *   - a reference that is zero throughout, its weights zero, leaves every value of e, y, psi and the other inputs' w and P equal
 *     (==) to those of a handle without that input: its terms add +-0 to y and 0 to s, and its own w stays 0;
 *   - reset(1) followed by the same input repeats a fresh handle's bits.
 *
 * One kernel launch per call, whatever its frames: a lane owns one (output, bin) and walks the call's frames with its weights,
 * the regressor and its variances in registers.  The shared history is never updated in place: a launch reads one of two buffers
 * and the lanes of output 0 write the other, which the next launch reads.
 */
#ifndef LLZ_KALMAN_BANDS_MATRIX_H
#define LLZ_KALMAN_BANDS_MATRIX_H

#ifdef __cplusplus
extern "C" {
#endif

/* inputs 1..8; outputs 1..4096; bins 1..4097; taps 1..32 with inputs x taps <= 32 (more is refused with a message of its own
 * that points to llz_adapt_bands_matrix_mc); a in (0, 1]; lam in [0, 1); p0 > 0 and finite; delta > 0 and finite, in units of
 * |x|^2 like p0 |x|^2.  Suggested: 0.999, 0.9, 1, 1e-3 for bands of unit variance.  Device memory: outputs x inputs x taps x bins
 * x 12 bytes of weights and variances, twice inputs x max(taps - 1, 1) x bins x 8 of history, outputs x bins x 4 of noise powers,
 * outputs x 4 of flags; when an allocation fails the message states the bytes asked for.  Every refusal leaves a message of its
 * own.  Returns the handle or (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_kalman_bands_matrix_mc_init(int inputs, int outputs, int bins, int taps, float a, float lam, float p0,
                                              float delta);
void llz_kalman_bands_matrix_mc_uninit(unsigned long h);
/* x (references): [inputs][frames][bins]; d (desired), e (error out), y (filter output; yre and yim both NULL or both set):
 * [outputs][frames][bins]; float32, device memory (used in place, asynchronous on the handle's stream) or host memory (staged,
 * synchronous), in any mix.  frames = 0 returns 0 and touches nothing.  Refused with LLZ_ERR_ARG, the handle left where it was: a
 * device range of an output that overlaps an input or another output, and frames x bins beyond 2^31 - 1.  Returns frames, or a
 * negative LLZ_ERR_* code. */
int  llz_kalman_bands_matrix_mc(unsigned long h, const float *xre, const float *xim, const float *dre, const float *dim,
                                float *ere, float *eim, float *yre, float *yim, int frames);
/* whether outputs [out_first, out_first + out_count) adapt: on = HOST [out_count], 0 = frozen, anything else = adapting; ordered
 * on the handle's stream behind the calls already issued */
int  llz_kalman_bands_matrix_mc_set_adapt(unsigned long h, int out_first, int out_count, const int *on);
/* the weights of the paths (out_first .. , in_first ..): wre, wim = HOST [out_count][in_count][taps][bins], row q the taps of
 * age q; the history, P and psi are kept; ordered on the stream */
int  llz_kalman_bands_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                         const float *wre, const float *wim);
/* the weights of those paths in the same layout, downloaded behind the calls already issued: the handle's own float32 values,
 * bit for bit */
int  llz_kalman_bands_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *wre,
                                         float *wim);
/* the variances of those paths: p = HOST [out_count][in_count][taps][bins], every value finite and >= 0 (else refused, nothing
 * changed); everything else is kept; ordered on the stream.  Raising P is how a caller re-opens adaptation after a path change it
 * knows of */
int  llz_kalman_bands_matrix_mc_set_variance(unsigned long h, int out_first, int out_count, int in_first, int in_count,
                                             const float *p);
int  llz_kalman_bands_matrix_mc_get_variance(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *p);
/* the noise powers psi of outputs [out_first, out_first + out_count): psi = HOST [out_count][bins] */
int  llz_kalman_bands_matrix_mc_get_noise(unsigned long h, int out_first, int out_count, float *psi);
/* the history to zeros and the frame count to 0; clear != 0: w = 0, P = p0 and psi = 0 as well -- the state of a fresh handle but
 * for the adapt flags --, else they are kept */
int  llz_kalman_bands_matrix_mc_reset(unsigned long h, int clear);
/* *out = the frames taken since the init or the last reset */
int  llz_kalman_bands_matrix_mc_frames(unsigned long h, long long *out);
/* out = {inputs of the kernel instance, entry ceiling of the instance (8, 16 or 32 >= inputs x taps), threads per workgroup,
 * workgroups, launches per call}; nothing is launched */
int  llz_kalman_bands_matrix_mc_plan(unsigned long h, int out[5]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_kalman_bands_matrix_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
