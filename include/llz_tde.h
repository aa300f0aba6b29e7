/*
 * include/llz_tde.h -- streaming time-delay estimator of many channel pairs, C ABI of libllzfilter_hip.so: the generalised
 * cross-correlation (Knapp and Carter 1976) of two running signals on recursively averaged cross-spectra, with plain, phase
 * transform (PHAT) or smoothed coherence (SCOT) weighting, and per frame the lag of its peak with a sub-sample fraction.  The
 * reference has no counterpart; float32 transforms, float32 recursion, one launch per call.
 *
 * Framing.  Frame f, counted from the last reset, covers samples [f hop, f hop + fft_len) of each channel's stream, is
 * multiplied by the float32 window table ((float) of llz_hamming / llz_blackman / llz_kaiser) and transformed: X_f[k], Y_f[k],
 * k = 0 .. fft_len / 2, each channel on its own.  No zero padding and no zero history: nothing comes out before fft_len
 * samples have arrived.
 *
 * Recursion, per pair (x, y) and bin k, in float32 and in frame order, every product and sum rounded on its own:
 *   P_f = conj(X_f) Y_f,  gx_f = |X_f|^2,  gy_f = |Y_f|^2
 *   S_0 = P_0,  S_f = lam S_{f-1} + g P_f   (Gx, Gy likewise from gx, gy),  g = (float)(1 - (double)lam)
 * lam == 0 takes S_f = P_f without a product by zero.  A pair (a, a) has Im S == 0 exactly.  THE BITS OF EVERY OUTPUT DO NOT
 * DEPEND ON HOW THE SAMPLES WERE SPLIT INTO CALLS.
 *
 * Weighting over bins k_lo .. k_hi (W = 0 outside), delta absolute:
 *   LLZ_TDE_CC     W = S
 *   LLZ_TDE_PHAT   W = S / (|S| + delta)
 *   LLZ_TDE_SCOT   W = S / (sqrt(Gx Gy) + delta)
 * and W = 0 where the denominator is 0.
 *
 * Curve.  r_f[tau] = (1 / N) sum_{k < N} W~[k] e^{+2 pi i k tau / N}, W~ the Hermitian extension of W (the imaginary parts of
 * bins 0 and N / 2 are dropped), N = fft_len: y[t] = x[t - D0] PEAKS AT tau = +D0.
 *
 * Peak, L = max_lag:  tau* = argmax over tau in [-L, L] of r_f[tau], the lowest tau among equal values;  a, b, c = r_f[tau* - 1],
 * r_f[tau*], r_f[tau* + 1] (circular);  den = a - 2 b + c;  delay = tau* + (den < 0 ? clamp(0.5 (a - c) / den, -0.5, 0.5) : 0),
 * peak = b.  If any r_f[tau] in the range is NaN, delay and peak of that pair and frame are NaN.  A NaN (or an infinity) in a
 * channel STAYS IN THE STATE of the pairs that contain that channel until llz_tde_mc_reset, because lam NaN is NaN; it never
 * reaches another pair.
 */
#ifndef LLZ_TDE_H
#define LLZ_TDE_H

#include "llz_fir.h"     /* win_t */

#ifdef __cplusplus
extern "C" {
#endif

enum { LLZ_TDE_CC = 0, LLZ_TDE_PHAT, LLZ_TDE_SCOT };
enum { LLZ_TDE_CURVE = 0, LLZ_TDE_STATE };

/* channels >= 1; pairs >= 1; pair_xy: HOST [pairs][2], every entry in [0, channels), repeated pairs and (a, a) are allowed;
 * fft_len a power of two in 64..4096, bins = fft_len / 2 + 1; hop one of fft_len, fft_len / 2, fft_len / 4; max_lag in
 * 1 .. fft_len / 2 - 1; weight LLZ_TDE_*; 0 <= k_lo <= k_hi <= fft_len / 2; lam in [0, 1); delta >= 0.  Returns the handle or
 * (unsigned long)-1 with a message. */
unsigned long llz_tde_mc_init(int channels, int pairs, const int *pair_xy, int fft_len, int hop, win_t win_type,
                              int max_lag, int weight, int k_lo, int k_hi, float lam, float delta);
void llz_tde_mc_uninit(unsigned long h);
int  llz_tde_mc_set_stream(unsigned long h, void *stream);
/* frames a call of n samples would complete now; no launch */
long llz_tde_mc_frames_for(unsigned long h, long n);
/* x: planar [channels][n], device or host memory (host memory is staged); n a multiple of hop, n >= hop.  delay, peak:
 * [pairs][out_pitch], device or host, peak may be NULL: element j < frames written of row p is frame (frames before the call) + j
 * of pair p, elements [frames written, out_pitch) of every row stay untouched.  out_pitch below the call's frames, and device
 * outputs that overlap x or each other, are refused; a refused call leaves the handle where it was.  The handle keeps the last
 * fft_len - hop samples of every channel on the device.  Returns frames written by this call (>= 0) or < 0 */
long llz_tde_mc_process(unsigned long h, const float *x, long n, float *delay, float *peak, long out_pitch);
long llz_tde_mc_frames(unsigned long h);                       /* frames since the last reset */
/* LLZ_TDE_CURVE: [pairs][2 max_lag + 1] of the last frame, lags -max_lag .. max_lag;
 * LLZ_TDE_STATE: [pairs][bins][4] = Re S, Im S, Gx, Gy.  Device or host memory.  Before the first frame: LLZ_ERR_ARG. */
int  llz_tde_mc_read(unsigned long h, int what, float *out);
int  llz_tde_mc_set_forget(unsigned long h, float lam);        /* from the next frame on */
/* back to the state of a fresh handle: no frames, no history; lam stays */
int  llz_tde_mc_reset(unsigned long h);

#ifdef __cplusplus
}
#endif
#endif
