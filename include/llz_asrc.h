/*
 * include/llz_asrc.h -- arbitrary-ratio sample-rate conversion for many channels, C ABI of libllzfilter_hip.so: llz_asrc_mc, a
 * float32 band-limited interpolator whose step -- input samples per output sample -- is set PER CHANNEL and may GLIDE while the
 * signals run.  It is what llz_resample_mc (llz_resample.h: one fixed L/M per handle) cannot be: a resampler with a ratio such as
 * 1.000023 in front of llz_adapt_mc, nudged by a rate-control loop while playback and capture clocks drift apart; varispeed and
 * Doppler for moving paths; 44.1 kHz and 48 kHz devices side by side in one batch.  The reference has no counterpart; the
 * checker is a float64 model written from the definition below (tests/asrc_checks.py).
 *
 * THE DEFINITION
 *
 * Table.  T taps per phase (even, 4..128), PHI phases (a power of two, 256..4096), cutoff in (0, 1] as a fraction of the input's
 * Nyquist frequency, gain and window as in llz_resample_mc_init.  The prototype is h = llz_fir_lpf_cof(PHI T + 1, cutoff / PHI,
 * win), in double, times gain PHI.  G[p][k] = float32(h[k PHI + p]) for p = 0 .. PHI (PHI + 1 rows) and k < T; an index past the
 * end of h gives 0; every entry is rounded once.  (Row PHI is row 0 moved by one tap.)
 *
 * Time is unsigned Q32.32, in input samples; the first input sample since init or reset is at time 0.  A channel has a step inc =
 * llround(step 2^32), step finite and in [1/16, 16] (LLZ_RATIO_MAX).  Output j of a channel is taken at t_j, t_0 = 0, t_(j+1) =
 * t_j + inc_j, all in integers.
 *
 * Output.  For output j: n = t_j >> 32; p = the top log2 PHI bits of the fraction; a = the remaining 32 - log2 PHI bits times
 * 2^-(32 - log2 PHI) (at most 24 bits: exact in float32);
 *     c_k = G[p][k] + a (G[p+1][k] - G[p][k])          y_j = sum_{k < T} x[n + T/2 - k] c_k
 * with samples before the stream's start zero.  Arithmetic is float32 in a fixed order: d = G[p+1][k] - G[p][k] (one rounding),
 * c_k = fma(a, d, G[p][k]), y = fma(x, c_k, y) for k ascending from y = +0.  No bit of an output depends on how the stream is
 * cut into calls, on the other channels, or on the table form the handle runs.
 *
 * Delivery.  The first call at whose end input sample n + T/2 has been received delivers output j: the latency is T/2 input
 * samples.  The count of outputs of a call differs per channel; it is a pure function of the integer state, and the host layer
 * computes it without a device round trip.
 *
 * Glide.  set_step(target, R) with R >= 1: from the channel's next output on inc_j = inc_start + j dinc for j < R, dinc =
 * (target_inc - inc_start) / R as a signed integer division that truncates toward zero; from the R-th output on inc = target_inc
 * exactly.  Within the glide t_j = t_0 + j inc_start + dinc j (j - 1) / 2: every output is computed independently and exactly.
 * R = 0 switches at once; a set_step during a glide starts a new one from the current inc; a glide may span calls; R <= 2^31 - 1.
 *
 * Why no intermediate overflows to a wrong value.  The library keeps a channel's time relative to the buffer of the next call
 * ([T - 1 history samples | input]) and the count of samples received apart, so that time is below (2^22 + 128) 2^32 < 2^55 when a
 * call starts.  Every step inside a glide lies between inc_start and target_inc (the truncation keeps |R dinc| <= |target_inc -
 * inc_start|), hence in [2^28, 2^36].  The closed form is evaluated for j <= 2^27 + 1025 only (a call delivers at most
 * (2^22 + 128) 16 outputs and the search for the count looks no further than (bound - t_0) / 2^28 + 1); for such j the true t_j
 * is at most 2^55 + j 2^36 < 2^64.  The terms j inc_start and dinc j (j - 1) / 2 may each wrap modulo 2^64 (j (j - 1) / 2 itself
 * is exact, j < 2^31), but their sum is the true value modulo 2^64 and the true value is below 2^64: it is the true value.
 */
#ifndef LLZ_ASRC_H
#define LLZ_ASRC_H

#include "llz_fir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* channels 1..65535; frame_len 1..2^22, the longest n_in; taps even in 4..128; phases a power of two in 256..4096; cutoff in
 * (0, 1]; gain finite and not 0; win HAMMING, BLACKMAN or KAISER; step in [1/16, 16], every channel's step.  The cutoff does not
 * follow the step: the caller picks it for the largest step in use (1 / step, less a margin, for steps above 1).  Every refusal
 * leaves a message of its own naming the range missed.  Returns the handle or (unsigned long)-1. */
unsigned long llz_asrc_mc_init(int channels, int frame_len, int taps, int phases, double cutoff, double gain, win_t win, double step);
void llz_asrc_mc_uninit(unsigned long h);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_asrc_mc_set_stream(unsigned long h, void *stream);
/* in: planar [channels][n_in] float32, 0 <= n_in <= frame_len; out: rows of out_pitch elements, row c receives its count_c
 * outputs and elements [count_c, out_pitch) are never written; counts: HOST int[channels], may be NULL.  Device memory is used in
 * place, asynchronous on the handle's stream -- no copy and no synchronisation in either direction --, host memory is staged.  If
 * any channel's count exceeds out_pitch the call is refused before anything is launched and the handle is exactly as it was
 * (llz_asrc_mc_out_len gives the counts beforehand).  Device ranges of out that overlap in are refused.  Returns the largest
 * count, or a negative LLZ_ERR_* code.  A call launches with values of its own: graph capture is not supported. */
long llz_asrc_mc(unsigned long h, const float *in, long n_in, float *out, long out_pitch, int *counts);
/* the counts the next call of n_in samples would deliver (counts: HOST int[channels], may be NULL) and their largest as the
 * return value; nothing is launched and the state does not move */
long llz_asrc_mc_out_len(unsigned long h, long n_in, int *counts);
/* the steps of channels [first, first + count): step = HOST [count], each in [1/16, 16]; ramp = R of the definition, 0 ..
 * 2^31 - 1 outputs.  Ordered on the handle's stream behind the calls already issued; it takes effect with each channel's next
 * output. */
int  llz_asrc_mc_set_step(unsigned long h, int first, int count, const double *step, long ramp);
/* the step that follows each channel's next output, inc 2^-32 (exact in double), and, where ramp_left is not NULL, the outputs
 * its glide still has to run (0: none in flight) */
int  llz_asrc_mc_get_step(unsigned long h, int first, int count, double *step, long *ramp_left);
/* the time of each channel's next output: whole input samples since init or reset and the fraction in units of 2^-32 (frac may
 * be NULL).  A rate-control loop reads its fill level from this. */
int  llz_asrc_mc_next_time(unsigned long h, int first, int count, long long *whole, unsigned int *frac);
/* G of the definition, (phases + 1) x taps floats, to HOST dst; returns that number, or LLZ_ERR_ARG when capacity is less */
int  llz_asrc_mc_get_table(unsigned long h, float *dst, int capacity);
/* history to zeros, time to 0, running glides end at their targets: the state of a fresh handle with the current targets */
int  llz_asrc_mc_reset(unsigned long h);
/* out = {taps, phases, history samples kept per channel, table form: 0 = in LDS, 1 = read from global memory} */
int  llz_asrc_mc_plan(unsigned long h, int out[4]);

#ifdef __cplusplus
}
#endif
#endif
