/*
 * include/llz_spectral.h -- Welch cross-spectra of many channel pairs, C ABI of libllzfilter_hip.so: the averaged power
 * spectra, cross-spectrum, coherence and H1 transfer-function estimate of recorded channels (the spectral side of llz_corr.h).
 * The reference has no counterpart; float32 transforms, float32 sums inside a run of frames, double across runs.
 *
 * Framing.  Frame f, counted from the last reset, covers samples [f hop, f hop + fft_len) of each channel's stream, is
 * multiplied by the float32 window table ((float) of llz_hamming / llz_blackman / llz_kaiser, as llz_stft_mc_init builds it)
 * and transformed: X_f[k], k = 0 .. fft_len / 2.  No zero padding and no zero history: nothing is summed before fft_len
 * samples have arrived.
 *
 * Sums, per pair (x, y) and bin k:  Sxx = sum_f |X_f|^2,  Syy = sum_f |Y_f|^2,  Sxy = sum_f conj(X_f) Y_f.  Inside a run of
 * LLZ_CSD_RUN consecutive frames they are added in float32 in frame order, as compensated (Kahan) sums: a run's sum is within
 * about one float32 rounding of the exact sum of its terms, which keeps the coherence of a fully coherent pair within 1 + 4 u,
 * u = 2^-24.  Runs sit on the absolute frame grid (run r = frames [32 r, 32 r + 32)) and a finished run is added to double
 * accumulators in run order.  A call that ends inside a run leaves the run's float32 partial, with its compensation terms, in
 * the handle and the next call continues it: THE BITS OF EVERY READ-OUT DO NOT DEPEND ON HOW THE
 * SAMPLES WERE SPLIT INTO CALLS.
 *
 * Read-outs, computed on the device in double and rounded once to float32; K = frames so far, U = sum_j w_j^2 (double, over
 * the float32 table):
 *   LLZ_SPEC_PXX / PYY   Sxx / (K U), Syy / (K U)
 *   LLZ_SPEC_CSD         Sxy / (K U), (re, im)
 *   LLZ_SPEC_COHERENCE   |Sxy|^2 / (Sxx Syy); NaN where Sxx Syy == 0 (a silent channel: NaN in its own pairs only)
 *   LLZ_SPEC_TF          Sxy / Sxx, the H1 estimate of the response from x to y, (re, im); NaN where Sxx == 0
 * PXX, PYY and CSD are TWO-SIDED values at bins 0 .. fft_len / 2: no one-sided doubling and no sample-rate scaling.
 */
#ifndef LLZ_SPECTRAL_H
#define LLZ_SPECTRAL_H

#include "llz_fir.h"     /* win_t */

#ifdef __cplusplus
extern "C" {
#endif

#define LLZ_CSD_RUN 32      /* frames summed in float32 before the sum goes to the double accumulators */
enum { LLZ_SPEC_PXX = 0, LLZ_SPEC_PYY, LLZ_SPEC_CSD, LLZ_SPEC_COHERENCE, LLZ_SPEC_TF };

/* channels >= 1; pairs >= 1; pair_xy: HOST [pairs][2], every entry in [0, channels): (a, b) is x = channel a against y =
 * channel b, (a, a) the Welch PSD of channel a, repeated pairs are allowed; fft_len a power of two in 64..4096, bins = fft_len /
 * 2 + 1; hop one of fft_len, fft_len / 2, fft_len / 4.  Returns the handle or (unsigned long)-1 with a message. */
unsigned long llz_csd_mc_init(int channels, int pairs, const int *pair_xy, int fft_len, int hop, win_t win_type);
void llz_csd_mc_uninit(unsigned long handle);
int  llz_csd_mc_set_stream(unsigned long handle, void *stream);
/* x: planar [channels][n], device or host memory (host memory is staged); n a multiple of hop, n >= hop.  The handle keeps the
 * last fft_len - hop samples of every channel on the device between calls.  Returns the frames summed so far, or < 0. */
long llz_csd_mc_update(unsigned long handle, const float *x, long n);
long llz_csd_mc_frames(unsigned long handle);
/* what: LLZ_SPEC_*; out: [pairs][bins] floats, CSD and TF [pairs][bins][2] = re, im; device or host memory.  Before the first
 * frame: LLZ_ERR_ARG. */
int  llz_csd_mc_read(unsigned long handle, int what, float *out);
/* the sums themselves: out [pairs][bins][4] doubles = Sxx, Syy, Re Sxy, Im Sxy; device or host memory */
int  llz_csd_mc_read_raw(unsigned long handle, double *out);
/* back to the state of a fresh handle: no frames, no history */
int  llz_csd_mc_reset(unsigned long handle);
/* what an update of n samples would run now, nothing launched: out = {form: 0 the staged LDS transform / 1 the register
 * transform, LLZ_CSD_RUN, runs per walk of the partial scratch, walks} */
int  llz_csd_mc_plan(unsigned long handle, long n, int out[4]);

#ifdef __cplusplus
}
#endif
#endif
