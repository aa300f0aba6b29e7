/*
 * include/llz_dft.h -- batched DFT of ANY length and zoom transform, C ABI of libllzfilter_hip.so: Bluestein's chirp-z algorithm
 * (Bluestein 1970; Rabiner, Schafer and Rader 1969) on the library's power-of-two transforms.  The reference has no counterpart.
 * All data is float32; complex values are interleaved re, im.  N is the transform length, w[n] an optional window (all ones
 * until llz_dft_mc_set_window says otherwise).
 *
 *   forward        X[k] = sum_{n < N} w[n] x[n] e^{-2 pi i n k / N},  k < N             complex rows in, complex rows out
 *   inverse        x[n] = w[n] (1 / N) sum_{k < N} X[k] e^{+2 pi i n k / N}             complex rows in, complex rows out
 *   real forward   the forward sum on real rows                                         real rows in, bins 0 .. N / 2 out
 *   real inverse   the inverse of the Hermitian extension of N / 2 + 1 bins             bins in, real rows out
 *   zoom           X[k] = sum_{n < N} w[n] x[n] e^{-2 pi i (f0 + k df) n},  k < K       complex or real rows in, complex out
 *
 * (N / 2 rounds down.)  The real inverse drops the imaginary part of bin 0 and, for even N, that of bin N / 2.  f0 and df are
 * in cycles per sample.  The window multiplies the time side: the input of forward and zoom transforms, the output of inverse
 * ones; it is folded into a table on the host and costs nothing at run time.
 *
 * Algorithm.  With c(m) = e^{-i pi m^2 / N} (zoom: e^{-2 pi i df m^2 / 2}) and M the smallest power of two with M >= N + K - 1
 * and M >= 8 (K = N for the DFT):  a[n] = x[n] w[n] c(n) (zoom: times e^{-2 pi i f0 n}), zeros up to M;  A = FFT_M(a);
 * B = A V, V = FFT_M(v) / M, v[m] = conj c(m) for 0 <= m < K, v[M - m] = conj c(m) for 1 <= m < N;  b = IFFT_M(B);
 * X[k] = b[k] c(k).  The inverse takes the conjugate tables with w[n] / N folded into the last one.  Every table is built in
 * double -- the DFT's phases from (m m mod 2 N) / (2 N) in 64-bit integers, the zoom's from the fractional part of df m^2 / 2 --
 * and rounded to float once.  Forms: M <= 4096 (every DFT with N <= 2048, every zoom) runs as ONE launch with each row in LDS
 * from load to store; longer DFTs run composed of the library's transforms on a device scratch of M complex values per row,
 * `count` walked in slabs under a scratch cap of 256 MiB.  llz_dft_mc_plan tells which; llz_dft_mc_configure overrides both.
 *
 * Error.  u = 2^-24, |x| the 2-norm of the windowed input row:  |X[k] - exact| <= 8 u log2(M) sqrt(N + K) |x| for every bin
 * (inverse transforms: divided by N), and a relative RMS error of dense rows below 1e-5 (measured: DESIGN.md).
 *
 * THE BITS OF A ROW'S OUTPUT DEPEND ON NOTHING BUT THAT ROW, the tables and the form: not on count, the row's place in the
 * batch, its neighbours (a NaN stays in its row), the pitches, or where the buffers live.
 */
#ifndef LLZ_DFT_H
#define LLZ_DFT_H

#ifdef __cplusplus
extern "C" {
#endif

enum { LLZ_DFT_FUSED = 0, LLZ_DFT_COMPOSED };

/* n in 2 .. 1048576.  Returns the handle or (unsigned long)-1 with a message (llz_hip_last_error). */
unsigned long llz_dft_mc_init(int n);
/* n >= 1 samples in, k >= 1 bins out, n + k - 1 <= 4096; f0, df finite, |df| <= 0.5 */
unsigned long llz_czt_mc_init(int n, int k, double f0, double df);
/* the calls below take the handles of both inits, except where they say otherwise */
void llz_dft_mc_uninit(unsigned long h);
int  llz_dft_mc_set_stream(unsigned long h, void *stream);
/* w: HOST, n floats, NULL for all ones.  Rebuilds the tables the window is folded into, ordered on the stream behind the calls
 * already issued. */
int  llz_dft_mc_set_window(unsigned long h, const float *w);
/* Measurement and tests: composed 1 = the composed form even where the fused kernel would be taken (M <= 4096), 0 = the
 * library's own choice; scratch_mb = the cap in MiB of the scratch the composed form walks `count` under (a row at the least;
 * negative: the library's 256).  A change of form rebuilds the chirp's spectrum in the other form's order, ordered on the stream
 * behind the calls already issued; the window stays. */
int  llz_dft_mc_configure(unsigned long h, int composed, int scratch_mb);
/* out = {form LLZ_DFT_*, M, rows per workgroup, LDS bytes per workgroup (both 0 for the composed form), slabs a call of `count`
 * rows walks as the handle is configured now}; nothing is launched */
int  llz_dft_mc_plan(unsigned long h, int count, int *out);

/* The transforms, all out of place: `count` >= 1 rows, row r at in + r in_pitch and out + r out_pitch, the pitches counted in
 * elements of the buffer's own kind (complex pairs or real floats).  in_pitch >= 1: INPUT ROWS MAY OVERLAP (a hop of samples
 * turns the real forward call into STFT analysis of any frame length).  out_pitch is at least the output row's length; what lies
 * between a row's end and the next row stays untouched.  Device or host memory (host memory is staged); real rows need 4-byte
 * alignment, complex rows 8-byte.  LLZ_ERR_ARG with a message and the handle unchanged for: a handle of the other init, a short
 * out_pitch, count < 1, device input and output ranges that overlap, device memory of another GPU. */
/* llz_dft_mc_init handles: rows of n complex -> n complex */
int  llz_dft_mc_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);
int  llz_dft_mc_inverse(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);
/* n real -> n / 2 + 1 complex, and back */
int  llz_dft_mc_real_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);
int  llz_dft_mc_real_inverse(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);
/* llz_czt_mc_init handles: rows of n complex (real) -> k complex */
int  llz_czt_mc_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);
int  llz_czt_mc_real_forward(unsigned long h, const float *in, long in_pitch, float *out, long out_pitch, int count);

#ifdef __cplusplus
}
#endif
#endif
