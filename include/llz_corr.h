/*
 * include/llz_corr.h -- auto / cross correlation, C ABI of libllzfilter_hip.so (the first caller
 * of llz_fft + llz_ifft back to back with a pointwise step in between, the same shape as the overlap-save FIR).
 * Part 1: the reference's symbols (reference libllzfilter/llz_corr.h, llz_corr.c:38-177), host `double` buffers, computed
 *         on the GPU in the reference's operation order: bit-identical results.
 * Part 2: many frames at once, float32, planar [frames][n] -> [frames][p+1] (cross-correlation: or [frames][2p+1]).
 */
#ifndef LLZ_CORR_H
#define LLZ_CORR_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Part 1: reference-identical symbols ---- */
/* r[k] = sum_{i} x[i]*x[i+k], k = 0..p (r has p+1 entries): llz_corr.c:38-47 */
void   llz_autocorr(double *x, int n, int p, double *r);
/* r[k] = sum_{i} x[i]*y[i+k]: llz_corr.c:49-58 */
void   llz_crosscorr(double *x, double *y, int n, int p, double *r);
/* <a,b> / sqrt(<a,a><b,b>): llz_corr.c:61-78 */
double llz_corr_cof(double *a, double *b, int len);
/* FFT autocorrelation, llz_corr.c:99-177: fft_len = 2^ceil(log2(2n)); NOTE the reference squares only the first n
 * spectrum bins and doubles the result -- kept, it is the reference's definition of this function. n <= 2048. */
unsigned long llz_autocorr_fast_init(int n);
void          llz_autocorr_fast_uninit(unsigned long handle);
void          llz_autocorr_fast(unsigned long handle, double *x, int n, int p, double *r);

/* ---- Part 2: batch extension, float32 ---- */
/* direct form for `frames` independent frames of n samples: r[f][k] = sum_i x[f][i]*x[f][i+k], k = 0..p.
 * x: planar [frames][n], r: planar [frames][p+1]; device or host pointers; p < n, p <= 255. out may not overlap in
 * (device memory): r overlapping x is refused with LLZ_ERR_ARG. Returns 0 or < 0. */
int llz_autocorr_mc(const float *x, float *r, int frames, int n, int p, void *stream);
/* FFT form with the reference's definition (first n bins, doubled), n <= 2048; out may not overlap in (device memory) */
unsigned long llz_autocorr_fast_mc_init(int frames, int n);
void          llz_autocorr_fast_mc_uninit(unsigned long handle);
int           llz_autocorr_fast_mc(unsigned long handle, const float *x, float *r, int p);
int           llz_autocorr_fast_mc_set_stream(unsigned long handle, void *stream);

/* r[f][k] = sum_i x[f][i] * y[f][i+k]  (llz_corr.c:49-58, the reference's definition), float32, planar.
 * two_sided = 0: r is [frames][p+1], lags 0..p.
 * two_sided = 1: r is [frames][2p+1], lag k in -p..p at index p+k, with r[-k] = sum_i y[f][i] * x[f][i+k].
 * x, y: [frames][n]; device or host pointers, each on its own; 0 <= p < n, p <= 255.
 * x == y is allowed and gives the autocorrelation (the bits of llz_autocorr_mc). r overlapping x or y in device memory is
 * refused with LLZ_ERR_ARG. Returns 0 or < 0. */
int llz_crosscorr_mc(const float *x, const float *y, float *r, int frames, int n, int p, int two_sided, void *stream);

/* c[f] = <a,b> / sqrt(<a,a><b,b>)  (llz_corr.c:61-78) for `frames` pairs of n samples; c: [frames]; float32 sums, the quotient in
 * double. A frame in which a or b is silent gives NaN (0/0), as the reference does, and touches no other frame. c overlapping
 * a or b in device memory is refused with LLZ_ERR_ARG. */
int llz_corr_cof_mc(const float *a, const float *b, float *c, int frames, int n, void *stream);

/* FFT form for wide lag ranges: the true linear cross-correlation through fft_len = 2^ceil(log2(2n)) (no wrap for |k| <= n-1;
 * NOT the first-n-bins quirk of llz_autocorr_fast, which has no cross counterpart in the reference). 4 <= n <= 2048,
 * 0 <= p <= n-1; x, y, r laid out as for llz_crosscorr_mc, device or host pointers; r may not overlap x or y (device memory). */
unsigned long llz_crosscorr_fast_mc_init(int frames, int n);
void          llz_crosscorr_fast_mc_uninit(unsigned long handle);
int           llz_crosscorr_fast_mc(unsigned long handle, const float *x, const float *y, float *r, int p, int two_sided);
int           llz_crosscorr_fast_mc_set_stream(unsigned long handle, void *stream);

#ifdef __cplusplus
}
#endif
#endif
