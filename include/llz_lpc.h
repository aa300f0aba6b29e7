/*
 * include/llz_lpc.h -- linear prediction by the autocorrelation method, C ABI of libllzfilter_hip.so.
 * Part 1: the reference's symbols (reference libllzfilter/llz_lpc.h:21-23, llz_lpc.c:19-95), host `double` buffers:
 *         llz_autocorr on the device in the reference's summation order, then llz_levinson: bit-identical results.
 * Part 2: many frames at once, float32 in, on the device, in one launch for p <= 32.
 * Part 3: the filters that apply part 2's coefficients on the device: residual A_f(z) and synthesis 1 / A_f(z).
 */
#ifndef LLZ_LPC_H
#define LLZ_LPC_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Part 1: reference-identical symbols ---- */
/* a handle of order p (llz_lpc.c:30-48): 0 <= p <= LLZ_LEVINSON_ORDER_MAX (64), else LLZ_BAD_HANDLE with a message; also
 * LLZ_BAD_HANDLE without a GPU (there is no CPU path) */
unsigned long llz_lpc_init(int p);
void          llz_lpc_uninit(unsigned long handle);
/* llz_lpc.c:69-95: r = llz_autocorr(x, x_len, p), llz_levinson on the handle's own r / acof / kcof, then
 * lpc_cof[0..p] = acof[0..p], kcof[0..p] = the handle's kcof[0..p] (p + 1 entries), *err = E_p / x_len; returns
 * r[0] / E_p, or 0 when E_p <= 0.  Kept from the reference: after a silent frame (r[0] == 0) lpc_cof[0], kcof[0] and
 * kcof[p] are whatever earlier calls on the same handle left in it (0 on a fresh handle).  x_len < 1, NULL arrays or a bad
 * handle are refused: message, outputs untouched, returns 0. */
double        llz_lpc(unsigned long handle, double *x, int x_len, double *lpc_cof, double *kcof, double *err);

/* ---- Part 2: batch extension, float32 ---- */
/* LPC analysis of `frames` independent frames of n samples (the autocorrelation method, llz_lpc per frame):
 * x planar [frames][n]; win NULL or [n] (applied as x*win in float32 before the correlation);
 * acof [frames][p+1] (acof[f][0] = 1), kcof [frames][p] (reference indexing kcof[0..p-1]), err [frames] (= E_p / n),
 * gain [frames] (= r0 / E_p, 0 when E_p <= 0), r [frames][p+1] (the float32 autocorrelation).
 * Every output but acof may be NULL.  Device or host pointers.  0 <= p <= 64, p < n.  Returns 0 or < 0.
 *
 * Arithmetic: r is llz_autocorr_mc's, bit for bit (same kernel code, same summation order).  The recursion runs in double
 * from (double) r[f][k] in llz_levinson's operation order (no contraction, IEEE division) and every output is rounded once
 * to float32: each frame's outputs are float32(llz_levinson((double) r)).  A silent frame (r[0] == 0) gives acof = [1, 0,
 * ...], kcof = 0, err = 0, gain = 0 -- unlike llz_lpc there is no handle, so no value carries over from another frame.
 * Nothing else is guarded: a recursion that divides by a zero error gives what the arithmetic gives, as in the reference.
 * p <= 32 computes the correlation and the recursion in one launch; 33 <= p <= 64 (and llz_hip_tune("lpc_split", 1))
 * runs llz_autocorr_mc's kernel and then the recursion as a second launch -- the same bits either way.
 * out may not overlap in (device memory): acof, kcof, err, gain or r overlapping x is refused with LLZ_ERR_ARG. */
int llz_lpc_mc(const float *x, const float *win, float *acof, float *kcof, float *err, float *gain, float *r,
               int frames, int n, int p, void *stream);

/* ---- Part 3: batch extension, the filters of a coefficient set per (channel, frame) ---- */
/* The prediction-error filter A_f(z) (residual) and the all-pole filter 1 / A_f(z) (synthesis) over `channels` planar
 * streams cut into frames of frame_len samples, each frame with its own coefficients: llz_levinson's sign convention,
 * A(z) = 1 + sum_{k=1..p} a[k] z^-k.  With f = t / frame_len the frame of sample t within the call and samples in front of
 * the stream's start taken as zero:
 *     residual:   e[t] = x[t] + sum_k a_f[k] x[t-k]          synthesis:   y[t] = e[t] - sum_k a_f[k] y[t-k]
 *
 * one handle serves both directions and keeps the state of each per channel (residual: the last p input samples,
 * float32; synthesis: the last p outputs, double), so consecutive calls continue the streams.
 * channels >= 1, 0 <= p <= LLZ_LEVINSON_ORDER_MAX (64), frame_len > p (llz_lpc_mc's p < n: a frame's history lies inside
 * the frame before it); otherwise LLZ_BAD_HANDLE with a message, as without a GPU (there is no CPU path). */
unsigned long llz_lpc_filter_mc_init(int channels, int frame_len, int p);
void          llz_lpc_filter_mc_uninit(unsigned long handle);
int           llz_lpc_filter_mc_set_stream(unsigned long handle, void *stream);
int           llz_lpc_filter_mc_reset(unsigned long handle);          /* both states back to zero */
/* x, e, y: planar [channels][frames*frame_len]; acof: [channels][frames][p+1] float32, exactly what
 * llz_lpc_mc(x, ..., frames = channels*frames, n = frame_len, p) writes for the same x.  acof[..][0] is taken as 1
 * and not read.  Device or host pointers, at a float's alignment.  frames >= 1, channels*frames and frames*frame_len fit
 * an int.  Return frames or < 0 (message through llz_hip_last_error()); a device output range that intersects a device
 * input range (e against x or acof; y against e or acof) is refused with LLZ_ERR_ARG and nothing is written.
 *
 * Arithmetic (part of the contract).  Residual, float32: acc = x[t]; for k = p, p-1, .., 1: acc = fmaf(a_f[k], x[t-k], acc);
 * e[t] = acc -- a sample depends on x[t-p..t] and a_f only, never on how frames were grouped into calls.  Synthesis, double:
 * acc = (double) e[t]; for k = p, p-1, .., 1: acc = acc - (double) a_f[k] * yd[t-k] (a rounded multiply, then a rounded
 * subtract); y[t] = (float) acc, and the unrounded acc enters the delay line yd, which stays in double in the handle between
 * calls.  Nothing is guarded: an unstable coefficient set gives what the arithmetic gives, as in llz_lpc_mc. */
int llz_lpc_residual_mc(unsigned long handle, const float *x, const float *acof, float *e, int frames);
int llz_lpc_synth_mc   (unsigned long handle, const float *e, const float *acof, float *y, int frames);

#ifdef __cplusplus
}
#endif
#endif
