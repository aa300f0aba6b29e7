/*
 * include/llz_iir.h -- IIR filters, C ABI of libllzfilter_hip.so.
 * Part 1: the reference's direct-form-I single-channel `double` API (reference libllzfilter/llz_iir.h:24-27).
 * Part 2: multi-channel float32 cascade of second-order sections, fused in one kernel (SURVEY.md M4:
 * an "8-biquad cascade" is 8 chained reference handles with M=N=2).
 * Part 3: multi-channel float32 form of the general direct-form-I filter itself (any orders up to 8).
 * Part 4: the biquad bank: the cascade of part 2 with a coefficient set per channel.
 */
#ifndef LLZ_IIR_H
#define LLZ_IIR_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Part 1: reference-identical symbols (llz_iir.c:37-156) ---- */
/* a[0..M] poles (a[0] ignored, taken as 1), b[0..N] zeros (NULL = all zero). Host pointers. */
unsigned long llz_iir_filter_init(int M, double *a, int N, double *b);
void          llz_iir_filter_uninit(unsigned long handle);
int           llz_iir_filter(unsigned long handle, double *x, double *y, int frame_len);   /* returns frame_len */
int           llz_iir_filter_flush(unsigned long handle, double *y);                       /* N more samples of x=0; returns N */

/* ---- Part 2: multi-channel float32 biquad cascade ---- */
/* coef: HOST pointer, stages x 6 doubles {b0,b1,b2,a0,a1,a2} (a0 ignored), shared by all channels.
 * State (2 x + 2 y values per stage and channel) is kept in double on the device between calls. */
unsigned long llz_iir_cascade_mc_init(int channels, int stages, const double *coef);
void          llz_iir_cascade_mc_uninit(unsigned long handle);
/* planar [channels][frame_len] float32, device or host pointers; any frame_len >= 1. out may not overlap in (device
 * memory): a later time segment reads x where an earlier one writes y, so y overlapping x is refused with LLZ_ERR_ARG
 * (host x == y is staged through the handle's own buffers and works in place). Returns frame_len. */
int           llz_iir_cascade_mc(unsigned long handle, const float *x, float *y, int frame_len);
int           llz_iir_cascade_mc_set_stream(unsigned long handle, void *stream);
/* working precision of the pipelined kernel for this coefficient set: 64, or 32 when every section's rounding-noise gain
 * (sum of squares of the impulse response of 1/A(z), measured at init) is at most 16 -- poles of radius up to about 0.8 */
int           llz_iir_cascade_mc_precision(unsigned long handle);
/* what a call with this frame_len would run as, under the current llz_hip_tune settings: out = {form, precision, segs,
 * seg_chunks, warm} for the launch that takes the frame's whole chunks -- form one of LLZ_IIR_FORM_* (chunks of 1024, 1024,
 * 2048 samples), precision 32 or 64, segs time segments per channel of seg_chunks chunks (the last may be shorter), a later
 * one started warm chunks early from the zero state; chunks of the form's own size.  The rest of the frame (with WAVE32 an
 * odd 1024-sample chunk, then up to 1023 samples through the per-channel kernel) runs as one segment.  Computed by the
 * functions the call itself plans with; launches nothing and reads no device memory.  Assumes 16-byte aligned rows, as
 * every frame_len % 4 == 0 of an aligned buffer gives; a frame without a whole chunk reports segs = seg_chunks = warm = 0.
 * Returns 0 or LLZ_ERR_ARG. */
#define LLZ_IIR_FORM_PIPE   0   /* the stage pipeline */
#define LLZ_IIR_FORM_WAVE16 1   /* a wave per (channel, segment), 16 samples per lane */
#define LLZ_IIR_FORM_WAVE32 2   /* the same with 32 samples per lane */
int           llz_iir_cascade_mc_plan(unsigned long handle, int frame_len, int out[5]);

/* ---- Part 3: multi-channel GENERAL direct form I -- llz_iir_filter itself for many channels (llz_iir.c:103-156): any pole
 * order M and zero order N up to 8 (the reference's only in-tree caller uses order 3: libllzaudio/llz_musicpitch.c:1277-1285),
 * a[0..M] (a[0] ignored, taken as 1) and b[0..N] (NULL = zeros) HOST pointers shared by all channels.  float32 in and out,
 * double arithmetic in the reference's operation order; delay lines stay on the device between calls. ---- */
unsigned long llz_iir_mc_init(int channels, int M, const double *a, int N, const double *b);
void          llz_iir_mc_uninit(unsigned long handle);
/* planar [channels][frame_len] float32, device or host pointers, out of place; any frame_len >= 1. Returns frame_len.
 * Time segments: to fill the chip, the batch forms (this one and the cascade of part 2) may split a channel's frame into
 * segments that run in parallel.  The first continues from the handle's state; a later one starts early, from ZERO state,
 * and drops its warm-up outputs.  The host probes the filter at init (its response to a unit state, zero input) and takes
 * as warm-up the length after which that response stays below 1e-13 of its peak, so the state error of a segment is below
 * 1e-13 of peak before its first kept sample; segments are at least 8 warm-ups long, and a filter that has not decayed within
 * the probe is never split.  The output then equals the one-segment (reference-order) double sequence to about 1e-13
 * relative before the rounding to float32, not bit for bit, and may depend on frame_len.  llz_hip_tune("iir_segs", 1)
 * opts out: one segment per channel, bit for bit the reference's sequence rounded once.
 * out may not overlap in (device memory), and x == y is refused for host memory too: LLZ_ERR_ARG. */
int           llz_iir_mc(unsigned long handle, const float *x, float *y, int frame_len);
/* the number of time segments per channel a call with this frame_len would run with, under the current llz_hip_tune
 * settings (the launch's own computation; nothing is launched): segments of ceil(frame_len / segments) samples */
int           llz_iir_mc_segments(unsigned long handle, int frame_len);
int           llz_iir_mc_flush(unsigned long handle, float *y);         /* N more samples of x = 0 per channel: [channels][N]; returns N */
int           llz_iir_mc_set_stream(unsigned long handle, void *stream);

/* ---- Part 4: the biquad bank -- llz_iir_cascade_mc with a coefficient set per channel (an equaliser per channel, crossover
 * networks, per-microphone correction, different weightings in one batch) ----
 * Arguments: channels >= 1; stages 1..16, the same for every channel: a channel that needs fewer sections pads with identity
 *   sections {1,0,0,1,0,0}.  coef is a HOST pointer, [channels][stages][6] doubles {b0,b1,b2,a0,a1,a2}, a0 ignored (taken as
 *   1).  Every refusal returns (unsigned long)-1 (init) or LLZ_ERR_ARG with a message that names the function.
 * Buffers: the contract of llz_iir_cascade_mc: planar [channels][frame_len] float32, any frame_len >= 1; device memory is
 *   used in place and asynchronously on the handle's stream, host memory is staged and the call synchronous, host x == y
 *   works in place; device x and y that overlap are refused with LLZ_ERR_ARG.  The state, [channels][stages][x1,x2,y1,y2]
 *   in double, stays on the device between calls.
 * Precision is the handle's: 32 only if EVERY channel's set passes the criterion of llz_iir_cascade_mc_precision (and the
 *   iir_f64 tune is not 1); one channel that needs double puts the whole handle in double.
 * Warm-up (time segments, part 3) is the handle's: the maximum over the channels of the memory probe run on each channel's
 *   own cascade.  If one channel's probe says "not decayed within 64 chunks" the handle is never split along time, exactly as
 *   a shared handle with such a cascade.
 * Path and plan are chosen by the functions llz_iir_cascade_mc chooses with, under the same tunes (iir_segs, iir_pipe,
 *   iir_wave_min_items, iir_unpacked, iir_f64).  The 32-samples-per-lane forms fold the b0 gains into one input gain, which in
 *   a bank is a decision and a gain per channel: the bank does not take them, and llz_iir_bank_mc_plan reports
 *   LLZ_IIR_FORM_WAVE16 where llz_iir_cascade_mc_plan would report LLZ_IIR_FORM_WAVE32.  A bank in double precision has no
 *   wave form at all (its pipeline measured faster): its plan always reports LLZ_IIR_FORM_PIPE.  A bank whose rows are all equal
 *   holds the table values of llz_iir_cascade_mc and gives the same bits wherever the two plans are equal and the shared
 *   handle runs the same form: on the stage pipeline, and on the float32 16-sample wave form (the shared handle under
 *   iir_unpacked = 2) with the same iir_segs forced on both, since the two kinds of workgroup hold different numbers of
 *   waves and so choose different segment counts by themselves.
 * Host cost of init: each DISTINCT set is probed once (equal rows are common in banks), single-threaded, and the answer is
 *   the probe's own number, never an estimate of it: a plant's run is cut short only where the rest is known exactly (the
 *   sections in front of the plant are not stepped; the run ends when the state repeats).  Measured per distinct 8-section
 *   set: 4.2 ms for low-Q sections, 26 ms for 0.99-radius ones (the plain probe: 170 and 300 ms), so a bank of 4096 distinct
 *   high-Q sets takes 105 s to initialise and llz_iir_bank_mc_set_coef 4 .. 33 ms per distinct set given. */
unsigned long llz_iir_bank_mc_init(int channels, int stages, const double *coef);
void          llz_iir_bank_mc_uninit(unsigned long handle);
int           llz_iir_bank_mc(unsigned long handle, const float *x, float *y, int frame_len);   /* returns frame_len */
/* replace the sets of channels [first, first + count) between calls; coef: HOST [count][stages][6].  Ordered on the handle's
 * stream after the calls already issued (the caller waits for them).  The delay-line state is KEPT: the next call continues
 * every section's x1, x2, y1, y2 under the new coefficients, which is what a direct-form-I parameter change means.  The
 * handle's precision and warm-up are evaluated again over all channels (llz_iir_bank_mc_precision may answer differently
 * afterwards).  A range outside [0, channels) returns LLZ_ERR_ARG and changes nothing.  A call that fails later (out of
 * memory, a device error) puts the host's record of the given rows back, so precision and warm-up stay those of sets the
 * handle has run with; the device tables of the given rows may then hold either version: repeat the call or drop the handle. */
int           llz_iir_bank_mc_set_coef(unsigned long handle, int first, int count, const double *coef);
int           llz_iir_bank_mc_set_stream(unsigned long handle, void *stream);
int           llz_iir_bank_mc_precision(unsigned long handle);                       /* 32 or 64 */
int           llz_iir_bank_mc_plan(unsigned long handle, int frame_len, int out[5]); /* as llz_iir_cascade_mc_plan */

#ifdef __cplusplus
}
#endif
#endif
