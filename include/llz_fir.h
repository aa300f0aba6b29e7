/*
 * include/llz_fir.h -- FIR design + streaming FIR, C ABI of libllzfilter_hip.so.
 *
 * Part 1 keeps the reference's single-channel `double` API symbol for symbol
 * (reference libllzfilter/llz_fir.h:26-95) so existing callers relink unchanged; the process functions run
 * on the GPU (HIP kernel, same accumulation order, no FMA contraction: results are bit-identical to the
 * reference CPU path for identical taps).
 * Part 2 is the multi-channel float32 batch extension of the same init / process / flush / uninit shape
 *  -- the path the MI355X kernels are built for.
 * Part 3 is the same batch with a tap set per channel: the filter bank (time domain, and overlap-save up to 257 taps).
 * Part 4 is the bank for long filters: the partitioned overlap-save of part 2 with a tap set per channel, 1..131073 taps.
 * Part 5 is the block convolver for short calls against long filters: it keeps the spectra of its input between calls.
 * Part 6 is that block convolver with a filter per (output, input) path: many inputs into many outputs, summed in the spectrum.
 */
#ifndef LLZ_FIR_H
#define LLZ_FIR_H

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef int win_t;                                   /* reference llz_fir.h:26 */
enum { HAMMING = 0, BLACKMAN, KAISER };              /* reference llz_fir.h:28-32 */

/* ---- Part 1: reference-identical symbols ------------------------------------------------------- */

/* replaces llz_fir.h:38-48 (llz_fir.c:442-530). Handle = pointer cast to unsigned long, as in the reference. */
unsigned long llz_fir_filter_lpf_init(int frame_len, int flt_len, double fc, win_t win_type);
unsigned long llz_fir_filter_hpf_init(int frame_len, int flt_len, double fc, win_t win_type);
unsigned long llz_fir_filter_bandpass_init(int frame_len, int flt_len, double fc1, double fc2, win_t win_type);
unsigned long llz_fir_filter_bandstop_init(int frame_len, int flt_len, double fc1, double fc2, win_t win_type);
void          llz_fir_filter_uninit(unsigned long handle);                       /* llz_fir.h:50 */

/* replaces llz_fir.h:56 (llz_fir.c:547-584). buf_in/buf_out are HOST pointers. Returns frame_len.
 * frame_len must equal the init frame_len: the reference's own history shift is only correct in that case
 * (llz_fir.c:562-566); a different length returns -1 where the reference asserts or
 * silently corrupts its history. */
int llz_fir_filter(unsigned long handle, double *buf_in, double *buf_out, int frame_len);
/* replaces llz_fir.h:58 (llz_fir.c:590-625): emits the flt_len-1 tail samples, returns flt_len-1 */
int llz_fir_filter_flush(unsigned long handle, double *buf_out);

/* windows and estimators, host side (llz_fir.h:64-79, llz_fir.c:61-193) */
int    llz_hamming(double *w, const int N);
int    llz_blackman(double *w, const int N);
int    llz_kaiser(double *w, const int N);
int    llz_kaiser_beta(double *w, const int N, const double beta);
double llz_kaiser_atten2beta(double atten);
int    llz_hamming_cof_num(double ftrans);
int    llz_blackman_cof_num(double ftrans);
int    llz_kaiser_cof_num(double ftrans, double atten);

/* tap design, host side (llz_fir.h:86-92, llz_fir.c:271-393). *h is malloc'ed; the CALLER frees it. */
int llz_fir_lpf_cof(double **h, int N, double fc, win_t win_type);
int llz_fir_hpf_cof(double **h, int N, double fc, win_t win_type);
int llz_fir_bandpass_cof(double **h, int N, double fc1, double fc2, win_t win_type);
int llz_fir_bandstop_cof(double **h, int N, double fc1, double fc2, win_t win_type);

/* llz_fir.h:94 (llz_fir.c:411-426): host dot product, x points at the newest sample */
double llz_conv(const double *x, const double *h, int h_len);

/* ---- Part 2: multi-channel float32 batch extension ---------------------------------------------- */

enum {
    LLZ_FIR_ALGO_AUTO = 0,       /* time domain up to 32 taps, overlap-save for 33..257 (1024-point), 258..513
                                  * (2048-point), 514..1025 (4096-point) and 1026..6145 (8192-point), matrix-core time
                                  * domain beyond (never LLZ_FIR_ALGO_PARTITIONED) */
    LLZ_FIR_ALGO_TIME = 1,       /* direct form, taps broadcast, input window staged in LDS */
    LLZ_FIR_ALGO_OVERLAP_SAVE = 2, /* 1024-point in-LDS FFT overlap-save, flt_len <= 257 */
    LLZ_FIR_ALGO_TIME_MFMA = 3,   /* direct form as a banded Toeplitz product on the fp32 matrix cores */
    LLZ_FIR_ALGO_OVERLAP_SAVE_2048 = 4, /* 2048-point register-transform overlap-save, 2 <= flt_len <= 1025 */
    LLZ_FIR_ALGO_OVERLAP_SAVE_4096 = 5, /* 4096-point register-transform overlap-save, 2 <= flt_len <= 3073 */
    LLZ_FIR_ALGO_OVERLAP_SAVE_8192 = 6, /* 8192-point register-transform overlap-save on pairs of waves, 2 <= flt_len <= 6145 */
    LLZ_FIR_ALGO_PARTITIONED = 7        /* uniformly partitioned overlap-save with the block spectra in device memory,
                                         * 1 <= flt_len <= 131073: the form for long filters, whose cost per sample grows with
                                         * flt_len / block instead of flt_len.  Never chosen by AUTO: name it.  (The other algos
                                         * end at 25248 taps, the time-domain kernel's LDS tile.) */
};

/* channels independent filters sharing one tap set. taps: HOST pointer, flt_len floats (double variant
 * below rounds to float once).  Returns (unsigned long)-1 on failure (llz_hip_last_error() says why). */
unsigned long llz_fir_filter_mc_init(int channels, int frame_len, const float *taps, int flt_len, int algo);
unsigned long llz_fir_filter_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len, int algo);
/* design + init in one call, mirroring llz_fir_filter_{lpf,hpf,bandpass,bandstop}_init */
unsigned long llz_fir_filter_mc_lpf_init(int channels, int frame_len, int flt_len, double fc, win_t win_type);
unsigned long llz_fir_filter_mc_hpf_init(int channels, int frame_len, int flt_len, double fc, win_t win_type);
unsigned long llz_fir_filter_mc_bandpass_init(int channels, int frame_len, int flt_len, double fc1, double fc2, win_t win_type);
unsigned long llz_fir_filter_mc_bandstop_init(int channels, int frame_len, int flt_len, double fc1, double fc2, win_t win_type);
void          llz_fir_filter_mc_uninit(unsigned long handle);

/* planar [channels][frame_len] float32 in and out (out may not alias in; out may not overlap in (device memory): refused
 * with LLZ_ERR_ARG). Pointers may be device memory
 * (used in place, asynchronous on the handle's stream) or host memory (staged through the GPU, synchronous).
 * frame_len must equal the init frame_len. Returns frame_len, or a negative LLZ_ERR_* code. */
int llz_fir_filter_mc(unsigned long handle, const float *in, float *out, int frame_len);
/* the same call on rows of larger buffers: channel c is in + c * in_pitch and out + c * out_pitch (pitches in floats, at least
 * frame_len).  Device memory only, used in place; the spans may not overlap.  Planes cut from a larger tensor keep the row
 * alignment they had, which the 1024-point overlap-save form uses: rows whose bases and pitches are multiples of 32 KB take its
 * aligned walk whatever frame_len is. */
int llz_fir_filter_mc_pitched(unsigned long handle, const float *in, float *out, int frame_len, long in_pitch, long out_pitch);
/* out: planar [channels][flt_len-1]; returns flt_len-1 */
int llz_fir_filter_mc_flush(unsigned long handle, float *out);
int llz_fir_filter_mc_flt_len(unsigned long handle);
int llz_fir_filter_mc_algo(unsigned long handle);
/* LLZ_FIR_ALGO_OVERLAP_SAVE: taps that are symmetric about a centre tap c = 32 K, K = 1..4 (65, 129, 193, 257 taps), are
 * filtered with the real spectrum of the centred taps.  Returns the K the handle's next call takes under the tunes set now, 0
 * for the complex spectrum product (every other tap set, every other algo, the ols_real_product = 0 tune). */
int llz_fir_filter_mc_real_rows(unsigned long handle);
/* LLZ_FIR_ALGO_PARTITIONED keeps the contract above.  Each call filters concat(history, frame) from scratch -- nothing spectral
 * is carried from call to call -- so a call costs about frame_len + flt_len samples of work: a frame much shorter than the
 * filter is legal but wasteful.  The flush runs through the same kernels.  The block spectra live in scratch allocated at init
 * from frame_len (at most 1 GiB; the channels go in passes of as many as fit; init fails when not one does).
 * out = {transform points N, partitions P = ceil(flt_len / (N / 2)), channels per pass, passes} for a call of n samples under
 * the tunes set now; nothing is launched.  LLZ_ERR_ARG for a handle of another algo. */
int llz_fir_filter_mc_partition_plan(unsigned long handle, int n, int out[4]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int llz_fir_filter_mc_set_stream(unsigned long handle, void *stream);

/* ---- Part 3: the filter bank -- the batch of part 2 with one tap set PER CHANNEL --------------------- */

/* channels independent filters, one tap set EACH (equaliser and crossover banks, per-microphone calibration, HRTF sets,
 * per-channel fractional delays).  taps: HOST pointer, planar [channels][flt_len] (the double variant rounds to float once).
 * channels 1..65535.  algo: LLZ_FIR_ALGO_TIME (any flt_len the time-domain kernel holds), LLZ_FIR_ALGO_OVERLAP_SAVE
 * (1024-point, 1..257 taps) or LLZ_FIR_ALGO_AUTO (time domain up to 32 taps, overlap-save for 33..257, time domain above);
 * the matrix-core form and the longer transforms are not built for a bank and are refused.  A bank of filters the time
 * domain does not hold (above 25248 taps), or cannot afford, is part 4's llz_fir_pbank_mc_init.
 * Returns (unsigned long)-1 on failure (llz_hip_last_error() says why). */
unsigned long llz_fir_bank_mc_init(int channels, int frame_len, const float *taps, int flt_len, int algo);
unsigned long llz_fir_bank_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len, int algo);
void          llz_fir_bank_mc_uninit(unsigned long handle);
/* the contract of llz_fir_filter_mc / llz_fir_filter_mc_flush: planar [channels][frame_len] float32, device memory (in
 * place, asynchronous on the handle's stream) or host memory (staged, synchronous), frame_len as at init, out may not
 * alias or overlap in (LLZ_ERR_ARG), flt_len-1 samples of history per channel carried from call to call; the flush
 * writes [channels][flt_len-1] */
int llz_fir_bank_mc(unsigned long handle, const float *in, float *out, int frame_len);
int llz_fir_bank_mc_flush(unsigned long handle, float *out);
/* replace the taps of channels [first, first+count) between calls; taps: HOST [count][flt_len], flt_len as at init.
 * Ordered on the handle's stream after the calls already issued; the history is kept: the next call filters
 * concat(history, frame) with the new taps.  A range outside [0, channels) is refused with LLZ_ERR_ARG. */
int llz_fir_bank_mc_set_taps(unsigned long handle, int first, int count, const float *taps);
int llz_fir_bank_mc_flt_len(unsigned long handle);
int llz_fir_bank_mc_algo(unsigned long handle);
int llz_fir_bank_mc_set_stream(unsigned long handle, void *stream);

/* ---- Part 4: the partitioned bank -- LLZ_FIR_ALGO_PARTITIONED with one tap set PER CHANNEL, 1..131073 taps ---------- */

/* channels (1..65535) independent filters of flt_len (1..131073) taps, one tap set each: room and cabinet responses, BRIR
 * sets, long per-microphone calibration.  taps: HOST pointer, planar [channels][flt_len] (the double variant rounds to float
 * once).  The handle IS A BANK HANDLE of part 3 with llz_fir_bank_mc_algo() == LLZ_FIR_ALGO_PARTITIONED: llz_fir_bank_mc,
 * _flush, _set_taps, _set_stream, _flt_len, _algo and _uninit take it with their contracts unchanged.  What part 2 says of
 * LLZ_FIR_ALGO_PARTITIONED holds: a call filters concat(history, frame) from scratch through the same three kernels, the flush
 * too; the transform size follows flt_len; the scratch is sized at init from frame_len (at most 1 GiB, channels in passes).  The
 * spectra of all tap sets stay in device memory: channels x ceil(flt_len / (N / 2)) x N x 8 bytes (2.1 MB per channel at
 * 131073 taps); when that allocation fails the message states the bytes asked for.  llz_fir_bank_mc_set_taps rebuilds the
 * spectra of the named channels.  Never reached through llz_fir_bank_mc_init, whose algo 7 stays refused.
 * Returns (unsigned long)-1 on failure (llz_hip_last_error() says why). */
unsigned long llz_fir_pbank_mc_init(int channels, int frame_len, const float *taps, int flt_len);
unsigned long llz_fir_pbank_mc_init_f64taps(int channels, int frame_len, const double *taps, int flt_len);
/* out = {N, P, channels per pass, passes} as llz_fir_filter_mc_partition_plan reports them; LLZ_ERR_ARG for every handle that
 * is not llz_fir_pbank_mc_init's (llz_fir_filter_mc_partition_plan in turn refuses every bank handle) */
int           llz_fir_pbank_mc_plan(unsigned long handle, int n, int out[4]);

/* ---- Part 5: the stream convolver -- short blocks against long filters, spectra kept between calls ------------------- */

/* Real-time convolution: frames of 64..4096 samples against up to 131073 taps (room and cabinet responses, BRIR sets).  A
 * uniformly partitioned overlap-save whose block is the CALLER'S: block (a power of two, 64..4096), frame_len = k x block with
 * k >= 1, P = ceil(flt_len / block) partitions.  The spectra of the last input blocks of every channel stay in device memory
 * between calls, in a ring of R = P + k - 1 half-spectra of `block` packed bins (a frequency-domain delay line), beside the
 * last `block` input samples: a call transforms only its k new blocks, sums the ring against the tap spectra and inverts --
 * one kernel launch, about P x block x 8 bytes of ring read per channel and block (1 MB at 131073 taps, at any block).
 * Which form when: this one for calls of ONE OR A FEW blocks, where LLZ_FIR_ALGO_PARTITIONED and llz_fir_pbank_mc_init redo
 * the whole history (about frame_len + flt_len samples of work per call) and cannot go below their 512..4096-sample block;
 * those two for LONG calls, whose blocks they run in parallel where this form walks a call's blocks in sequence, one
 * workgroup per channel.
 * channels 1..65535, flt_len 1..131073.  rows == 1: taps = HOST pointer to flt_len floats, one tap set for all channels;
 * rows == channels: planar [channels][flt_len], a tap set per channel (the double variant rounds to float once).  A bank of
 * equal rows gives the bits of the shared handle.  Device memory: rows x P x block x 8 bytes of tap spectra and channels x R x
 * block x 8 bytes of ring (about 1 MB per channel at 131073 taps); when an allocation fails the message states the bytes
 * asked for.  Every refusal leaves a message of its own.  Returns (unsigned long)-1 on failure (llz_hip_last_error() says why).
 * The result is llz_fir_filter_mc's on the concatenated stream (to rounding: the summation order differs). */
unsigned long llz_fir_stream_mc_init(int channels, int block, int frame_len, const float *taps, int rows, int flt_len);
unsigned long llz_fir_stream_mc_init_f64taps(int channels, int block, int frame_len, const double *taps, int rows, int flt_len);
void          llz_fir_stream_mc_uninit(unsigned long handle);
/* planar [channels][frame_len] float32 in and out, device memory (used in place, asynchronous on the handle's stream) or host
 * memory (staged, synchronous); frame_len as at init; out may not alias or overlap in (LLZ_ERR_ARG).  Returns frame_len, or a
 * negative LLZ_ERR_* code.  The ring's head is kept on the host and passed by value with each launch (no device-side
 * counter), so a call CAPTURED INTO A GRAPH would replay one and the same ring slot: graph capture is not supported.  How
 * calls group the blocks of a stream does not change a bit of the result. */
int llz_fir_stream_mc(unsigned long handle, const float *in, float *out, int frame_len);
/* out: planar [channels][flt_len-1], the response to ceil((flt_len-1) / block) zero blocks through the same kernel; returns
 * flt_len-1 and leaves the handle as llz_fir_stream_mc_reset does: reused, it gives the bits of a fresh handle.  With one tap
 * nothing is written, out may be NULL, and the call returns 0 after the same reset */
int llz_fir_stream_mc_flush(unsigned long handle, float *out);
/* the delay line (ring and last block) to zeros, ordered on the handle's stream; the taps stay */
int llz_fir_stream_mc_reset(unsigned long handle);
/* replace tap rows [first, first+count) between calls; taps: HOST [count][flt_len].  rows == channels: any range inside
 * [0, channels); rows == 1: only first 0, count 1.  Ordered on the handle's stream behind the calls already issued.  The
 * delay line is kept, and it holds INPUT spectra: from the next call on the output is the new taps applied to the whole
 * input so far -- a step in the output; llz_fir_xfade_stream_mc below fades instead.  While a fade is pending or in flight the
 * call is refused (LLZ_ERR_ARG, the message gives the blocks left). */
int llz_fir_stream_mc_set_taps(unsigned long handle, int first, int count, const float *taps);
/* out = {N = 2 block, P = ceil(flt_len / block), ring slots R, blocks per call k}; nothing is launched */
int llz_fir_stream_mc_plan(unsigned long handle, int out[4]);
int llz_fir_stream_mc_flt_len(unsigned long handle);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int llz_fir_stream_mc_set_stream(unsigned long handle, void *stream);
/* A click-free change of taps: rows [first, first+count) (taps: HOST [count][flt_len], ranges as _set_taps takes them) FADE to the
 * new taps over fade_blocks blocks, 1..4096.  The fade starts with the first block processed after the call.  With F =
 * fade_blocks, B = block and n = 0 .. F B - 1 counting samples from that block's first one, a fading row's output is
 *     y[n] = fmaf(w[n], y_new[n] - y_old[n], y_old[n]),    w[n] = (float)n / (float)(F B), correctly rounded
 * (F B <= 2^24, so n is exact in float32), where y_old is the output of the row's taps as they were, applied to the whole input
 * so far -- what llz_fir_stream_mc computes without the fade -- and y_new the same for the new taps: both filters run on the
 * one delay line, which holds input spectra.  From sample F B on the output is y_new alone and the handle is in exactly the
 * state _set_taps(new) would have left it in.  w[0] = 0: the first faded sample is the old filter's value to the bit; equal old
 * and new taps give y_new - y_old = 0: the whole fade is bit-equal to no fade; rows that do not fade keep their bits
 * throughout.  A fade spans calls: a call of k blocks may hold its start and its end, blocks past the end are plain new-taps
 * blocks, the weight depends on the sample's index within the fade alone, and how calls group the blocks does not change a bit.
 * ONE fade at a time per handle: a call while one is in flight is refused -- except that until the first block of a pending
 * fade has been processed, further calls with the same fade_blocks add or replace rows of that fade, so that a bank can fade
 * rows that are not neighbours together.  The new rows' spectra go into a second buffer of rows x P x block x 8 bytes,
 * allocated at the first fade and kept (a failed allocation names the bytes), built on the handle's stream behind the calls
 * already issued.  Refused, each with a message of its own: a bad handle, NULL taps, rows outside the handle, fade_blocks
 * outside 1..4096, a fade already in flight (a pending one with another fade_blocks gets a hint).  While a fade is pending or in
 * flight _set_taps is refused, _reset clears the delay line and adopts the new taps at once, and _flush goes on with the ramp
 * through its zero blocks (flush block j is fade block done + j) and then leaves the handle reset WITH THE NEW TAPS adopted.
 * Returns 0 or a negative LLZ_ERR_* code. */
int llz_fir_xfade_stream_mc(unsigned long handle, int first, int count, const float *taps, int fade_blocks);
/* the blocks of the fade still to run (fade_blocks while it is pending), 0 when none is pending or in flight; LLZ_ERR_ARG for a
 * bad handle */
int llz_fir_xfade_stream_mc_left(unsigned long handle);

/* ---- Part 6: the matrix convolver -- many inputs into many outputs, y_o = sum_i x_i * h_{o,i} -------------------------- */

/* N sources rendered to 2 ears (HRTF and BRIR sets), M microphones filtered and summed into B beams, crosstalk cancellers,
 * wave-field synthesis, multi-way crossovers: part 5's block convolver with a filter per PATH (o, i) and a sum over inputs.
 * block (a power of two, 64..4096), frame_len = k x block with k in 1..65535, P = ceil(flt_len / block), R = P + k - 1 as in
 * part 5.  There is one delay line per INPUT -- inputs x R x block x 8 bytes of ring beside the last `block` samples of every
 * input -- shared by all outputs; the sum over inputs and partitions happens in the spectrum, and one inverse transform runs
 * per output block: inputs + outputs transforms per block where a part-5 bank of inputs x outputs channels on replicated inputs
 * runs inputs x outputs forward and as many inverse ones, keeps as many rings, and leaves the sum to the caller.  A call is
 * three launches ordered by the handle's stream: the forward transforms, the product -- the sum over inputs cut into G groups
 * of neighbouring inputs, G fixed at init from (inputs, outputs, block) alone, each group's partial spectrum in a scratch --
 * and the inverse transforms, which add the partials g ascending.  Within a group the inputs go ascending, p ascending within
 * an input, one fma chain per bin: how calls group the blocks of a stream does not change a bit of the result, a fresh handle
 * repeats its bits, and with all inputs but one at zero an output is part 5's for that path, value for value.
 * A path whose flt_len taps are ALL ZERO is not connected: the product skips it -- it costs no memory traffic and passes
 * nothing on, not even a NaN or an Inf of its input -- so a routing matrix that is mostly zeros costs what its connected paths
 * cost.  (Its spectra stay allocated.)
 * Which form when: this one wherever an output sums several inputs or several outputs share an input: by count it reads half
 * the bytes of the part-5 emulation and runs inputs + outputs transforms for its inputs x outputs (the timing
 * table against that emulation is not measured yet, so no shape is known at which the emulation wins).  For inputs == outputs
 * with a diagonal matrix part 5's bank is the direct form: one launch per call and no scratch.
 * inputs, outputs 1..4096, flt_len 1..131073.  taps: HOST pointer, [outputs][inputs][flt_len] (the double variant rounds to
 * float once).  Device memory: outputs x inputs x P x block x 8 bytes of tap spectra, the rings, and G x outputs x max(k, blocks
 * of a flush pass) x block x 8 bytes of partial spectra (a flush's passes are cut so that these stay within 64 MiB); when an
 * allocation fails the message states the bytes asked for.  Every refusal leaves a message of its own.  Returns
 * (unsigned long)-1 on failure (llz_hip_last_error() says why). */
unsigned long llz_fir_matrix_mc_init(int inputs, int outputs, int block, int frame_len, const float *taps, int flt_len);
unsigned long llz_fir_matrix_mc_init_f64taps(int inputs, int outputs, int block, int frame_len, const double *taps, int flt_len);
void          llz_fir_matrix_mc_uninit(unsigned long handle);
/* in: planar [inputs][frame_len], out: planar [outputs][frame_len], float32, device memory (used in place, asynchronous on the
 * handle's stream) or host memory (staged, synchronous); frame_len as at init; out may not alias or overlap in (LLZ_ERR_ARG).
 * Returns frame_len, or a negative LLZ_ERR_* code.  The rings' head is kept on the host and passed by value with each launch,
 * and the two buffers of the last input block are swapped there, so a call CAPTURED INTO A GRAPH would replay one and the same
 * ring slot: graph capture is not supported. */
int llz_fir_matrix_mc(unsigned long handle, const float *in, float *out, int frame_len);
/* out: planar [outputs][flt_len-1], the response to ceil((flt_len-1) / block) zero blocks, run side by side; returns flt_len-1
 * and leaves the handle as llz_fir_matrix_mc_reset does: reused, it gives the bits of a fresh handle.  With one tap nothing is
 * written, out may be NULL, and the call returns 0 after the same reset */
int llz_fir_matrix_mc_flush(unsigned long handle, float *out);
/* the delay lines (rings and last blocks) to zeros, ordered on the handle's stream; the taps stay */
int llz_fir_matrix_mc_reset(unsigned long handle);
/* replace the sub-matrix of paths [out_first, out_first+out_count) x [in_first, in_first+in_count) between calls; taps: HOST
 * [out_count][in_count][flt_len].  A range outside the matrix is refused.  Ordered on the handle's stream behind the calls
 * already issued, the connection table too: a path is connected from then on exactly when its new taps are not all zero.  The
 * delay lines are kept, and they hold INPUT spectra: from the next call on the output is the new taps applied to the whole
 * input so far (no crossfade: llz_fir_xfade_matrix_mc below fades instead, and while its fade is pending or in flight this
 * call is refused with LLZ_ERR_ARG, the message giving the blocks left). */
int llz_fir_matrix_mc_set_taps(unsigned long handle, int out_first, int out_count, int in_first, int in_count, const float *taps);
/* out = {N = 2 block, P = ceil(flt_len / block), ring slots R, blocks per call k, input groups G, connected paths}; nothing is
 * launched */
int llz_fir_matrix_mc_plan(unsigned long handle, int out[6]);
int llz_fir_matrix_mc_flt_len(unsigned long handle);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int llz_fir_matrix_mc_set_stream(unsigned long handle, void *stream);
/* A click-free change of paths: the sub-matrix [out_first, out_first+out_count) x [in_first, in_first+in_count) (taps: HOST
 * [out_count][in_count][flt_len], ranges as _set_taps takes them) FADES to the new taps over fade_blocks blocks, 1..4096: part 5's
 * fade carried to outputs that sum inputs.  An output FADES when at least one of its paths is in the fade.  The fade starts with
 * the first block processed after the call.  With F = fade_blocks, B = block and n = 0 .. F B - 1 counting samples from that
 * block's first one, a fading output o is
 *     y_o[n] = fmaf(w[n], y_new_o[n] - y_old_o[n], y_old_o[n]),    w[n] = (float)n / (float)(F B), correctly rounded
 * (F B <= 2^24, so n is exact in float32), where y_old_o is exactly what llz_fir_matrix_mc computes with the row's taps as they
 * were -- the same G groups, the same chain order -- and y_new_o the same with the faded paths replaced; both run on the one
 * set of delay lines, which hold input spectra (one walk of the rings serves both sums).  The blend is per OUTPUT, after the sum
 * over inputs, not per path.  From sample F B on the output is y_new alone and the handle is in exactly the state
 * _set_taps(new) would have left it in: the spectra, the connection table and _plan's out[5].  For finite data: w[0] = 0, so the
 * first faded sample has the old filter's bits; a fade to equal taps is bit-equal to no fade; an output with no path in the fade
 * keeps its bits throughout; and the weight depends on the sample's index within the fade alone, so a fade spans calls (a call
 * of k blocks may hold its start and its end, blocks past the end are plain new-taps blocks) and how calls group the blocks
 * changes no bit.
 * The connection follows the tap set: the old sum skips the paths whose old taps are all zero, the new sum those whose new taps
 * are.  A path fading FROM all-zero taps is a source fading in; a path fading TO all-zero taps is a source fading out, and it is
 * unconnected and free of traffic once the fade is over.  While the fade runs a NaN or an Inf of x_i reaches y_o if (o, i) is
 * connected under EITHER tap set.  _plan's out[5], while a fade is pending or in flight, counts the paths connected under the
 * old or the new taps -- what a fading block reads -- and the new taps' count afterwards.
 * ONE fade at a time per handle: a call while one is in flight is refused -- except that until the first block of a pending
 * fade has been processed, further calls with the same fade_blocks add or replace paths of that fade (a later call to the same
 * path replaces the earlier one), so that a renderer can fade columns that are not neighbours together.  The new paths' spectra
 * go into a second buffer of the tap spectra's size and the new sums' partial spectra into a second scratch, both allocated at
 * the first fade and kept (a failed allocation names the bytes); the spectra are built as _set_taps builds them, on the handle's
 * stream behind the calls already issued.  A handle that never fades allocates nothing of this and launches its three kernels
 * untouched.  Refused, each with a message of its own, none of them starting or altering a fade: a bad handle, NULL taps, an
 * output range outside the handle, an input range outside it, fade_blocks outside 1..4096, a fade already in flight (a pending
 * one with another fade_blocks gets a hint).  While a fade is pending or in flight _set_taps is refused (LLZ_ERR_ARG, the message
 * gives the blocks left), _reset clears the delay lines and adopts the new taps at once, _flush goes on with the ramp through
 * its zero blocks (flush block j is fade block done + j, across the flush's scratch passes too) and then leaves the handle reset
 * WITH THE NEW TAPS adopted, and _uninit is clean.  Returns 0 or a negative LLZ_ERR_* code. */
int llz_fir_xfade_matrix_mc(unsigned long handle, int out_first, int out_count, int in_first, int in_count, const float *taps,
                            int fade_blocks);
/* the blocks of the fade still to run (fade_blocks while it is pending), 0 when none is pending or in flight; LLZ_ERR_ARG for a
 * bad handle */
int llz_fir_xfade_matrix_mc_left(unsigned long handle);

#ifdef __cplusplus
}
#endif
#endif
