/*
 * include/llz_adapt_matrix.h -- the multi-reference adaptive FIR filter, C ABI of libllzfilter_hip.so: llz_adapt_matrix_mc, a
 * partitioned-block frequency-domain NLMS filter with I shared references x_i, O desired signals d_o and a weight set per path
 * (o, i).  Where a microphone hears several loudspeakers at once -- stereo and surround echo cancellation, a cabin with several
 * noise references, online identification of the [O][I] room matrix a llz_fir_matrix_mc handle renders with -- a bank of
 * llz_adapt_mc filters cannot serve: each would take the other references' echo for noise and normalise by the wrong power.
 * Here the error of output o drives all of that output's I paths, normalised by the JOINT power of all references.  The
 * reference has no counterpart; the checker is a float64 model written from the definition below
 * (tests/adapt_matrix_checks.py).
 *
 * It is the matrix convolver of llz_fir.h part 6 -- a ring of input spectra per INPUT, the sum over inputs in groups -- with
 * the error, the normalised gradient and the constrained update of llz_adapt.h on those rings.
 *
 * The algorithm: block B, N = 2 B, P = ceil(flt_len / B) partitions, k blocks per call of the init's frame_len, R = P + k - 1
 * ring slots per input.  X_{i,q} is the N-point DFT (unnormalised, e^-j) of blocks (q - 1, q) of x_i.  W_{o,i,p} is the
 * spectrum of partition p of path (o, i); the weights start at zero.  For block j, in order:
 *   1. Every X_{i,j} enters ring i.
 *   2. Y_o = sum_i sum_{p < P} X_{i,j-p} W_{o,i,p}, in the order llz_fir_matrix_mc uses for a handle of the same (inputs,
 *      outputs, block): the inputs fall into its G groups; within a group the sum is one fma chain per bin from zero, i
 *      ascending and p ascending within i; the group partials are added g ascending.  y_o = the last B samples of IDFT_N(Y_o).
 *   3. e_o = d_o - y_o, one float32 subtraction per sample.  e is always stored, y when the caller passes a buffer for it.
 *   4. D = sum_i sum_{p < P} |X_{i,j-p}|^2, one value per bin, shared by all outputs: i ascending, p ascending within i; real
 *      and imaginary squares are summed apart by fma and added at the end; packed bin 0 (DC, Nyquist) is two real bins.
 *      There is no smoothed power state.
 *   5. For every output with mu_o != 0: E_o = DFT_N([0_B, e_o]), G_o = mu_o E_o / (D + delta).
 *   6. For every (o, i, p) with mu_o != 0: W_{o,i,p} += DFT_N(constrain(IDFT_N(conj(X_{i,j-p}) G_o))); the constraint zeroes
 *      every sample t >= min(B, flt_len - p B), with llz_adapt_mc's arithmetic and power-of-two scalings.
 * An output whose mu is 0 is FROZEN: steps 5 and 6 are skipped for it and its weights keep their bits.  With every output frozen
 * y has the bits of llz_fir_matrix_mc with those taps (all paths connected); with inputs = 1, e, y and the weights have the
 * bits of llz_adapt_mc with channels = outputs fed the one reference on every row.
 *
 * An output's values depend on all x and on its own d and mu alone.  The summation orders are fixed: the same calls give the
 * same bits, and how calls group the blocks of a stream changes no bit.  There is no connection table here: A NaN IN ANY x_i
 * REACHES EVERY ADAPTING OUTPUT through D (and every output's y through the product).
 *
 * Per call one forward and one power launch, then per block three launches (product, error, update) on the handle's stream,
 * the ring slot by value with each: a call CAPTURED INTO A GRAPH would replay one and the same slot -- graph capture is not
 * supported, as for llz_fir_stream_mc, llz_fir_matrix_mc and llz_adapt_mc.
 */
#ifndef LLZ_ADAPT_MATRIX_H
#define LLZ_ADAPT_MATRIX_H

#ifdef __cplusplus
extern "C" {
#endif

/* inputs, outputs 1..4096; block a power of two in 64..2048 (4096 is refused: the kernels would not fit their registers);
 * frame_len = k x block, k in 1..65535, the longest call; flt_len 1..131073; mu in [0, 2], the step size of every output (0 =
 * frozen); delta > 0 and finite, the regularisation of step 5 in units of |X|^2 (1e-3 x block x inputs suits references of unit
 * variance).  Device memory: outputs x inputs x P x block x 8 bytes of weights, inputs x R x block x 8 of rings, and scratch of
 * (G x outputs + outputs + k) x block x 8; when an allocation fails the message states the bytes asked for.  Every refusal
 * leaves a message of its own.  Returns the handle or (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_adapt_matrix_mc_init(int inputs, int outputs, int block, int frame_len, int flt_len, float mu, float delta);
void llz_adapt_matrix_mc_uninit(unsigned long h);
/* x (references): planar [inputs][n]; d (desired), e (error out), y (filter output, may be NULL): planar [outputs][n]; float32,
 * device memory (used in place, asynchronous on the handle's stream) or host memory (staged, synchronous); n a multiple of
 * block, at most the init's frame_len.  Device ranges of e or y that overlap x, d or each other are refused (LLZ_ERR_ARG).
 * Returns n, or a negative LLZ_ERR_* code. */
int  llz_adapt_matrix_mc(unsigned long h, const float *x, const float *d, float *e, float *y, int n);
/* the step sizes of outputs [out_first, out_first + out_count): mu = HOST [out_count], each in [0, 2], 0 = frozen; ordered on
 * the handle's stream behind the calls already issued */
int  llz_adapt_matrix_mc_set_step(unsigned long h, int out_first, int out_count, const float *mu);
/* the weights of the paths (out_first .. , in_first ..): taps = HOST [out_count][in_count][flt_len], laid out as
 * llz_fir_matrix_mc_set_taps takes it; the delay lines are kept; ordered on the stream */
int  llz_adapt_matrix_mc_set_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, const float *taps);
/* the weights of those paths as taps: HOST [out_count][in_count][flt_len].  The spectra are downloaded behind the calls already
 * issued and each partition is inverted on the host in double; its first min(block, flt_len - p block) samples are the taps,
 * rounded to float once -- what llz_fir_matrix_mc_init and _set_taps take. */
int  llz_adapt_matrix_mc_get_taps(unsigned long h, int out_first, int out_count, int in_first, int in_count, float *taps);
/* the delay lines (rings and last blocks) to zeros; clear_taps != 0: the weights to zero as well -- the state of a fresh handle
 * but for the step sizes --, else they are kept */
int  llz_adapt_matrix_mc_reset(unsigned long h, int clear_taps);
/* out = {N = 2 block, P = ceil(flt_len / block), ring slots R, blocks per call k of the init's frame_len, input groups G of the
 * product, inputs per group}; nothing is launched */
int  llz_adapt_matrix_mc_plan(unsigned long h, int out[6]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_adapt_matrix_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
