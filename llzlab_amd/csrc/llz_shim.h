/*
 * llz_shim.h -- INTERNAL boundary between the host C layer (csrc/host, .c files, gcc) and the HIP translation
 * units (csrc/kernels, .hip files, hipcc).  "Host code stays C and calls HIP through a thin C-ABI shim": the host
 * layer never includes a HIP header; everything it needs from the device is one of these functions.
 * All pointers named dev_* / in / out / hist are DEVICE pointers unless stated; stream is a hipStream_t as void*.
 * Every function returns 0 on success or a negative LLZ_ERR_* code and records text for llz_hip_last_error().
 */
#ifndef LLZ_SHIM_H
#define LLZ_SHIM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ---- */
void  llzs_set_error(const char *fmt, ...);
void *llzs_malloc(size_t bytes);
void  llzs_free(void *p);
int   llzs_h2d(void *dev_dst, const void *host_src, size_t bytes, void *stream);   /* synchronous for the caller */
int   llzs_d2h(void *host_dst, const void *dev_src, size_t bytes, void *stream);   /* synchronous for the caller */
int   llzs_d2d(void *dev_dst, const void *dev_src, size_t bytes, void *stream);    /* asynchronous on stream */
int   llzs_memset(void *dev_dst, int value, size_t bytes, void *stream);
int   llzs_fill_f32(float *dst, float value, size_t count, void *stream);          /* dst[i] = value, i < count, on stream */
int   llzs_sync(void *stream);
int   llzs_is_device_ptr(const void *p);

/* ---- tuning overrides (measurement and tests only) ----
 * The library never reads the environment.  Every algorithm / launch-shape choice is made from the problem's shape; a
 * choice can be overridden for A/B measurements and for tests that force a rarely taken form through the public
 * llz_hip_tune(name, value) (include/llz_hip.h).  value < 0 = unset (the library's own choice). */
enum {
    LLZS_TUNE_OLS_WG_PER_CU = 0,        /* resident workgroups per CU the overlap-save grid is sized for */
    LLZS_TUNE_RS_GENERIC,           /* 1: general L/M resampler without the register-window kernel; 2: first LDS kernel */
    LLZS_TUNE_RS_TILES,             /* tiles per workgroup of the general L/M resampler */
    LLZS_TUNE_RS_DEC_VALU,          /* 1: L = 1 float32 decimator on the vector pipe (LDS polyphase kernel) */
    LLZS_TUNE_RS_I16_PATH,          /* 1: no screened pass: LLZ_PCM_I16 on the all-double kernel, LLZ_PCM_I16_FAST on the float32-sum one */
    LLZS_TUNE_MFMA_NACC,            /* accumulator tiles per wave of the matrix-core FIR (1 / 2) */
    LLZS_TUNE_MFMA_WG_PER_CU,
    LLZS_TUNE_FFT_GENERIC,          /* 1: staged LDS passes instead of the register transforms */
    LLZS_TUNE_IIR_SEGS,             /* time segments per channel */
    LLZS_TUNE_IIR_UNPACKED,         /* 2: the fetch-ahead kernels with 16 samples per lane only (no 32-sample forms); (1 selected
                                     * the first wave-autonomous kernels, retired in round 3: profiles/r02/time_iir.txt keeps
                                     * their numbers) */
    LLZS_TUNE_IIR_F64,              /* 1: double arithmetic whatever the noise-gain check says */
    LLZS_TUNE_IIR_PIPE,             /* 1: stage pipeline even where the wave form would be taken */
    LLZS_TUNE_IIR_WAVE_MIN_ITEMS,   /* crossover (channel, segment) item count of the wave form */
    LLZS_TUNE_SHARD_RCCL,           /* 1: sharded handles broadcast their tables through RCCL even on a single device */
    LLZS_TUNE_RS_MFMA_FORM,         /* 1: matrix-core L/M resampler with a wave per PERIOD tile (first form) */
    LLZS_TUNE_OLS_SEG_LEN,          /* jobs per segment of the 1024-point overlap-save walk (1..16) */
    LLZS_TUNE_MDCT_RUN,             /* MDCT-frames synthesis: output segments per group (0: a launch for the even and one for
                                     * the odd frames) */
    LLZS_TUNE_MDCTQ_STEPS,          /* 1: fixed-point MDCT (both FFT forms) as three launches (step, transform, step) */
    LLZS_TUNE_RS_I16_TILES,         /* bit-exact int16 L/M resampler: period tiles per span (1..4) */
    LLZS_TUNE_RS_I16_WALK,          /* ... consecutive spans per workgroup */
    LLZS_TUNE_ACF_LDS,              /* 1: direct autocorrelation always on the LDS-window kernel (no register form for p <= 32) */
    LLZS_TUNE_STFT_FULL,            /* 1: STFT synthesis frames of 512 / 2048 points on the full-size complex inverse transform */
    LLZS_TUNE_LPC_SPLIT,            /* 1: batch LPC with p <= 32 as two launches (correlation, then recursion) like p > 32 */
    LLZS_TUNE_BANK_GLOBAL_H,        /* 1: filter-bank overlap-save reads each spectrum bin from global memory per job (the form
                                     * measured against and dropped: fir_bank.hip) instead of a half-wave's own LDS image */
    LLZS_TUNE_PART_NFFT,            /* partitioned overlap-save: transform points (1024, 2048, 4096, 8192), read at init */
    LLZS_TUNE_PART_SCRATCH_MB,      /* ... cap of the spectra scratch in MiB (1 .. 1024; the library's own: 1024), read at init and per call */
    LLZS_TUNE_OLS_SUPERBLOCK,       /* 1024-point overlap-save on large batches with 32 KB-aligned rows: 1 = the super-block walk
                                     * on small batches too (never without the alignment), 0 = the segment walk */
    LLZS_TUNE_CSD_SCRATCH_KB,       /* llz_csd_mc: cap of the run-partial scratch in KiB (the library's own: 256 MiB), read per call */
    LLZS_TUNE_OLS_REAL_PRODUCT,     /* 1024-point overlap-save, tap sets that are symmetric about a centre tap at 32, 64, 96 or 128:
                                     * 0 = the complex spectrum product all the same (unset: the real product of the centred
                                     * taps), read at init and per call */
    LLZS_TUNE_ADAPT_PPW,            /* llz_adapt_mc, llz_adapt_matrix_mc: partitions per workgroup of the weight update (1..64), read per call; no bit
                                     * of the result depends on it */
    LLZS_TUNE_ASRC_TABLE_GLOBAL,    /* llz_asrc_mc: 1 = the table is read from global memory even where it fits the LDS form, read at init */
    LLZS_TUNE_PFB_GLOBAL,           /* llz_pfb_mc: 1 = the analysis fold reads its samples through the caches even where a run's span fits LDS,
                                     * read per call; no bit of the result depends on it */
    LLZS_TUNE_COUNT
};
int llzs_tune(int id);                                   /* current override or -1 */

/* ---- devices, streams, events (sharded handles: llz_shard_host.c) ---- */
int   llzs_device_get(void);                       /* current device, negative on error */
int   llzs_device_set(int device);
int   llzs_device_enter(int device);               /* make `device` current; returns the previous one (or -1) */
void  llzs_device_leave(int previous);
void *llzs_stream_create(void);                    /* non-blocking stream on the current device, NULL on failure */
void  llzs_stream_destroy(void *stream);
void *llzs_event_create(void);
void  llzs_event_destroy(void *event);
int   llzs_event_record(void *event, void *stream);
double llzs_event_elapsed_ms(void *start, void *stop);   /* synchronises on stop; negative on error */

/* Coefficient-table uploads go through llzs_h2d_table so that a sharded init can see them: mode 1 uploads and records
 * (destination, size) of every table of the handle being built on this thread, mode 2 records WITHOUT uploading (the
 * tables of the other shards are filled by llzs_tables_broadcast from shard 0's), mode 0 = plain upload. */
typedef struct {
    void *dev;
    size_t bytes;
} llzs_table_ref;
#define LLZS_MAX_TABLES 16
void llzs_table_capture(int mode);
int  llzs_table_captured(llzs_table_ref *dst, int capacity);     /* number recorded since the last llzs_table_capture */
int  llzs_h2d_table(void *dev_dst, const void *host_src, size_t bytes);
/* tables[s][t]: table t of shard s (same count and sizes in every shard), shard 0 holds the data.  Shards on shard 0's
 * device get device-to-device copies; every other device receives ONE ncclBroadcast per table over a communicator of
 * the distinct devices (ncclCommInitAll, librccl loaded on first use) and hands copies to its further shards. */
int  llzs_tables_broadcast(llzs_table_ref *const *tables, int ntables, int nshards, const int *device,
                           void *const *stream);
int  llzs_tables_broadcast_ranks(void);     /* ranks of the RCCL communicator the last broadcast of this thread used (0: none) */

/* ---- FIR ---- */
#define LLZS_FIR_TAP_PAD 8      /* time-domain kernels read taps in groups of 8: pad the table with zeros */

/* y[c][i] = sum_k taps[k] * x[c][i-k]; x[c][i<0] = hist[c][flt_len-1+i] (hist NULL = zeros).
 * in/out planar with row pitch in_pitch/out_pitch elements. taps: flt_len floats padded to a multiple of 8. */
int llzs_fir_td_f32(const float *in, float *out, const float *hist, const float *taps_padded,
                    int channels, int n, long in_pitch, long out_pitch, int flt_len, void *stream);
int llzs_fir_td_f32_fits(int flt_len);      /* 1 when the taps fit the time-domain kernel's LDS tile */
/* the filter bank: the same with a tap row per channel, taps_bank = [channels][tpad], tpad = flt_len rounded up to 16 */
int llzs_fir_td_bank_f32(const float *in, float *out, const float *hist, const float *taps_bank, int channels, int n,
                         long in_pitch, long out_pitch, int flt_len, void *stream);
/* overlap-save with nfft = 1024, 2048, 4096 or 8192 points (fir_ols.hip): 1..257, 2..1025, 2..3073 or 2..6145 taps.  The
 * tables, all complex floats: hfreq = DFT_nfft(taps) / nfft as P = nfft / 1024 planes of 1024 (bin k in plane k mod P, row
 * k / P; P = 1 is natural order), twid = [32][32] W_1024^(ab), tw2k = [1024] W_2048^n (2048 and 4096 points, else NULL),
 * tw4k = [2048] W_4096^n (4096 and 8192 points, else NULL). */
typedef struct {
    float *hfreq, *twid, *tw2k, *tw4k;
    /* 1024 points only, else NULL / 0.  Taps that are bit for bit symmetric about tap c = 32 K, K = 1..4 (flt_len = 2 c + 1),
     * have a REAL spectrum once they are centred at index 0: hreal = [1024] floats Re DFT_1024(g) / 1024, g[n] = taps[n + c]
     * circularly, natural bin order, and real_rows = K: the product with it yields every output c samples = K rows of 32 early */
    float *hreal;
    int real_rows;
} llzs_ols_tables;
int llzs_fir_ols_f32(int nfft, const llzs_ols_tables *t, const float *in, float *out, const float *hist, int channels,
                     int n, long in_pitch, long out_pitch, int flt_len, void *stream);
/* 1 when the 1024-point call of this shape takes the super-block walk (k_fir_ols_chain_f32), 0 for the segment walk: the
 * launcher's own decision under the tunes set now, for tests and measurement tools; nothing is launched */
int llzs_fir_ols_superblock(const float *in, const float *out, int channels, int n, long in_pitch, long out_pitch, int flt_len);
/* the K of the spectrum product a 1024-point call with these tables takes under the tunes set now: t->real_rows, or 0 (the
 * complex product) without a real table or under ols_real_product = 0; nothing is launched */
int llzs_fir_ols_real_rows(const llzs_ols_tables *t);
/* 1024-point overlap-save with a spectrum per channel (fir_bank.hip), 1..257 taps: hbank = [channels][LLZS_BANK_PITCH] complex
 * floats, row c = bins 0..512 of DFT_1024(taps of channel c) / 1024 (the taps are real: the kernel mirrors the rest), the
 * row's tail unused; twid as above */
#define LLZS_BANK_BINS 513
#define LLZS_BANK_PITCH 520
int llzs_fir_bank_ols_f32(const float *hbank, const float *twid, const float *in, float *out, const float *hist, int channels,
                          int n, long in_pitch, long out_pitch, int flt_len, void *stream);
/* time domain on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), with optional decimation:
 * y[c][i] = gain * sum_{k<T} taps[k] * x[c][i*M - k], x[c][<0] = hist[c][T-1+idx] (hist NULL = zeros); n_out outputs
 * per channel from n_in inputs, (n_out-1)*M < n_in.  taps: T floats (no padding needed). */
int llzs_fir_mfma_f32(const float *in, float *out, const float *hist, const float *taps, int channels,
                      long n_in, long n_out, long in_pitch, long out_pitch, int T, int M, float gain, void *stream);
int llzs_fir_mfma_f32_fits(int T, int M);           /* 1 when the LDS image of one tile fits */
/* the same with int16 samples in and out (fp32 accumulate, clamp, truncate toward zero): within 1 LSB of the reference's
 * double accumulation, not bit-exact; taps as floats, gain folded into them */
int llzs_fir_mfma_i16(const short *in, short *out, const short *hist, const float *taps, int channels,
                      long n_in, long n_out, long in_pitch, long out_pitch, int T, int M, float gain, void *stream);
int llzs_fir_mfma_i16_fits(int T, int M);
/* int16 in and out, BIT-EXACT with the reference's double loop (llz_resample.c:583-603, L = 1), screened on the matrix
 * cores (fir_mfma_i8.hip): digits = [5][T] balanced base-256 digits of G[k] = round(g[k] 2^shift), bias = 128 sum G[k],
 * gd = the T double taps, eps = the host's bound on |screen value - reference value| (< 0.25) */
int llzs_fir_mfma_i16x(const short *in, short *out, const short *hist, const signed char *digits, const double *gd,
                       int channels, long n_in, long n_out, long in_pitch, long out_pitch, int T, int M, int shift,
                       long long bias, double gain, double eps, void *stream);
int llzs_fir_mfma_i16x_fits(int T, int M);
#define LLZS_MX_PLANES 5
/* uniformly partitioned overlap-save (fir_part.hip), 1..LLZS_FIR_PART_MAX_TAPS taps, nfft = 1024, 2048, 4096 or 8192, block
 * B = nfft / 2, P = ceil(flt_len / B) partitions.  hpart = [P][nfft] complex floats, row p = DFT_nfft(taps[p B .. p B + B),
 * zero-padded) / nfft in the ORDER OF A DECIMATION-IN-FREQUENCY TRANSFORM'S OUTPUT (entry i = bin bitrev(i)); tw = [nfft / 2]
 * complex W_nfft^m.  scratch: device memory of scratch_bytes for the block spectra; the channels go in passes of as many as
 * it holds (llzs_fir_part_need bytes each), LLZ_ERR_NOMEM when not one does.  llzs_fir_part_plan launches nothing:
 * plan = {nfft, P, channels per pass, passes}. */
#define LLZS_FIR_PART_MAX_TAPS 131073
int llzs_fir_part_need(int nfft, int flt_len, int n, size_t *bytes);      /* scratch bytes of one channel */
int llzs_fir_part_plan(int nfft, int flt_len, int n, int channels, size_t scratch_bytes, int plan[4]);
int llzs_fir_part_f32(int nfft, const float *hpart, const float *tw, float *scratch, size_t scratch_bytes, const float *in,
                      float *out, const float *hist, int channels, int n, long in_pitch, long out_pitch, int flt_len,
                      void *stream);
/* the same with a tap set per channel: hbank = [channels][P][nfft] complex floats, channel c's rows as hpart's */
int llzs_fir_part_bank_f32(int nfft, const float *hbank, const float *tw, float *scratch, size_t scratch_bytes, const float *in,
                           float *out, const float *hist, int channels, int n, long in_pitch, long out_pitch, int flt_len,
                           void *stream);
/* the block convolver with a frequency-domain delay line (fir_stream.hip), block = 64 .. 4096 (a power of two), N = 2 block,
 * P = ceil(flt_len / block) partitions.  hspec = [P][block] complex floats (bank != 0: [channels][P][block]) as
 * llz_host_stream_spectra builds them: the packed half-spectra of the partitions over 2 N, in the order of a decimation-in-
 * frequency transform's output; tw = [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i); ring =
 * [channels][R][block] complex, the spectra of the last input blocks, R >= P; prev = [channels][block], the last input block.
 * flush == 0: the nblk blocks of in ([channels][in_pitch], in_pitch >= nblk block) in order, block j's spectrum into ring slot
 * (head + j) mod R, prev updated; the caller advances head by nblk.  flush != 0: nblk <= P zero blocks behind the input so far;
 * in is not read, ring and prev are not written.  Either way the first n_out <= nblk block samples of every channel are stored
 * to out ([channels][out_pitch]). */
int llzs_fir_stream_f32(int block, const float *hspec, int bank, const float *tw, float *ring, float *prev, const float *in,
                        float *out, int channels, int nblk, int flush, long n_out, long in_pitch, long out_pitch, int P, int R,
                        int head, void *stream);
/* llzs_fir_stream_f32 with a fade between tap sets in flight (fir_stream_fade.hip): the same launch arguments, then hspec_new =
 * the new taps' spectra laid out as hspec (only rows marked fading are read), fading = one byte per tap row on the device
 * (bank != 0: channels rows, else one), and the fade's position: block j of this launch is block fade_done + j of fade_blocks
 * (1 .. 4096, 0 <= fade_done < fade_blocks).  A fading row's samples are fmaf(w, y_new - y_old, y_old), w = (float)n / (float)
 * (fade_blocks block), n counted from the fade's first sample; from block fade_blocks on they are y_new alone; rows not marked
 * get llzs_fir_stream_f32's bits. */
int llzs_fir_stream_fade_f32(int block, const float *hspec, int bank, const float *tw, float *ring, float *prev, const float *in,
                             float *out, int channels, int nblk, int flush, long n_out, long in_pitch, long out_pitch, int P,
                             int R, int head, const float *hspec_new, const unsigned char *fading, int fade_done,
                             int fade_blocks, void *stream);
/* the many-in, many-out stream convolver (fir_matrix.hip): llzs_fir_stream_f32's block, tw and packed spectra, with a delay line
 * per INPUT and a sum over inputs, as three launches ordered by the stream.  ring = [inputs][R][block] complex; prev_in /
 * prev_out = [inputs][block], two different buffers (the caller swaps them after a call); hspec = [outputs][inputs][P][block]
 * complex, a row as llz_host_stream_spectra builds it; conn = [outputs][inputs] bytes, 0 = the path (o, i) is skipped; ypart =
 * [groups][outputs][nblk][block] complex scratch, group g the inputs [g group_size, (g + 1) group_size) (the last group may be
 * short).  inputs, outputs 1..4096, nblk 1..65535.
 * fwd: the spectra of the nblk blocks of in ([inputs][in_pitch]) into ring slots (head + j) mod R, block nblk - 1 into prev_out;
 *      flush != 0: nblk == 1, the spectrum of (prev_in, zeros) into slot head, in and prev_out untouched.
 * mac: ypart[g][o][j] = the sum over group g's connected inputs (ascending) and p (ascending) of ring_i[(head + j - p) mod R]
 *      H[o][i][p]; flush != 0: the launch's block j is block j0 + j of the flush and starts at p = j0 + j, j0 + nblk <= P
 *      (a long flush goes in passes of as many blocks as ypart holds); flush == 0: j0 == 0.
 * inv: the partials added g ascending, the inverse transform, the first n_out <= nblk block samples of every output stored to
 *      out ([outputs][out_pitch]). */
int llzs_fir_matrix_fwd_f32(int block, const float *tw, float *ring, const float *prev_in, float *prev_out, const float *in,
                            int inputs, int nblk, int flush, long in_pitch, int R, int head, void *stream);
int llzs_fir_matrix_mac_f32(int block, const float *hspec, const float *ring, const unsigned char *conn, float *ypart, int inputs,
                            int outputs, int nblk, int flush, int j0, int P, int R, int head, int groups, int group_size,
                            void *stream);
int llzs_fir_matrix_inv_f32(int block, const float *ypart, const float *tw, float *out, int outputs, int nblk, int groups,
                            long n_out, long out_pitch, void *stream);
/* the product and the inverse of the matrix convolver with a fade between tap sets pending or in flight (fir_matrix_fade.hip;
 * the forward launch does not change: the rings hold input spectra).  The plain launches' arguments, and: hspec_new / conn_new =
 * the new taps' spectra and connection table laid out as hspec / conn, read only where fade[o][i] != 0; fade = [outputs][inputs]
 * bytes, the paths in the fade; ofade = [outputs] bytes, the outputs with at least one such path; ypart_new = a second scratch
 * of ypart's size; the fade's position: block j of the launch is block fade_done + j0 + j of fade_blocks (1 .. 4096, 0 <=
 * fade_done < fade_blocks; the inverse takes j0 for it, the same value as its product).  An output marked in ofade: inside the
 * fade ypart holds the old taps' partial sums, ypart_new the new taps' (one walk of the rings for both) and its samples are
 * fmaf(w, y_new - y_old, y_old), w = (float)n / (float)(fade_blocks block), n counted from the fade's first sample; from block
 * fade_blocks on it is the new taps' output alone.  Outputs not marked get the plain launches' bits. */
int llzs_fir_matrix_mac_fade_f32(int block, const float *hspec, const float *hspec_new, const float *ring,
                                 const unsigned char *conn, const unsigned char *conn_new, const unsigned char *fade,
                                 const unsigned char *ofade, float *ypart, float *ypart_new, int inputs, int outputs, int nblk,
                                 int flush, int j0, int P, int R, int head, int groups, int group_size, int fade_done,
                                 int fade_blocks, void *stream);
int llzs_fir_matrix_inv_fade_f32(int block, const float *ypart, const float *ypart_new, const unsigned char *ofade,
                                 const float *tw, float *out, int outputs, int nblk, int j0, int groups, long n_out,
                                 long out_pitch, int fade_done, int fade_blocks, void *stream);
/* the partitioned frequency-domain NLMS adaptive filter (fir_adapt.hip, the error tail and the update kernel from
 * adapt_steps.hpp; include/llz_adapt.h), block = 64 .. 2048: two launches per block, ordered by the stream.  w = [channels][P][block] complex, the weights' packed spectra laid out and scaled as
 * llz_host_stream_spectra builds them; tw, ring ([channels][R][block] complex), prev as llzs_fir_stream_f32's; g = [channels]
 * [block] complex scratch; mu = [channels] step sizes on the device, 0 = the channel is frozen; x, d, e, y = [channels][pitch],
 * y may be NULL.
 * filter: block j of the call's nblk: its spectrum into ring slot `slot` (prev updated by block nblk - 1), y = the filter's
 *         output with the bits of llzs_fir_stream_f32 for these spectra, e = d - y, and for the channels with mu != 0 g = mu E /
 *         (D + delta), D the power of the P spectra the product walked.
 * update: w_p += conj(X_(j-p)) g under the gradient constraint (samples from min(block, flt_len - p block) on zeroed), every p,
 *         every channel with mu != 0; the same block and slot as the filter launch in front of it. */
int llzs_fir_adapt_filter_f32(int block, int flt_len, const float *w, const float *tw, float *ring, float *prev, float *g,
                              const float *mu, float delta, const float *x, const float *d, float *e, float *y, int channels,
                              int nblk, int j, long pitch, int P, int R, int slot, void *stream);
int llzs_fir_adapt_update_f32(int block, int flt_len, float *w, const float *tw, const float *ring, const float *g,
                              const float *mu, int channels, int P, int R, int slot, void *stream);
/* the multi-reference adaptive filter (fir_adapt_matrix.hip, the error tail and the update kernel from adapt_steps.hpp, the
 * same as the filter's above; include/llz_adapt_matrix.h), block = 64 .. 2048, on the matrix convolver's rings: behind llzs_fir_matrix_fwd_f32 of a call's nblk blocks one power launch, then per block
 * llzs_fir_matrix_mac_f32 (nblk = 1, head = the block's slot, conn all ones), error and update, ordered by the stream.  w =
 * [outputs][inputs][P][block] complex laid out and scaled as hspec; den = [nblk][block] pairs of floats; g = [outputs][block]
 * complex scratch; mu = [outputs] step sizes on the device, 0 = the output is frozen; d, e, y = [outputs][pitch], y may be NULL.
 * power:  den[j] = delta + sum_i sum_p |ring_i[(slot + j - p) mod R]|^2, i ascending, p ascending within i, for every block j of
 *         the call; position 0 holds the DC and the Nyquist bin's denominators, every other position its own twice.
 * error:  block j: the `groups` partials of ypart ([groups][outputs][block]) added ascending, y with the bits of
 *         llzs_fir_matrix_inv_f32, e = d - y, and for the outputs with mu != 0 g = mu E / den (den: block j's row).
 * update: w[o][i][p] += conj(X_(i, j-p)) g_o under the gradient constraint, every path and partition of every output with
 *         mu != 0; slot = the block's ring slot.  The adapt_ppw override groups the partitions of a path; no bit depends on it. */
int llzs_fir_adapt_matrix_power_f32(int block, int flt_len, const float *ring, float *den, float delta, int inputs, int nblk,
                                    int P, int R, int slot, void *stream);
int llzs_fir_adapt_matrix_error_f32(int block, const float *ypart, const float *tw, const float *den, float *g, const float *mu,
                                    const float *d, float *e, float *y, int outputs, int groups, int j, long pitch, void *stream);
int llzs_fir_adapt_matrix_update_f32(int block, int flt_len, float *w, const float *tw, const float *ring, const float *g,
                                     const float *mu, int inputs, int outputs, int P, int R, int slot, void *stream);
/* the normalised LMS filter per band (adapt_bands.hip; include/llz_adapt_bands.h), float32: `taps` = K complex taps, 1..64, for
 * every (channel, bin), one launch for a call of `frames` >= 1 frames.  x, d, e, y = [channels][frames][bins], re and im apart,
 * y re and im both NULL or both set; w = [channels][K][bins] weights by age, h = [channels][max(K - 1, 1)][bins] history, row q
 * holding x[-1 - q] of the call; both are read, walked through the frames and written back.  mu = [channels] step sizes on the
 * device, 0 = the channel is frozen.  plan: out = {tap ceiling of the instance, threads per workgroup, workgroups, launches}. */
int llzs_bands_nlms_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere, float *eim,
                        float *yre, float *yim, float *wre, float *wim, float *hre, float *him, const float *mu, float delta,
                        int channels, int bins, int taps, int frames, void *stream);
int llzs_bands_nlms_plan(int channels, int bins, int taps, int *out);
/* its multi-reference form (adapt_bands_matrix.hip; include/llz_adapt_bands_matrix.h): `inputs` = I references, 1..8, of `taps`
 * = K complex taps each, I K <= 64, for every (output, bin), one launch for a call of `frames` >= 1 frames.  x = [inputs][frames]
 * [bins]; d, e, y = [outputs][frames][bins]; w = [outputs][inputs][K][bins] weights by age, read, walked and written back.  The
 * history [inputs][max(K - 1, 1)][bins], row q holding x_i[-1 - q] of the call, is shared by the outputs: hin is read, hout --
 * ANOTHER buffer -- takes the history behind the call's last frame, each element from one lane.  mu = [outputs] step sizes on the
 * device.  plan: out = {inputs of the instance, entry ceiling of the instance, threads per workgroup, workgroups, launches}. */
int llzs_matrix_bands_nlms_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere, float *eim,
                               float *yre, float *yim, float *wre, float *wim, const float *hin_re, const float *hin_im,
                               float *hout_re, float *hout_im, const float *mu, float delta, int inputs, int outputs, int bins,
                               int taps, int frames, void *stream);
int llzs_matrix_bands_nlms_plan(int inputs, int outputs, int bins, int taps, int *out);
/* the Kalman filter per band (kalman_bands.hip; include/llz_kalman_bands.h), float32: `taps` = K complex taps, 1..32, for every
 * (channel, bin), one launch for a call of `frames` >= 1 frames.  x, d, e, y, w and h as llzs_bands_nlms_f32 has them; var =
 * [channels][K][bins] state variances by age and noise = [channels][bins] noise powers, read, walked through the frames and
 * written back like w.  adapt = [channels] ints on the device, 0 = the channel is frozen.  consts = HOST {A2, 1 - A2, lam,
 * 1 - lam, delta}, the header's float32 constants.  plan: out = {tap ceiling of the instance, threads per workgroup, workgroups,
 * launches}. */
int llzs_kalman_bands_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere, float *eim,
                          float *yre, float *yim, float *wre, float *wim, float *hre, float *him, float *var, float *noise,
                          const int *adapt, const float *consts, int channels, int bins, int taps, int frames, void *stream);
int llzs_kalman_bands_plan(int channels, int bins, int taps, int *out);
/* its multi-reference form (kalman_bands_matrix.hip; include/llz_kalman_bands_matrix.h): `inputs` = I references, 1..8, of `taps`
 * = K complex taps each, I K <= 32, for every (output, bin), one launch for a call of `frames` >= 1 frames.  x, d, e, y, w, hin
 * and hout -- ANOTHER buffer -- as llzs_matrix_bands_nlms_f32 has them; var = [outputs][inputs][K][bins] state variances and noise
 * = [outputs][bins] noise powers, read, walked through the frames and written back like w.  adapt = [outputs] ints on the device,
 * 0 = the output is frozen (the history moves on all the same).  consts as llzs_kalman_bands_f32's.  plan: out = {inputs of the
 * instance, entry ceiling of the instance, threads per workgroup, workgroups, launches}. */
int llzs_mkalman_bands_f32(const float *xre, const float *xim, const float *dre, const float *dim, float *ere, float *eim,
                           float *yre, float *yim, float *wre, float *wim, const float *hin_re, const float *hin_im,
                           float *hout_re, float *hout_im, float *var, float *noise, const int *adapt, const float *consts,
                           int inputs, int outputs, int bins, int taps, int frames, void *stream);
int llzs_mkalman_bands_plan(int inputs, int outputs, int bins, int taps, int *out);
/* the noise and residual-echo postfilter per band (suppress_bands.hip; include/llz_suppress_bands.h), float32: a real gain for
 * every (channel, bin, frame), one launch for a call of `frames` >= 1 frames.  e, y (both NULL or both set), o and g (NULL: not
 * stored) = [channels][frames][bins].  state = [7][channels][bins], S Smin Stmp q N R Z, read, walked through the frames and
 * written back.  floors, leaks = [channels] floats and enable = [channels] ints on the device, 0 = the channel is passed through.
 * consts = HOST {omas, omaq, omad, omb, kt, aq, beta, rho, delta, t1}, the header's float32 constants; window = W.  n0 = the frame
 * count at the call's first frame folded into [0, 2 W): the count itself below W, else W + count % W.  plan: out = {with_y != 0,
 * threads per workgroup, workgroups, launches}. */
int llzs_suppress_bands_f32(const float *ere, const float *eim, const float *yre, const float *yim, float *ore, float *oim,
                            float *g, float *state, const float *floors, const float *leaks, const int *enable,
                            const float *consts, int window, int channels, int bins, int frames, int n0, void *stream);
int llzs_suppress_bands_plan(int channels, int bins, int with_y, int *out);
/* hist_new[c][:] = last (flt_len-1) samples of concat(hist_old[c], in[c][0:n]) */
int llzs_fir_tail_f32(const float *in, const float *hist_old, float *hist_new,
                      int channels, long n, long in_pitch, int flt_len, void *stream);
/* single channel, double, the reference's exact accumulation order (ascending k, multiply then add) */
int llzs_fir_td_f64(const double *in, double *out, const double *hist, const double *taps,
                    int n, int flt_len, void *stream);

/* ---- IIR ---- */
/* cascade of `stages` biquads; coef: stages x 5 doubles {b0,b1,b2,a1,a2}; state: [channels][stages][4] doubles
 * {x1,x2,y1,y2} per stage, read and written. */
int llzs_iir_cascade_f32(const float *in, float *out, const double *coef, double *state,
                         int channels, int n, long in_pitch, long out_pitch, int stages, void *stream);
/* fast path (stage pipeline + lanes along time): n % 1024 == 0, 16-byte aligned rows.  pd = [stages][6][4] powers
 * P^(2^d) of P = A^16 with A = [[-a1,-a2],[1,0]], pl = [stages][64][12] = P^lane, P^(lane%16+1), P^(lane%32+1); same coef / state layout as above. */
#define LLZS_IIR_PIPE_CHUNK 1024     /* 64 lanes x 16 samples */
int llzs_iir_cascade_pipe_f32(const float *in, float *out, const double *coef, const double *pd, const double *pl,
                              const double *state_in, double *state_out /* a different buffer: segments of one launch
                                                                         * are not ordered */, int channels, int n, long in_pitch, long out_pitch, int stages,
                              int warm_chunks /* 0: never split a channel along time */,
                              int float32 /* 1: float32 arithmetic (every section passed the host's noise-gain check) */,
                              void *stream);
/* cascades of up to 8 sections with a short memory: a wave owns a (channel, time segment) and runs all sections in
 * registers (iir.hip: one row of IIR_WAVE_ROWS per form).  n a multiple of the form's chunk, 16-byte aligned rows,
 * warm_chunks >= 1 in units of 1024 samples whatever the form; state as above, read and written in different buffers.
 * Tables (powers of P = A^16 or A^32, A = [[-a1,-a2],[1,0]]; the 32-sample forms fold the b0 gains out: b' = b / b0,
 * xfac_s = prod_{t >= s} b0_t, yfac_s = xfac_(s+1), in_gain = xfac_0):
 *   WAVE16_F32  k_iir_cascade_wave_pk    floats: cf [S][24] = (h1[k], h2[k]) k < 8, the outputs at k of the unit start states,
 *                                        then b0 b1 b2 a1 a2 and 3 pad; pd [S][16] = P^(2^d) d < 4; pl [S][64][12]
 *   WAVE16_F64  k_iir_cascade_wave_pf64  the stage pipeline's own tables: cf = coef [S][5], pd [S][6][4], pl [S][64][12]
 *   WAVE32_F32  k_iir_cascade_wave_pk32  floats: cf [S][40] = (h1[k], h2[k]) k < 16, then 1 b1' b2' a1 a2 xfac yfac pad; pd, pl
 *                                        as for WAVE16_F32
 *   WAVE32_F64  k_iir_cascade_wave_pf64w doubles: cf [S][8] = b1', b2', a1, a2, xfac, yfac, 0, 0; pd [S][16]; pl [S][448] =
 *                                        P^lane for 64 lanes, P^(i+1) i < 16, P^(i+1) i < 32
 *   BANK16_F32  k_iir_cascade_wave_pk<S, true>    the tables of WAVE16_F32 per channel: cf [C][S][24], pd [C][S][16],
 *                                        pl [C][S][64][12]
 * The bank form (llz_iir_bank_mc: a coefficient set per channel) runs one item per 64-thread workgroup; a bank in double has
 * no wave form (the bank pipeline measured faster). */
enum { LLZS_IIR_WAVE16_F32, LLZS_IIR_WAVE16_F64, LLZS_IIR_WAVE32_F32, LLZS_IIR_WAVE32_F64, LLZS_IIR_BANK16_F32,
       LLZS_IIR_WAVE_FORMS };
#define LLZS_IIR_WAVE_IS32(form) ((form) == LLZS_IIR_WAVE32_F32 || (form) == LLZS_IIR_WAVE32_F64)
#define LLZS_IIR_WAVE_CHUNK(form) (LLZS_IIR_WAVE_IS32(form) ? 2048 : 1024)
typedef struct {
    const void *cf, *pd, *pl;
    double in_gain;             /* the 32-sample forms scale the input once */
} llzs_iir_wave_tables;
int llzs_iir_cascade_wave(int form, const llzs_iir_wave_tables *t, const float *in, float *out, const double *state_in,
                          double *state_out, int channels, int n, long in_pitch, long out_pitch, int stages, int warm_chunks,
                          void *stream);
/* the tail and the stage pipeline with a coefficient set per channel (llz_iir_bank_mc): the same arguments, with coef
 * [channels][stages][5], pd [channels][stages][6][4], pl [channels][stages][64][12] */
int llzs_iir_bank_f32(const float *in, float *out, const double *coef, double *state,
                      int channels, int n, long in_pitch, long out_pitch, int stages, void *stream);
int llzs_iir_bank_pipe_f32(const float *in, float *out, const double *coef, const double *pd, const double *pl,
                           const double *state_in, double *state_out, int channels, int n, long in_pitch, long out_pitch,
                           int stages, int warm_chunks, int float32, void *stream);
/* the plan such a launch of n samples would run with, nothing launched: form < 0 the stage pipeline, else a wave form;
 * out = {segments per channel, chunks per segment, warm-up chunks} in chunks of the form's own size */
int llzs_iir_cascade_plan(int form, int channels, int n, int stages, int warm_chunks, int out[3]);
/* general direct form I, one channel, double, the reference's exact operation order (llz_iir.c:103-132).
 * xs: N+1 doubles, ys: M+1 doubles (delay lines, read and written) */
int llzs_iir_df1_f64(const double *in, double *out, const double *a, const double *b, double *xs, double *ys,
                     int M, int N, int n, void *stream);
/* the same recurrence for many channels (iir_df1.hip): float32 in / out, double arithmetic in the reference's order; ab =
 * a[0..ord] then b[0..ord] zero padded (ord = llzs_iir_df1_mc_max_order()); state [channels][2][ord + 1] = the reference's x[]
 * then y[] delay lines, read from state_in and written to state_out (two buffers); segs time segments per channel, later ones
 * warmed up over `warm` samples from zero delay lines */
int llzs_iir_df1_mc_f32(const float *in, float *out, const double *ab, const double *state_in, double *state_out, int channels,
                        long n, long in_pitch, long out_pitch, int M, int N, int segs, int warm, void *stream);
int llzs_iir_df1_mc_max_order(void);
/* the segment count llzs_iir_df1_mc_f32 runs with when asked for `segs` (every segment non-empty and at least `warm` long) */
int llzs_iir_df1_mc_segments(long n, int segs, int warm);

/* ---- resample ---- */
/* y[c][i] = gain * sum_{k<Q} x[c][(i0+i)*M/L - k - in0] * g[(i0+i)%L][k], x before the call start comes from
 * hist[c][Q-1 + idx] (hist holds the previous Q-1 samples).  i0 = global index of the first output of this call,
 * in0 = global index of the first input sample of this call.  n_out outputs per channel. */
int llzs_resample_f32(const float *in, float *out, const float *hist, const float *g,
                      int channels, long n_in, long n_out, long in_pitch, long out_pitch,
                      int L, int M, int Q, float gain, long long i0, long long in0, void *stream);
/* general L/M float32 on the fp32 matrix cores (resample_mfma.hip): atab [ceil(L/16)][steps][64] = the banded tap matrix in
 * MFMA operand order with the gain folded in (steps = llzs_resample_mfma_f32_table_steps), c0tab [ceil(L/16)] =
 * floor(16 t M / L).  The call must start on a period boundary (input index % M == 0, output index % L == 0); the phase-tile
 * form declines n_out % L != 0 with LLZ_ERR_RANGE (it stores whole periods), the period-tile form bounds its stores by n_out. */
int llzs_resample_mfma_f32(const float *in, float *out, const float *hist, const float *atab, const int *c0tab,
                           int channels, long n_in, long n_out, long in_pitch, long out_pitch, int L, int M, int Q,
                           void *stream);
int llzs_resample_mfma_f32_fits(int L, int M, int Q);
int llzs_resample_mfma_f32_table_steps(int L, int M, int Q);
/* L = 1 (decimate by M) float32 fast path: gp = M x tp phase taps gp[m][j] = g[j*M+m], zero padded, tp % 16 == 0;
 * input index of output i is i*M (calls start on a period boundary); hist as above. */
int llzs_resample_dec_f32(const float *in, float *out, const float *hist, const float *gp, int channels,
                          long n_in, long n_out, long in_pitch, long out_pitch, int M, int Q, int tp,
                          float gain, void *stream);
int llzs_resample_dec_f32_fits(int M, int tp);     /* 1 when the fast path's LDS image fits */
/* int16 PCM, double taps, double accumulate in ascending k with separate multiply and add, clamp, truncate */
int llzs_resample_i16(const short *in, short *out, const short *hist, const double *g,
                      int channels, long n_in, long n_out, long in_pitch, long out_pitch,
                      int L, int M, int Q, double gain, long long i0, long long in0, void *stream);
/* the same bit-exact int16 result for L >= 2, screened on the int8 matrix cores per phase (resample_i8.hip): atab [ceil(L/16)]
 * [steps][5][64][16] tap digits in operand order (steps = llzs_resample_i16x_ksteps), aoff [ceil(L/16)] band starts, bqtab
 * [16 ceil(L/16)][4] = floor(128 sum_k G_f[k] / 256) as (lo, hi), the phase's own e32, first | last << 8 non-zero tap | exact
 * << 16; g the L x Q double taps, eps the largest per-phase bound, any_exact: some phase carries the exact flag.
 * The call must start on a period boundary (input index % M == 0, output index % L == 0) and hold whole periods: n_out % L != 0
 * is declined with LLZ_ERR_RANGE (the kernel stores whole periods). */
int llzs_resample_i16x(const short *in, short *out, const short *hist, const signed char *atab, const int *aoff,
                       const int *bqtab, const double *g, int channels, long n_in, long n_out, long in_pitch, long out_pitch,
                       int L, int M, int Q, int shift, double gain, double eps, int any_exact, void *stream);
int llzs_resample_i16x_fits(int L, int M, int Q);
int llzs_resample_i16x_ksteps(int L, int M, int Q);
/* the launch a call would make (measurement / documentation): plan[0..6] = waves per workgroup, periods per span, spans per
 * workgroup, workgroups, workgroups resident per CU, LDS bytes per workgroup, 1 when a wave takes several phase tiles */
int llzs_resample_i16x_plan(int L, int M, int Q, int channels, long n_out, int shift, int *plan);
int llzs_tail_i16(const short *in, const short *hist_old, short *hist_new, int channels, long n, long in_pitch,
                  int keep, void *stream);
/* llz_decimate (forward indexed polyphase sum over a history of n samples) and llz_interp (no history),
 * single channel int16, exact order: see llz_resample.c:457-483 and :515-536 */
int llzs_decimate_i16(const short *buf /* n hist + num_in */, short *out, const double *p, int M, int K, int n,
                      int num_out, double gain, void *stream);
int llzs_interp_i16(const short *x /* num_in + K zero padded */, short *out, const double *p, int L, int K,
                    int num_in, double gain, void *stream);

/* ---- arbitrary-ratio resampler (asrc.hip; include/llz_asrc.h) ----
 * state: [channels] llz_asrc_state (llz_asrc_time.h) on the device, a channel's position, step and glide in front of the
 * call; table: [phases + 1] rows of LLZ_ASRC_PITCH(T) floats; hist: [channels][T - 1], the samples in front of in
 * ([channels][in_pitch], n_in >= 1 of them).  llzs_asrc_f32 stores output j < count_c of channel c, count_c the state's own
 * count for n_in, to out[c][j] and nothing else; max_count: the largest count (>= 1), which sizes the grid; table_lds: 1 = the
 * table is loaded into LDS (LLZ_ERR_RANGE beyond LLZ_ASRC_LDS_TABLE_BYTES), 0 = read through the caches; the same bits either
 * way.  llzs_asrc_advance moves every channel's state behind the call. */
int llzs_asrc_f32(const float *in, float *out, const float *hist, const float *table, const void *state, int channels,
                  long n_in, long in_pitch, long out_pitch, int T, int phases, int table_lds, long max_count, void *stream);
int llzs_asrc_advance(void *state, int channels, long n_in, int T, void *stream);

/* ---- FFT ---- */
/* float32 batch, in place; cs = size cos then size sin values (float). inverse: 0 forward, 1 inverse (divides by size) */
int llzs_fft_f32(float *data, int count, int size, const float *cs, int inverse, void *stream);
/* double, one transform, exact reference butterfly order and rounding (no contraction) */
int llzs_fft_f64(double *data, int size, const double *cs, int inverse, void *stream);
/* int32 data, Q15 twiddles (size cos then size sin shorts), bit-exact */
int llzs_fft_fixed(int *data, int count, int size, const short *cs, int inverse, void *stream);
/* transforms of 8192 .. LLZS_FFT_MAX points (fft_large.hip), in place, same contract as the two above.  cs: the size-point
 * table.  twb (float32): a device buffer of llzs_fft_large_twb_bytes(size) bytes, filled once by
 * llzs_fft_large_twb.  llzs_fft_large_passes: passes over device memory of one transform. */
#define LLZS_FFT_MAX (1 << 24)
int llzs_fft_large_f32(float *data, int count, int size, const float *cs, const float *twb, int inverse, void *stream);
int llzs_fft_large_f64(double *data, int size, const double *cs, int inverse, void *stream);
int llzs_fft_large_twb_bytes(int size);
int llzs_fft_large_twb(float *twb, int size, const float *cs, void *stream);
int llzs_fft_large_passes(int size, int f32);

/* ---- correlation ---- */
/* r[k] = sum_i x[i]*y[i+k], k = 0..p, one channel, double, the reference's summation order (llz_corr.c:38-58) */
int llzs_corr_exact_f64(const double *x, const double *y, int n, int p, double *r, void *stream);
/* frames x n float32 -> frames x (p+1), direct form */
int llzs_autocorr_mc_f32(const float *x, float *r, int frames, int n, int p, void *stream);
/* r[f][k] = sum_i x[f][i]*y[f][i+k] on the same kernels (x == y: the same bits as llzs_autocorr_mc_f32); two_sided = 0:
 * frames x (p+1); 1: frames x (2p+1), lag k at index p+k (the negative lags: the rows swapped, lags 1..p) */
int llzs_crosscorr_mc_f32(const float *x, const float *y, float *r, int frames, int n, int p, int two_sided, void *stream);
/* c[f] = <a,b> / sqrt(<a,a><b,b>): float32 sums, the quotient in double */
int llzs_corr_cof_mc_f32(const float *a, const float *b, float *c, int frames, int n, void *stream);
/* pointwise steps of the FFT cross-correlation around llzs_fft_f32 (F points, z: frames x F complex): z = x + i y zero-padded;
 * conj(X) Y separated from Z[k] and conj(Z[F-k]), in place; lags 0..p or -p..p (lag -k at bin F-k) of the inverse transform */
int llzs_xcf_pack(const float *x, const float *y, float *z, int frames, int n, int F, void *stream);
int llzs_xcf_product(float *z, int frames, int F, void *stream);
int llzs_xcf_extract(const float *z, float *r, int frames, int p, int two_sided, int F, void *stream);
/* pointwise steps of the FFT form around llzs_fft_f32: real -> zero-padded complex; |X|^2 of the first n bins; 2*Re */
int llzs_acf_pack(const float *x, float *z, int frames, int n, int F, void *stream);
int llzs_acf_power(float *z, int frames, int n, int F, void *stream);
int llzs_acf_extract(const float *z, float *r, int frames, int p, int F, void *stream);
/* the same five steps fused in LDS (acf_fft.hip): one read of the frames, p+1 floats written per frame */
int llzs_acf_fused_f32(const float *x, float *r, int frames, int n, int p, int size, const float *cs, void *stream);

/* ---- Welch cross-spectra (csd.hip; include/llz_spectral.h) ----
 * Frames are counted from the handle's last reset; frame f covers samples [(f - hops0) hop, (f - hops0) hop + fft_len) of the
 * call's x ([channels][x_pitch]), negative indices in hist ([channels][fft_len - hop], the samples in front of the call; may be
 * NULL when hop == fft_len), hops0 = the hops taken before the call.  The call holds frames [f_lo, f_hi); run r = frames
 * [32 r, 32 r + 32).  One launch walks the runs [r0, r0 + nruns) of every pair: a run that began before f_lo starts from
 * carry_in ([2][pairs][bins][4] floats: Sxx, Syy, Re Sxy, Im Sxy, then the compensation terms of these compensated float32
 * sums), a run that ends behind f_hi goes to carry_out, ANOTHER buffer of that layout (both can happen in one launch, in work
 * items that nothing orders), a finished run's sums go to scratch slot (r - r0) of [nruns][pairs][bins][4] floats.  pair_xy:
 * [pairs][2] channel indices, checked by the caller.
 * w: fft_len window floats; cs: cos then sin of 2 pi i / fft_len.  fft_len 64..4096, hop fft_len, fft_len / 2 or fft_len / 4. */
int llzs_csd_form(int fft_len);         /* 1: the register form serves this size under the tunes set now, 0: the staged form */
int llzs_csd_runs_f32(const float *x, const float *hist, const float *w, const float *cs, const int *pair_xy, float *scratch,
                      const float *carry_in, float *carry_out, int pairs, int fft_len, int hop, long x_pitch, long hops0, long f_lo, long f_hi, long r0,
                      int nruns, void *stream);
/* acc ([pairs][bins][4] doubles) += the first nfin slots of scratch, in slot order */
int llzs_csd_fold_f64(const float *scratch, double *acc, int pairs, int bins, int nfin, void *stream);
/* the read-outs from acc + the sums in carry (its first [pairs][bins][4]; NULL: no run is open), in double, rounded once: what 0..4 = LLZ_SPEC_PXX .. LLZ_SPEC_TF
 * into out ([pairs][bins] floats, CSD and TF [pairs][bins][2]), ku = frames x sum w^2; what 5: the four sums into raw */
int llzs_csd_read_f64(const double *acc, const float *carry, int pairs, int bins, int what, double ku, float *out, double *raw,
                      void *stream);

/* ---- time-delay estimator (tde.hip; include/llz_tde.h) ----
 * Framing as the cross-spectra's above: frame f covers samples [(f - hops0) hop, (f - hops0) hop + fft_len) of the call's x
 * ([channels][x_pitch]), negative indices in hist ([channels][fft_len - hop]; may be NULL when hop == fft_len).  One launch, a
 * workgroup per pair, walks frames [f_lo, f_hi) in order: state ([pairs][bins][4] = Re S, Im S, Gx, Gy) is read when f_lo > 0 and
 * written back; frame 0 starts the recursion, lam == 0 takes S = P; delay: [pairs][delay_pitch], peak (may be NULL): [pairs][peak_pitch], element
 * f - f_lo of each row; curve: [pairs][2 max_lag + 1], the curve of frame f_hi - 1 at lags -max_lag .. max_lag.  weight 0 CC,
 * 1 PHAT, 2 SCOT over bins k_lo .. k_hi; g = (float)(1 - (double)lam).  pair_xy checked by the caller. */
int llzs_tde_frames_f32(const float *x, const float *hist, const float *w, const float *cs, const int *pair_xy, float *state,
                        float *curve, float *delay, float *peak, int pairs, int fft_len, int hop, long x_pitch, long hops0,
                        long f_lo, long f_hi, long delay_pitch, long peak_pitch, int max_lag, int weight, int k_lo, int k_hi, float lam, float g,
                        float delta, void *stream);

/* ---- DFT of any length and zoom transform by the chirp-z algorithm (dft.hip; include/llz_dft.h) ----
 * A row of n points becomes k outputs through two m-point transforms, m a power of two >= n + k - 1 (at least 8): a = x pre,
 * zero-padded; A = FFT_m(a); B = A v; b = IFFT_m(B) unscaled; out[j] = b[j] post[j], j < k.  pre [n], v [m], post [k] complex
 * floats, the host's tables (llz_dft_host.c); cs: cos then sin of 2 pi i / m.  in: count rows in_pitch >= 1 elements apart, out:
 * out_pitch >= k apart, elements of the buffer's own kind.  mode 0: complex rows in and out; 1: real rows in; 2: bins 0 .. n / 2
 * in, extended to the Hermitian row of n (the imaginary parts of the real bins dropped), and real rows out.
 * fused: m <= 4096, one launch, v = FFT_m(.) / m in the ORDER OF A DECIMATION-IN-FREQUENCY TRANSFORM'S OUTPUT (entry i = bin
 * bitrev(i)).  plan: out = {rows per workgroup, LDS bytes} of such a launch, nothing launched.
 * pack, mul, extract: the composed form's steps around llzs_fft_f32 / llzs_fft_large_f32 (forward, then inverse, which divides
 * by m) on z = [count][m] complex, m <= 2^21, v = FFT_m(.) in natural order. */
int llzs_dft_plan(int m, int count, int *out);
int llzs_dft_fused_f32(const float *in, float *out, const float *pre, const float *v, const float *post, const float *cs,
                       int count, int n, int k, int m, long in_pitch, long out_pitch, int mode, void *stream);
int llzs_dft_pack_f32(const float *in, float *z, const float *pre, int count, int n, int m, long in_pitch, int mode,
                      void *stream);
int llzs_dft_mul_f32(float *z, const float *v, int count, int m, void *stream);
int llzs_dft_extract_f32(const float *z, float *out, const float *post, int count, int k, int m, long out_pitch, int mode,
                         void *stream);

/* ---- linear prediction (lpc.hip) ---- */
/* LPC of frames x n float32 (0 <= p <= 32): the correlation of llzs_autocorr_mc_f32 (the same bits; on x*win when win is not
 * NULL) and the Levinson-Durbin recursion in double in one launch.  acof [frames][p+1]; kcof [frames][p], err, gain
 * [frames] and r [frames][p+1] may be NULL */
int llzs_lpc_fused_f32(const float *x, const float *win, float *acof, float *kcof, float *err, float *gain, float *r,
                       int frames, int n, int p, void *stream);
/* the recursion alone from r [frames][p+1] (0 <= p <= 64), outputs as above; n divides the error */
int llzs_levinson_f32(const float *r, float *acof, float *kcof, float *err, float *gain, int frames, int n, int p,
                      void *stream);
/* y[f][i] = x[f][i] * win[i] (float32, one rounding) */
int llzs_window_f32(const float *x, const float *win, float *y, int frames, int n, void *stream);

/* ---- the filters that apply LPC coefficients (lpc_filter.hip; include/llz_lpc.h part 3) ----
 * x, e, y planar [channels][frames * frame_len]; acof [channels][frames][p + 1], entry 0 of a set is not read; 0 <= p <= 64,
 * p < frame_len.  Rows and coefficient sets need their element's alignment only.
 * residual: e[t] = x[t] + sum_k a_f[k] x[t - k] as a float32 fma chain over k = p .. 1.  hist_in / hist_out: [channels][64]
 * floats, [c][i] = x(-1 - i) in front of / behind the call (i < p), two different buffers */
int llzs_lpc_residual_f32(const float *x, const float *acof, float *e, const float *hist_in, float *hist_out, int channels,
                          int frames, int frame_len, int p, void *stream);
/* synthesis: y[t] = e[t] - sum_k a_f[k] y[t - k] in double over k = p .. 1, rounded multiply then rounded subtract, stored as
 * float32.  state: [channels][64] doubles, [c][i] = the unrounded y(-1 - i) (i < p), updated in place */
int llzs_lpc_synth_f32(const float *e, const float *acof, float *y, double *state, int channels, int frames, int frame_len,
                       int p, void *stream);

/* windowed-FFT frames (llz_asmodel.c:180-310), float32 batch, fft_len 8..4096 in one launch per direction: x planar
 * [C][frames*F] (row pitch x_pitch), spectra [C][frames][size/2+1]; hist / ola: [C][size-F] state carried between calls
 * (ola_old != ola_new); w: size floats; cs: cos then sin of 2*pi*i/size */
int llzs_stft_analysis_f32(const float *x, const float *hist, float *re, float *im, const float *w, const float *cs,
                           int channels, int frames, int F, int size, long x_pitch, void *stream);
int llzs_stft_synthesis_f32(const float *re, const float *im, float *x, const float *ola_old, float *ola_new,
                            const float *w, const float *cs, int channels, int frames, int F, int size, long x_pitch,
                            float magic, void *stream);
/* the composed form (stft_large.hip) for fft_len above 4096, and 4096 under the fft_generic tune: per chunk of
 * `count` consecutive transforms g0 .. g0+count-1 (g = c * frames + f), z: count * N interleaved complex scratch points.
 * frames: windowed frames into z; bins: bins 0..N/2 of z into re / im; mirror: Hermitian extension of re / im into z;
 * ola: overlap-add of the inverse-transformed z into x, tail read from ola_old (a channel's first frame) or ola_new and
 * written to ola_new through `tail` ((channels in the chunk) * (N - F) floats).  A chunk holds at most
 * LLZS_STFT_CHUNK_POINTS points (at least one transform). */
#define LLZS_STFT_CHUNK_POINTS (1 << 24)
int llzs_stft_frames_large_f32(const float *x, const float *hist, float *z, const float *w, int frames, int F, int N,
                               long x_pitch, long g0, int count, void *stream);
int llzs_stft_bins_large_f32(const float *z, float *re, float *im, int N, long g0, int count, void *stream);
int llzs_stft_mirror_large_f32(const float *re, const float *im, float *z, int N, long g0, int count, void *stream);
int llzs_stft_ola_large_f32(const float *z, float *x, const float *ola_old, float *ola_new, float *tail, const float *w,
                            int frames, int F, int N, long x_pitch, long g0, int count, float magic, void *stream);

/* ---- polyphase DFT filter bank (pfb.hip; include/llz_pfb.h), float32, M bands, hop D, prototype length L = P M ----
 * x planar [C][frames*D] (row pitch x_pitch), spectra [C][frames][M/2+1]; cs: cos then sin of 2*pi*i/M.  rot0, rstep: frame f
 * of the call is rotated by (rot0 + f rstep) mod M (FRAME phase: 0, 0; TIME phase: (m + 1) D mod M of the call's first frame, D).
 * analysis: hist [C][L-D], the samples in front of x; w: L floats.  Synthesis runs per chunk of `count` frames f0 .. f0+count-1
 * of the call: inverse writes the real inverse transforms, rotation undone, to u = [C][count][M]; ola adds g[i] u[i mod M] onto
 * the tail ([C][L-D], tail_old != tail_new), oldest frame first, count D samples to x (the chunk's first sample) and the rest to
 * tail_new.  plan: out[0..3] = analysis form (0 LDS span, 1 through the caches), frames per workgroup, workgroups, LDS bytes;
 * out[4..7] = synthesis form (1), frames per workgroup, workgroups and LDS bytes of inverse over a chunk of `chunk` frames. */
int llzs_pfb_analysis_f32(const float *x, const float *hist, float *re, float *im, const float *w, const float *cs,
                          int channels, int frames, int M, int D, int L, int rot0, int rstep, long x_pitch, void *stream);
int llzs_pfb_inverse_f32(const float *re, const float *im, float *u, const float *cs, int channels, int frames, int f0,
                         int count, int M, int D, int rot0, int rstep, void *stream);
int llzs_pfb_ola_f32(const float *u, float *x, const float *tail_old, float *tail_new, const float *g, int channels, int count,
                     int M, int D, int L, long x_pitch, void *stream);
int llzs_pfb_plan(int channels, int frames, int chunk, int M, int D, int L, int *out);

/* MDCT (llz_mdct.c): y[r] = sum_c x[c]*A[r][c] in ascending c, separately rounded multiply and add (device doubles) */
int llzs_matvec_exact_f64(const double *A, const double *x, double *y, int rows, int cols, void *stream);
/* twiddle steps of the FFT forms in double, exact order, device data (mdct.hip): quarter 0 = N-point form, 1 = N/4-point
 * form; post 0 = the step in front of the transform, 1 = the step behind it; cs2: (cos, sin) pairs */
int llzs_mdct_rot_f64(int quarter, int post, const double *in, double *out, const double *cs2, int N, int inverse,
                      double cof, void *stream);
/* fixed-point MDCT steps (mdct_q15.hip), `count` frames per launch, int32 data, Q15 tables, wrapping adds:
 * sums: y[f][r] = sum_c q15(x[f][c], A[r][c]) (llz_mdct_fixed.c:116-152), then (4 y) / quarter_over_n when that is not 0;
 * step: the twiddle steps of the two FFT forms (llz_mdct_fixed.c:155-283); quarter 0 = N-point form, 1 = N/4-point form;
 * post 0 = the step in front of the transform, 1 = the step behind it; tw: (cos, sin) Q15 pairs; cof = Q15 1/sqrt(N) */
int llzs_mdctq_sums(const short *A, const int *x, int *y, int count, int rows, int cols, int quarter_over_n, void *stream);
int llzs_mdctq_step(int quarter, int post, const int *in, int *out, const short *tw, int count, int N, int inverse,
                    int cof, void *stream);
/* the N/4-point form whole in one launch (fold, transform, unfold in LDS): N a power of two in 8..16384; pre / post: the two
 * step tables of this direction; cs: the N/4-point transform's table */
int llzs_mdct4_q15(const int *in, int *out, int count, int N, const short *pre, const short *post, const short *cs,
                   int inverse, int cof, void *stream);
/* the N-point form whole in one launch: N a power of two in 4..4096; pre N pairs, post N/2 (forward) or N (inverse) pairs */
int llzs_mdct1_q15(const int *in, int *out, int count, int N, const short *pre, const short *post, const short *cs, int inverse,
                   void *stream);
/* framing of the single-channel analysis / synthesis symbols in double, exact order (frames_f64.hip; llz_asmodel.c:177-462):
 * slide_window: held_next = (held << hop) ++ fresh, dst = held_next * window (interleaved complex with zero imaginary part
 * when as_complex); split / mirror: interleaved spectrum <-> planes [re 0..N/2 | im 0..N/2]; overlap_add: acc + src * window,
 * the first hop sums leave scaled, the rest slides down into acc_next, zeros enter at the top (acc != acc_next) */
int llzs_frame_slide_window_f64(const double *fresh, const double *held, double *held_next, const double *window,
                                double *dst, int N, int hop, int as_complex, void *stream);
int llzs_spectrum_split_f64(const double *z, double *planes, int bins, void *stream);
int llzs_spectrum_mirror_f64(const double *planes, double *z, int N, void *stream);
int llzs_frame_overlap_add_f64(const double *src, int src_stride, const double *window, const double *acc,
                               double *acc_next, double *leaving, int N, int hop, double scale, void *stream);
int llzs_scale_4_over_n_f64(double *v, int n, double divisor, void *stream);   /* v = (v * 4) / divisor, two roundings */
/* N/4-point-FFT MDCT / IMDCT of `count` float32 frames: forward [count][N] -> [count][N/2], inverse the other way;
 * tc/ts: cos/sin of -2*pi*(k+1/8)/N, k < N/4; cs: cos then sin of 2*pi*i/(N/4) */
int llzs_mdct4_f32(const float *in, float *out, int count, int N, const float *tc, const float *ts, const float *cs,
                   int inverse, void *stream);
/* the same on the register transforms for N in {256, 512, 1024, 2048, 4096, 8192}; LLZ_ERR_RANGE for other N */
int llzs_mdct4_reg_f32(const float *in, float *out, int count, int N, const float *tc, const float *ts, const float *cs,
                       int inverse, void *stream);
/* windowed 50 %-overlap MDCT frames in batch on the same kernels (N in {256 .. 8192}, F = N/2): analysis x [channels][frames F]
 * -> X [channels][frames][F]; synthesis the other way with overlap-add.  win [N]; state_in / state_out [channels][F]
 * (analysis: the previous frame; synthesis: the overlap-add tail), two different buffers */
int llzs_mdct4_frames_f32(const float *in, float *out, int channels, int frames, int N, const float *tc, const float *ts,
                          const float *cs, const float *win, const float *state_in, float *state_out, int inverse,
                          void *stream);

/* ---- PCM ingest / egress ---- */
int llzs_pcm_deinterleave_i16_f32(const short *in, float *out, int channels, long n, float scale, void *stream);
int llzs_pcm_interleave_f32_i16(const float *in, short *out, int channels, long n, float scale, void *stream);

/* ---- synthetic PCM ---- */
int llzs_synth_f32(float *dst, int channels, long n, long pitch, unsigned seed, int chan0, void *stream);
int llzs_synth_i16(short *dst, int channels, long n, long pitch, unsigned seed, int chan0, void *stream);

#ifdef __cplusplus
}
#endif
#endif
