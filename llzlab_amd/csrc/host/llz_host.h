/* llz_host.h -- INTERNAL helpers shared by the host C layer */
#ifndef LLZ_HOST_H
#define LLZ_HOST_H

#include <stddef.h>
#include "../../../include/llz_hip.h"
#include "../../../include/llz_fir.h"
#include "../llz_shim.h"

enum { LLZ_KIND_LPF = 0, LLZ_KIND_HPF = 1, LLZ_KIND_BPF = 2, LLZ_KIND_BSF = 3 };

/* windowed-sinc design shared by the four llz_fir_*_cof symbols; *out is malloc'ed, returns the tap count
 * (odd-forced for HPF/BPF/BSF) or -1 */
int llz_host_design(int kind, double **out, int n, double fc1, double fc2, win_t win);

/* handle tags: a wrong or stale handle fails the tag check instead of dereferencing garbage */
enum {
    LLZ_TAG_FIR1 = 0x4c5a4631, LLZ_TAG_FIRM = 0x4c5a464d, LLZ_TAG_IIR1 = 0x4c5a4931, LLZ_TAG_IIRM = 0x4c5a494d,
    LLZ_TAG_RS1 = 0x4c5a5231, LLZ_TAG_RSM = 0x4c5a524d, LLZ_TAG_FFT1 = 0x4c5a5431, LLZ_TAG_FFTB = 0x4c5a5442,
    LLZ_TAG_FFTX = 0x4c5a5458, LLZ_TAG_FIRB = 0x4c5a4642, LLZ_TAG_IIRB = 0x4c5a4942, LLZ_TAG_FIRS = 0x4c5a4653,
    LLZ_TAG_FIRX = 0x4c5a4658, LLZ_TAG_ADPT = 0x4c5a4144, LLZ_TAG_ADPX = 0x4c5a4158,
    LLZ_TAG_ASRC = 0x4c5a5352, LLZ_TAG_PFB = 0x4c5a5046, LLZ_TAG_ADPB = 0x4c5a4142,
    LLZ_TAG_ADBX = 0x4c5a4258, LLZ_TAG_KALB = 0x4c5a4b42,
    LLZ_TAG_SUPB = 0x4c5a5342, LLZ_TAG_KALX = 0x4c5a4b58, LLZ_TAG_DFTM = 0x4c5a4446
};

#define LLZ_HANDLE_OK(h, type, tagv) ((h) != 0 && (h) != LLZ_BAD_HANDLE && ((type *)(h))->tag == (tagv))

/* one frame of a llz_mdct_init() handle between two device buffers of doubles (llz_mdct_host.c; used by the frame handles
 * of llz_asmodel_host.c): forward N samples -> N/2 coefficients, inverse the other way; d_src != d_dst */
int llz_host_mdct_on_device(unsigned long handle, const double *d_src, double *d_dst, int inverse);

/* ---- the head of a handle (llz_util.c) ----
 * The handles of the transform and analysis family start with this head, so one lookup, one set_stream and one retire serve
 * them all.  device: the device the handle's buffers live on, bound by every call; stream: NULL for the handles without one. */
typedef struct {
    int tag, device;
    void *stream;
} llz_head_t;
/* a zeroed handle of `size` bytes with its tag set and (on_device) the current device taken; NULL when out of host memory.  An
 * init that fails calls its destroy on the partly built handle: every destroy takes a handle with any of its members still zero */
void *llz_handle_new(size_t size, int tag, int on_device);
/* the handle, or NULL -- with the message "<who>: bad handle" when who is not NULL */
void *llz_handle(unsigned long handle, int tag, const char *who);
int   llz_handle_set_stream(unsigned long handle, int tag, const char *who, void *stream);
/* the uninit of a handle: its device entered, its stream synchronised, destroy(handle), the device left; nothing on a bad handle */
void  llz_handle_retire(unsigned long handle, int tag, void (*destroy)(void *));

/* ---- llz_tables.c: the window, twiddle and MDCT tables of the transform and analysis family ----
 * Every builder returns DEVICE memory (llzs_malloc, filled through llzs_h2d on the default stream) or NULL; the values come from
 * libm in the reference's own expressions and operation order, so that a table is the reference's to the last bit. */

/* Hamming / Blackman / Kaiser (llz_fir.c:61-158) by win_t; 0: unknown window, nothing written */
int llz_host_window(double *w, int n, win_t win_type);
/* a device copy of `bytes` of host memory; of `count` doubles rounded to float; `bytes` of zeros */
void  *llz_host_upload(const void *host, size_t bytes);
float *llz_host_upload_f32(const double *host, size_t count);
void  *llz_host_zeros(size_t bytes);
/* cos then sin of 2 pi i / size, i < size, as llz_fft_init builds them (llz_fft.c:222-229): in double, rounded to float once,
 * and in Q15 as llz_fft_fixed_init does (llz_fft_fixed.c:243-247) */
double *llz_host_cs_f64(int size);
float  *llz_host_cs_f32(int size);
short  *llz_host_cs_q15(int size);
/* LLZ_FIX15 of the reference (llz_fft_fixed.h:42-66): v * 2^15 rounded half away from zero, saturated to int32, clipped to
 * +-32767 */
short llz_host_q15(double v);
/* the twiddle steps of the MDCT's FFT forms: step = one of these for the N-point form; the N/4-point form (quarter) has one
 * table for all four.  A table is `count` (cos, sin) pairs of the reference's angle of (step, k, length), in double or Q15 */
enum { LLZ_ROT_FWD_PRE = 0, LLZ_ROT_FWD_POST = 1, LLZ_ROT_INV_PRE = 2, LLZ_ROT_INV_POST = 3 };
double *llz_host_mdct_rot_f64(int quarter, int step, int count, int length);
short  *llz_host_mdct_rot_q15(int quarter, int step, int count, int length);
/* the cosine kernels of the defining sums: *fwd = [N/2][N], *inv = [N][N/2], in double or Q15; LLZ_OK or LLZ_ERR_NOMEM (what
 * was built stays in *fwd / *inv for the handle's destroy) */
int llz_host_mdct_sums_f64(int N, double **fwd, double **inv);
int llz_host_mdct_sums_q15(int N, short **fwd, short **inv);
/* the float pre-twiddles of the N/4-point form: cos and sin of -2 pi (k + 1/8) / N, k < N / 4 (llz_mdct.c:459-462) */
int llz_host_mdct_pretwiddles_f32(int N, float **tc, float **ts);

/* ---- llz_dft_host.c: the chirp tables of llz_dft_mc / llz_czt_mc (include/llz_dft.h has the algorithm) ----
 * m: the transform length of n points in, k bins out.  The tables of one direction into HOST memory, each built in double and
 * rounded to float once; a NULL table is skipped: pre [n] and post [k] complex with the window w (n floats, NULL: ones) folded
 * into the forward pre and the inverse post; v [m] complex, FFT_m of the wrapped chirp -- natural == 0: divided by m, entry e =
 * bin bitrev(e) (the fused kernel's); natural != 0: unscaled in natural order (the composed form's).  zoom == 0: the DFT
 * (k == n; f0, df unused; inverse 0 or 1), else the zoom transform (inverse == 0).  LLZ_OK or LLZ_ERR_NOMEM with a message. */
int llz_host_dft_m(int n, int k);
int llz_host_dft_tables(int n, int k, int zoom, double f0, double df, int inverse, int natural, const float *w, float *pre,
                        float *v, float *post);

/* ---- llz_spectra.c: the tables of the frequency-domain FIR forms ---- */

/* cs: 2 N doubles, cos then sin of 2 pi i / N, i < N, with exact quadrant values: the one table every FIR form's spectra and
 * twiddles come from */
void llz_host_cs_table(double *cs, int N);
/* z = DFT_N(z), N interleaved complex doubles, by radix-2 decimation in frequency in double, in place and left in that
 * transform's output order: entry e is bin bitrev_N(e); cs: llz_host_cs_table(cs, N) */
void llz_host_dif_f64(double *z, int N, const double *cs);

/* the real spectrum product of the 1024-point overlap-save (llz_fir_host.c): K = c / 32 for float taps that mirror bit for bit
 * about tap c = (flt_len - 1) / 2 = 32, 64, 96 or 128, else 0 (also under the ols_real_product = 0 tune); and the table it
 * takes, in double (the device table is its cast to float): dst[k] = Re DFT_1024(g)[k] / 1024, g[n] = taps[n + c] circularly,
 * natural order, cs: llz_host_cs_table(cs, 1024); *imag_max (may be NULL): the largest dropped |Im| / 1024 */
int  llz_host_ols_real_rows(const float *taps, int flt_len);
void llz_host_ols_real_table(double *dst, double *imag_max, const float *taps, int flt_len, const double *cs);

/* one tap row into the [P][N] complex floats of its partition spectra (LLZ_FIR_ALGO_PARTITIONED), P = ceil(flt_len / (N / 2)):
 * row p = DFT_N(taps[p N / 2 .. (p + 1) N / 2), zero-padded) / N, computed in double and rounded to float once, in the order of a
 * decimation-in-frequency transform's output (entry i = bin bitrev(i)); cs: llz_host_cs_table(cs, N); z: 2 N doubles of work
 * space */
void llz_host_part_spectra(float *dst, const float *taps, int flt_len, int N, const double *cs, double *z);

/* one tap row into the [P][block] complex floats of its partition spectra for the delay-line forms (llz_fir_stream_mc,
 * llz_fir_matrix_mc), P = ceil(flt_len / block): row p holds bins 0 .. block of the same transform, N = 2 block, scaled by
 * 1 / (2 N).  Entry i > 0 is bin bitrev(i) (over log2 block bits); entry 0 packs the two real bins: (DC, Nyquist).  cs:
 * llz_host_cs_table(cs, N); z: 2 N doubles of work space */
void llz_host_stream_spectra(float *dst, const float *taps, int flt_len, int block, const double *cs, double *z);
/* the way back (llz_adapt_mc_get_taps): the first `count` <= block samples of the real sequence whose packed row (layout and
 * 1 / (2 N) as above) is `row`, by an N-point transform in double, each rounded to float once; cs, z as above */
void llz_host_stream_taps(float *taps, int count, const float *row, int block, const double *cs, double *z);
/* the device table of both delay-line forms uploaded through llzs_h2d_table: [block / 2] complex W_block^m, then [block] complex
 * W_N^bitrev(i); d_tw: 2 (block / 2 + block) floats */
int  llz_host_stream_twiddles(float *d_tw, int block);

/* The spectra of `count` tap rows (taps: [count][flt_len]) built with N-point transforms -- llz_host_stream_spectra if packed,
 * else llz_host_part_spectra -- into d_dst = [count][row] floats, in chunks of whole rows of at most 8 MiB of host staging (one
 * row at least): at init through llzs_h2d_table, one table per chunk in row order, else (set_taps) through llzs_h2d on
 * `stream`, behind the calls already issued.  Out of host memory: LLZ_ERR_NOMEM and a message naming `who`. */
int llz_host_load_spectra(const char *who, float *d_dst, size_t row, int count, const float *taps, int flt_len, int N, int packed,
                          int at_init, void *stream);

/* The input groups of the matrix product (llzs_fir_matrix_mac_f32) for llz_fir_matrix_mc and llz_adapt_matrix_mc, which
 * promises the former's summation order: G and the inputs per group from (inputs, outputs, block) alone -- as many groups as
 * bring the product to LLZ_MATRIX_WG_TARGET workgroups per block, LLZ_MATRIX_MAX_GROUPS at the most, of equal size but for a
 * ragged last one */
#define LLZ_MATRIX_WG_TARGET 1024               /* workgroups of the product asked for before the sum over inputs stays whole */
#define LLZ_MATRIX_MAX_GROUPS 32
static inline void llz_host_matrix_groups(int inputs, int outputs, int block, int *G, int *gsize)
{
    const long rows = (long)outputs * (block >= 1024 ? block / 512 : 1);        /* workgroups of one group: outputs x bin tiles */
    long cap = (LLZ_MATRIX_WG_TARGET + rows - 1) / rows;
    if (cap > LLZ_MATRIX_MAX_GROUPS) cap = LLZ_MATRIX_MAX_GROUPS;
    if (cap > inputs) cap = inputs;
    *gsize = (int)((inputs + cap - 1) / cap);
    *G = (inputs + *gsize - 1) / *gsize;
}

/* a malloc'ed float copy of `count` double taps; NULL, with a message naming `who`, when out of host memory */
float *llz_host_taps_f32(const char *who, const double *taps, size_t count);

/* Caller buffers: llzs_is_device_ptr(p) is 1 for device memory of the CURRENT device (used in place), 0 for host memory
 * (staged through the GPU) and LLZ_ERR_ARG, with a message, for device memory that lives on another device -- a handle
 * binds its device before it looks at the caller's pointers, so a buffer of the wrong GPU is refused instead of faulting. */

/* 1 when the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share at least one byte (an empty range shares none) */
int llz_ranges_intersect(const void *a, size_t a_bytes, const void *b, size_t b_bytes);
/* The out-of-place batch entry points call this before they stage or launch anything: LLZ_ERR_ARG, with the message
 * "<who>: <out_name> may not overlap <in_name> (device memory)", when both buffers are device memory (in_dev / out_dev as
 * llzs_is_device_ptr() answered) and their ranges intersect -- a kernel reads and writes such a pair in no defined order;
 * LLZ_OK otherwise.  Host buffers are staged through the library's own device memory, so they are never refused here. */
int llz_refuse_device_overlap(const char *who, const char *in_name, const void *in, size_t in_bytes, int in_dev,
                              const char *out_name, const void *out, size_t out_bytes, int out_dev);

/* The register transforms (fft.hip: llz_fft_batch, llz_fft_fixed_batch, llz_mdct_batch, llz_mdct_frames_mc_*) move 8 or 16
 * bytes per lane and take their rows on a 16-byte boundary; the headers ask no more of a caller's pointer than its element's
 * alignment.  llz_in_place() is 1 for device memory (dev as llzs_is_device_ptr() answered) such a kernel may use where it
 * lies; everything else -- host memory, and device memory at a lesser alignment -- goes through the handle's staging buffer
 * with the llz_vec_stage_* calls below (a copy from / to host memory waits for the stream, one between device buffers is
 * ordered on it). */
enum { LLZ_VEC_ALIGN = 16 };
int llz_in_place(const void *p, int dev);

/* staging buffers for callers that hand over host memory */
typedef struct {
    void *dev;
    size_t bytes;
} llz_stage_t;

/* grow-only device scratch; returns NULL on failure */
void *llz_stage_reserve(llz_stage_t *s, size_t bytes);
void  llz_stage_release(llz_stage_t *s);

/* The staged call of the out-of-place batch entry points, once the caller's pointers are classified (user_dev as
 * llzs_is_device_ptr() answered, 0 or 1) and overlap is refused: where a kernel reads its input and writes its output.  Device
 * memory is used where it lies; for host memory llz_stage_in reserves `bytes` of s and copies the input there on `stream`,
 * llz_stage_out only reserves, and the call ends with llzs_d2h from the stage.  Both chain on *rc: with *rc != LLZ_OK on entry
 * they do nothing (a failed upload skips the output's reserve), and they set it to LLZ_ERR_NOMEM when the reserve fails or to
 * the copy's error. */
const void *llz_stage_in(llz_stage_t *s, const void *user, size_t bytes, int user_dev, void *stream, int *rc);
void *llz_stage_out(llz_stage_t *s, void *user, size_t bytes, int user_dev, int *rc);

/* The same three steps under the 16-byte rule above: memory that llz_in_place() accepts is used where it lies, everything else
 * goes through s with a copy from host or device memory (llz_vec_stage_in), is reserved (llz_vec_stage_out), and is copied back
 * when d, the pointer the kernel wrote, is not the caller's (llz_vec_stage_back).  All three chain on *rc. */
const void *llz_vec_stage_in(llz_stage_t *s, const void *user, size_t bytes, int user_dev, void *stream, int *rc);
void *llz_vec_stage_out(llz_stage_t *s, void *user, size_t bytes, int user_dev, int *rc);
void  llz_vec_stage_back(void *user, const void *d, size_t bytes, int user_dev, void *stream, int *rc);

/* The staged call of the one-shot entry points, which have no handle to keep a stage in.  A call declares its buffers in the
 * order its kernel takes them: name, pointer, bytes, input or output (a NULL pointer or no bytes: an optional buffer that is
 * absent; LLZ_BIND_SCRATCH: the library's own, filled in by llz_bind_scratch).  llz_bind classifies them all (memory of another
 * GPU: LLZ_ERR_ARG), refuses a device overlap of each input with each output through llz_refuse_device_overlap before anything
 * is staged, then, in declaration order, uploads host inputs (an input whose pointer is an earlier input's shares its copy) and
 * reserves host outputs; dev is what to launch with.  llz_bind_finish(rc of the launch) downloads the staged outputs in
 * declaration order, synchronises the stream once if anything was staged, frees, and returns the first error. */
enum { LLZ_BIND_IN = 0, LLZ_BIND_OUT = 1, LLZ_BIND_SCRATCH = 2 };
typedef struct {
    const char *name;
    const void *user;
    size_t bytes;
    int kind;
    void *dev;                  /* filled in by llz_bind */
    int on_dev, staged;
} llz_bind_t;
int   llz_bind(const char *who, llz_bind_t *b, int count, void *stream);
void *llz_bind_scratch(llz_bind_t *b, size_t bytes, int *rc);     /* chains on *rc; freed by llz_bind_finish */
int   llz_bind_finish(llz_bind_t *b, int count, void *stream, int rc);

/* ---- llz_adapt_core.c: what the adaptive handles share (llz_adapt_mc, llz_adapt_matrix_mc) ---- */

/* the refusals of an init behind its channel or port counts, with a message naming `who`, 1 when refused: block (a power of two
 * in 64..2048; 4096 has a message of its own), frame_len = k x block with k >= 1 (max_blocks != 0: k in 1..max_blocks), flt_len,
 * mu in 0..2, delta finite and above 0 */
int  llz_adapt_refuse(const char *who, int block, int frame_len, int max_blocks, int flt_len, float mu, float delta);
/* its last two on their own, for the per-band filters: "<who>: mu <mu> outside 0..2" and "<who>: delta <delta> is not a finite
 * value above 0" */
int  llz_adapt_refuse_mu(const char *who, float mu);
int  llz_adapt_refuse_delta(const char *who, float delta);

/* the step sizes of `count` rows (channels, outputs): the device array the kernels read and its host copy, which tells a call
 * whether anything adapts */
typedef struct {
    float *h_mu, *d_mu;         /* HOST and device [count] */
    int count, adapting;        /* rows whose mu is not zero */
} llz_adapt_steps_t;
/* every row at mu.  Out of host memory: LLZ_ERR_NOMEM and a message.  Out of device memory: d_mu stays NULL and the answer is
 * LLZ_OK, for the init's own message about its small device buffers */
int  llz_adapt_steps_create(llz_adapt_steps_t *s, const char *who, int count, float mu);
void llz_adapt_steps_destroy(llz_adapt_steps_t *s);
/* rows [first, first + count) (inside the state: the caller checks) to mu[], uploaded on the stream; a mu outside 0..2 is
 * refused with "<who>: mu <mu> of <noun> <row> outside 0..2" */
int  llz_adapt_steps_set(llz_adapt_steps_t *s, const char *who, const char *noun, int first, int count, const float *mu,
                         void *stream);

/* get_taps: the flt_len taps of each of `count` neighbouring weight rows at d_w ([P][block] packed spectra each, as
 * llz_host_load_spectra built them) into taps = [count][flt_len], through at most 8 MiB of host staging (one row at least) */
int  llz_adapt_get_taps(const char *who, float *taps, const float *d_w, int count, int block, int flt_len, void *stream);

/* the staged call: x of xbytes, d, e and y (may be NULL) of `bytes` each.  begin refuses in-place use and device overlap of an
 * input with an output or of e with y, then x, d, e, y are where the launches read and write (the caller's device memory, or the
 * stages); end(rc of the launches) copies e and y back to host memory and returns the first error */
typedef struct {
    llz_stage_t st_x, st_d, st_e, st_y;
    const float *x, *d;
    float *e, *y;
    float *user_e, *user_y;     /* host memory to copy back to, or NULL */
    size_t bytes;
} llz_adapt_io_t;
int  llz_adapt_io_begin(llz_adapt_io_t *io, const char *who, const float *x, size_t xbytes, const float *d, float *e, float *y,
                        size_t bytes, void *stream);
int  llz_adapt_io_end(llz_adapt_io_t *io, int rc, void *stream);
void llz_adapt_io_release(llz_adapt_io_t *io);

/* ---- llz_bands_core.c: what the per-band handles share (llz_adapt_bands_mc, llz_adapt_bands_matrix_mc, llz_kalman_bands_mc,
 * llz_kalman_bands_matrix_mc, llz_suppress_bands_mc) ---- */

#define LLZ_BANDS_MAX_BINS 4097
#define LLZ_BANDS_MAX_CHANNELS 65535
enum { LLZ_BANDS_MAX_BUFS = 8 };

/* an init's refusal of a count: 1 and "<who>: <name> <value> outside <lowest>..<highest>" */
int  llz_bands_refuse_count(const char *who, const char *name, int value, int lowest, int highest);
/* a call's refusals behind its handle, 1 when refused: frames negative or frames x bins not below 2^31; half a y */
int  llz_bands_refuse_call(const char *who, int frames, int bins, const float *yre, const float *yim);

/* One caller buffer of a call, in the order the kernel takes them, the inputs first.  user NULL: an optional buffer that is
 * absent -- it is not classified, refused, staged or counted. */
typedef struct {
    const char *name;
    const void *user;
    size_t bytes;
    int optional;
} llz_bands_buf_t;
/* x, d, e and an optional y, re and im apart, of xb and db bytes: the table of the three adaptive calls, from their parameters */
#define LLZ_BANDS_XDEY(xb, db)                                                                                             \
    { { "xre", xre, xb, 0 }, { "xim", xim, xb, 0 }, { "dre", dre, db, 0 }, { "dim", dim, db, 0 },                          \
      { "ere", ere, db, 0 }, { "eim", eim, db, 0 }, { "yre", yre, db, 1 }, { "yim", yim, db, 1 } }
typedef struct {
    llz_stage_t st[LLZ_BANDS_MAX_BUFS];
    void *dev[LLZ_BANDS_MAX_BUFS];      /* what to launch with: the caller's device memory or the stage; NULL when absent */
    void *back[LLZ_BANDS_MAX_BUFS];     /* host memory an output is copied back to, or NULL */
    size_t bytes[LLZ_BANDS_MAX_BUFS];
    int count, inputs, entered, prev;
} llz_bands_io_t;
/* what every per-band handle starts with */
typedef struct {
    llz_head_t head;
    long long frames;                   /* frames since init or reset */
    llz_bands_io_t io;
} llz_bands_t;
/* The staged call.  begin: a missing buffer that is not optional is refused ("<who>: NULL buffer"); then the handle's device is
 * entered, the buffers are classified, every output is refused against every buffer in front of it (llz_refuse_device_overlap),
 * and only then inputs are staged and uploaded and outputs reserved, in the table's order; out of device memory the message
 * names the buffers and their bytes (split != 0: b[0]'s as x's and b[split]'s).  io.dev is what to launch with.  end(rc of the
 * launch) counts the frames of a launch that was issued, copies the host outputs back, leaves the device and returns frames or
 * the first error; it is called whatever begin returned. */
int  llz_bands_begin(llz_bands_t *f, const char *who, const llz_bands_buf_t *b, int count, int inputs, int split);
int  llz_bands_end(llz_bands_t *f, int rc, int frames);
void llz_bands_release(llz_bands_t *f);

/* the handle, or NULL with "<who>: bad handle" or, out being NULL, "<who>: no out": the head of plan and frames */
void *llz_bands_out(unsigned long h, int tag, const char *who, const void *out);
int  llz_bands_frames(unsigned long h, int tag, const char *who, long long *out);
/* the refusals of a set_* or get_* call behind its handle, 1 when refused: a or b NULL; rows [first, first + count) outside
 * [0, have), with the rows' noun ("channels", "outputs", "inputs") */
int  llz_bands_refuse_range(const char *who, const char *noun, int first, int count, int have, const void *a, const void *b);
/* rows [first, first + count) of a state array of row_bytes per row, up from src (not NULL) or down to dst, on the handle's
 * device and ordered on its stream; _pair: the re and im arrays of `row` floats per row, one after the other */
int  llz_bands_copy(const llz_bands_t *f, void *d_state, size_t row_bytes, int first, int count, const void *src, void *dst);
int  llz_bands_copy_pair(const llz_bands_t *f, float *const d_state[2], size_t row, int first, int count, const float *src_re,
                         const float *src_im, float *dst_re, float *dst_im);
/* zeros in `count` floats of a re and an im array, on the stream */
int  llz_bands_zero_pair(float *const d[2], size_t count, void *stream);
/* flags [first, first + count) of a device array of ints to on[] != 0 (on NULL: all 1), through llz_bands_copy; out of host
 * memory "<who>: no host memory for <bytes> B of <what>" */
int  llz_bands_flags(const llz_bands_t *f, const char *who, const char *what, int *d_flags, int first, int count, const int *on);

/* ---- llz_fade.c: the crossfade state of the delay-line convolvers (llz_fir_xfade_stream_mc, llz_fir_xfade_matrix_mc) ---- */

#define LLZ_FADE_MAX_BLOCKS 4096        /* fade_blocks x block <= 2^24: a sample's index within the fade is exact in float */

/* A fade over `rows` rows of spectra of `row` floats each (the stream handle's tap rows, the matrix handle's paths in
 * [outputs][inputs] order): the same rows and row go with every call below.  Zeroed = a handle that has never faded. */
typedef struct {
    float *d_new;               /* the handle's spectra buffer's size and layout: the spectra the rows in the fade go to */
    unsigned char *h_rows;      /* HOST [rows]: 1 = the row is in the fade */
    unsigned char *d_rows;      /* its device copy, updated on the handle's stream: the fade kernels' table */
    int blocks, done;           /* the fade's length (0: none pending or in flight) and the blocks of it already launched */
} llz_fade_t;

/* the refusals of a fade request, with a message naming `who`: fade_blocks outside 1..LLZ_FADE_MAX_BLOCKS, and one fade at a
 * time -- until its first block has run, requests with the same fade_blocks add or replace rows (`noun`: "rows", "paths") */
int  llz_fade_refuse(const llz_fade_t *fd, const char *who, const char *noun, int fade_blocks);
/* set_taps while a fade is pending or in flight: refused with the blocks left */
int  llz_fade_refuse_set_taps(const llz_fade_t *fd, const char *who);
/* the handle's first fade: d_new and the two tables, kept until the release; LLZ_ERR_NOMEM with a message naming who and the bytes */
int  llz_fade_reserve(llz_fade_t *fd, const char *who, const char *noun, size_t rows, size_t row);
/* `table` (h_rows with the request's rows set) goes up on the stream, behind the last launch that read d_rows; the host copy,
 * blocks = fade_blocks and done = 0 are taken only when the upload succeeded */
int  llz_fade_commit(llz_fade_t *fd, const unsigned char *table, size_t rows, int fade_blocks, void *stream);
/* the fade is over (its last block launched, a reset, a flush): the new rows become the handle's, on the stream behind the
 * launches already issued -- *d_h and d_new swapped when every row faded, else each run of faded rows copied into *d_h; the
 * table is cleared and blocks = done = 0 */
int  llz_fade_adopt(llz_fade_t *fd, float **d_h, size_t rows, size_t row, void *stream);
/* blocks of the fade still to be launched; 0: none pending or in flight */
int  llz_fade_left(const llz_fade_t *fd);
void llz_fade_release(llz_fade_t *fd);

#endif
