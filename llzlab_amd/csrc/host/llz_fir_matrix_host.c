/* llz_fir_matrix_host.c -- include/llz_fir.h part 6: llz_fir_matrix_mc, the many-in, many-out stream convolver y_o = sum_i x_i *
 * h_{o,i} (kernels K4g, fir_matrix.hip).  llz_fir_stream_mc's scheme (llz_fir_stream_host.c) with a delay line per INPUT, tap
 * spectra per path (o, i) and three launches per call: forward transforms, the product summed over inputs in G groups, inverse
 * transforms.  The tap spectra and the twiddles come from the builders the stream convolver uses (llz_spectra.c), so one
 * path of the matrix is a stream channel.  Staging, pointer classification and error conventions are those of llz_fir_host.c.
 *
 * llz_fir_xfade_matrix_mc fades paths to new taps over fade_blocks blocks.  The fade's state and rules are llz_fade.c's, with
 * the paths in [outputs][inputs] order as its rows (the second spectra buffer, the table of fading paths, the refusals, the
 * adoption); what is the handle's own is here: the second scratch of partial spectra, the tables of the outputs that fade and of
 * the new taps' connections (taken by the handle only when all tables are up), and the connection table's update at adoption.
 * While the fade is pending or in flight the product and the inverse of every call go to fir_matrix_fade.hip with the fade's
 * position by value; after the launches of a call or of a whole flush the handle moves the fade on by the blocks launched and
 * adopts at its end, so that the next call runs the three untouched kernels.  A handle that never fades allocates and launches
 * nothing of this. */
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"

#define FIRX_MIN_BLOCK 64
#define FIRX_MAX_BLOCK 4096
#define FIRX_MAX_PORTS 4096                     /* inputs, outputs */
#define FIRX_MAX_BLOCKS 65535                   /* blocks of a launch: a grid dimension */
#define FIRX_SCRATCH_BYTES ((size_t)64 << 20)   /* the partial spectra of a flush beyond this go in several passes */

typedef struct {
    int tag;                    /* LLZ_TAG_FIRX */
    int device;
    int inputs, outputs, block, frame_len, flt_len;
    int k, P, R;                /* blocks per call, partitions, ring slots = P + k - 1 */
    int head;                   /* the ring slot the next block writes: kept here, passed by value with each launch */
    int cur;                    /* d_prev[cur] holds the last input block; a call writes the other and swaps */
    int G, gsize;               /* input groups of the product, inputs per group */
    int ycap;                   /* blocks the partial-spectra scratch holds */
    int connected;              /* paths with a non-zero tap */
    unsigned char *conn;        /* HOST [outputs][inputs]: 1 = connected */
    unsigned char *d_conn;      /* its device copy, updated on the handle's stream */
    float *d_h;                 /* [outputs][inputs][P][block] complex: the partition spectra (llz_host_stream_spectra) */
    float *d_tw;                /* [block / 2] complex W_block^m, then [block] complex W_N^bitrev(i) */
    float *d_ring;              /* [inputs][R][block] complex: spectra of the last R blocks of every input */
    float *d_prev[2];           /* [inputs][block]: the last input block, double-buffered */
    float *d_y;                 /* [G][outputs][ycap][block] complex: the groups' partial spectra */
    /* the fade (llz_fir_xfade_matrix_mc): everything below is allocated at the first fade and kept */
    llz_fade_t fade;            /* over the paths of d_h in [outputs][inputs] order (llz_fade.c) */
    float *d_yn;                /* d_y's size: the new taps' partial spectra of a blending block */
    unsigned char *h_ofade;     /* HOST [outputs]: 1 = the output has a path in the fade */
    unsigned char *conn_new;    /* HOST [outputs][inputs]: connected under the new taps (only the fade's paths are read) */
    unsigned char *d_ofade, *d_conn_new;    /* their device copies, updated on the handle's stream */
    void *stream;
    llz_stage_t st_in, st_out;  /* only for callers passing host memory */
} firx_t;

static void firx_destroy(firx_t *f)
{
    if (!f) return;
    llzs_free(f->d_h); llzs_free(f->d_tw); llzs_free(f->d_ring); llzs_free(f->d_prev[0]); llzs_free(f->d_prev[1]);
    llzs_free(f->d_y); llzs_free(f->d_conn);
    llz_fade_release(&f->fade);
    llzs_free(f->d_yn); llzs_free(f->d_ofade); llzs_free(f->d_conn_new);
    free(f->h_ofade); free(f->conn_new);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    free(f->conn);
    f->tag = 0;
    free(f);
}

static int firx_row_connected(const float *taps, int flt_len)
{
    for (int t = 0; t < flt_len; t++)
        if (taps[t] != 0.0f) return 1;
    return 0;
}

/* the spectra of the paths (o, in_first .. in_first + in_count) (taps: [in_count][flt_len]) built and uploaded, and the paths'
 * entries of the connection table: at init as tables, from set_taps on the handle's stream behind the calls already issued */
static int firx_load_paths(firx_t *f, int o, int in_first, int in_count, const float *taps, int at_init)
{
    const size_t row = 2 * (size_t)f->P * (size_t)f->block;         /* floats of one path's spectra */
    const size_t first = (size_t)o * (size_t)f->inputs + (size_t)in_first;
    const int rc = llz_host_load_spectra("llz_fir_matrix_mc", f->d_h + first * row, row, in_count, taps, f->flt_len, 2 * f->block, 1,
                                         at_init, f->stream);
    if (rc != LLZ_OK) return rc;
    for (int i = 0; i < in_count; i++) {
        const unsigned char now = (unsigned char)firx_row_connected(taps + (size_t)i * (size_t)f->flt_len, f->flt_len);
        f->connected += (int)now - (int)f->conn[first + (size_t)i];
        f->conn[first + (size_t)i] = now;
    }
    /* at init the whole table goes up once, behind the last row */
    return at_init ? LLZ_OK : llzs_h2d(f->d_conn + first, f->conn + first, (size_t)in_count, f->stream);
}

/* the refusals of both inits, each with a message of its own that names `who` and the range */
static int firx_refuse(const char *who, int inputs, int outputs, int block, int frame_len, const void *taps, int flt_len)
{
    if (inputs < 1 || inputs > FIRX_MAX_PORTS) {
        llzs_set_error("%s: inputs %d outside 1..%d", who, inputs, FIRX_MAX_PORTS);
        return 1;
    }
    if (outputs < 1 || outputs > FIRX_MAX_PORTS) {
        llzs_set_error("%s: outputs %d outside 1..%d", who, outputs, FIRX_MAX_PORTS);
        return 1;
    }
    if (block < FIRX_MIN_BLOCK || block > FIRX_MAX_BLOCK || (block & (block - 1))) {
        llzs_set_error("%s: block %d is not a power of two in %d..%d", who, block, FIRX_MIN_BLOCK, FIRX_MAX_BLOCK);
        return 1;
    }
    if (frame_len < block || frame_len % block || frame_len / block > FIRX_MAX_BLOCKS) {
        llzs_set_error("%s: frame_len %d is not k x block with k in 1..%d (block %d)", who, frame_len, FIRX_MAX_BLOCKS, block);
        return 1;
    }
    if (flt_len < 1 || flt_len > LLZS_FIR_PART_MAX_TAPS) {
        llzs_set_error("%s: flt_len %d outside 1..%d", who, flt_len, LLZS_FIR_PART_MAX_TAPS);
        return 1;
    }
    if (!taps) {
        llzs_set_error("%s: no taps", who);
        return 1;
    }
    return 0;
}

/* zeros in the delay lines (rings and last blocks), ordered on the handle's stream */
static int firx_clear(firx_t *f)
{
    const size_t pbytes = sizeof(float) * (size_t)f->inputs * (size_t)f->block;
    int rc = llzs_memset(f->d_ring, 0, sizeof(float) * 2 * (size_t)f->inputs * (size_t)f->R * (size_t)f->block, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev[0], 0, pbytes, f->stream);
    if (rc == LLZ_OK) rc = llzs_memset(f->d_prev[1], 0, pbytes, f->stream);
    f->head = 0;
    f->cur = 0;
    return rc;
}

unsigned long llz_fir_matrix_mc_init(int inputs, int outputs, int block, int frame_len, const float *taps, int flt_len)
{
    const char *who = "llz_fir_matrix_mc_init";
    if (firx_refuse(who, inputs, outputs, block, frame_len, taps, flt_len)) return LLZ_BAD_HANDLE;
    firx_t *f = (firx_t *)calloc(1, sizeof(*f));
    if (!f) return LLZ_BAD_HANDLE;
    f->tag = LLZ_TAG_FIRX;
    f->device = llzs_device_get();
    f->inputs = inputs; f->outputs = outputs; f->block = block; f->frame_len = frame_len; f->flt_len = flt_len;
    f->k = frame_len / block;
    f->P = (flt_len + block - 1) / block;
    f->R = f->P + f->k - 1;
    llz_host_matrix_groups(inputs, outputs, block, &f->G, &f->gsize);
    const size_t paths = (size_t)outputs * (size_t)inputs;
    const size_t ybytes1 = sizeof(float) * 2 * (size_t)f->G * (size_t)outputs * (size_t)block;     /* one block's partials */
    const int nflush = (flt_len - 1 + block - 1) / block;
    size_t ycap = FIRX_SCRATCH_BYTES / ybytes1;
    if (ycap > (size_t)nflush) ycap = (size_t)nflush;
    if (ycap < (size_t)f->k) ycap = (size_t)f->k;
    if (ycap > FIRX_MAX_BLOCKS) ycap = FIRX_MAX_BLOCKS;
    f->ycap = (int)ycap;
    const size_t hbytes = sizeof(float) * 2 * paths * (size_t)f->P * (size_t)block;
    const size_t rbytes = sizeof(float) * 2 * (size_t)inputs * (size_t)f->R * (size_t)block;
    const size_t ybytes = ybytes1 * ycap;
    const size_t twbytes = sizeof(float) * 2 * ((size_t)block / 2 + (size_t)block);
    const size_t pbytes = sizeof(float) * (size_t)inputs * (size_t)block;
    int rc = LLZ_OK;
    f->conn = (unsigned char *)calloc(paths, 1);
    if (!f->conn) {
        llzs_set_error("%s: no host memory for the connection table: %zu B asked for", who, paths);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_h = (float *)llzs_malloc(hbytes))) {
        llzs_set_error("%s: no device memory for the partition spectra: %zu B asked for (%d outputs x %d inputs x %d partitions x "
                       "%d bins)", who, hbytes, outputs, inputs, f->P, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_ring = (float *)llzs_malloc(rbytes))) {
        llzs_set_error("%s: no device memory for the delay lines: %zu B asked for (%d inputs x %d slots x %d bins)", who, rbytes,
                       inputs, f->R, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK && !(f->d_y = (float *)llzs_malloc(ybytes))) {
        llzs_set_error("%s: no device memory for the partial spectra: %zu B asked for (%d groups x %d outputs x %d blocks x %d "
                       "bins)", who, ybytes, f->G, outputs, f->ycap, block);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) {
        f->d_tw = (float *)llzs_malloc(twbytes);
        f->d_prev[0] = (float *)llzs_malloc(pbytes);
        f->d_prev[1] = (float *)llzs_malloc(pbytes);
        f->d_conn = (unsigned char *)llzs_malloc(paths);
        if (!f->d_tw || !f->d_prev[0] || !f->d_prev[1] || !f->d_conn) {
            llzs_set_error("%s: no device memory for the twiddles, the last input blocks and the connection table: %zu B, 2 x %zu B "
                           "and %zu B asked for", who, twbytes, pbytes, paths);
            rc = LLZ_ERR_NOMEM;
        }
    }
    /* tables through llzs_h2d_table, in a fixed order */
    for (int o = 0; o < outputs && rc == LLZ_OK; o++)
        rc = firx_load_paths(f, o, 0, inputs, taps + (size_t)o * (size_t)inputs * (size_t)flt_len, 1);
    if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_conn, f->conn, paths);
    if (rc == LLZ_OK) rc = llz_host_stream_twiddles(f->d_tw, block);
    if (rc == LLZ_OK) rc = firx_clear(f);
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    if (rc != LLZ_OK) {
        firx_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

unsigned long llz_fir_matrix_mc_init_f64taps(int inputs, int outputs, int block, int frame_len, const double *taps, int flt_len)
{
    const char *who = "llz_fir_matrix_mc_init_f64taps";
    if (firx_refuse(who, inputs, outputs, block, frame_len, taps, flt_len)) return LLZ_BAD_HANDLE;
    float *t = llz_host_taps_f32(who, taps, (size_t)outputs * (size_t)inputs * (size_t)flt_len);
    if (!t) return LLZ_BAD_HANDLE;
    unsigned long h = llz_fir_matrix_mc_init(inputs, outputs, block, frame_len, t, flt_len);
    free(t);
    return h;
}

void llz_fir_matrix_mc_uninit(unsigned long handle)
{
    if (LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX)) {
        firx_t *f = (firx_t *)handle;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        firx_destroy(f);
        llzs_device_leave(prev);
    }
}

/* the fade is over (its last block launched, a reset, a flush): the new paths become the handle's and the connection table
 * follows the new taps, on the stream behind the launches already issued */
static int firx_adopt(firx_t *f)
{
    const size_t paths = (size_t)f->outputs * (size_t)f->inputs;
    f->connected = 0;
    for (size_t q = 0; q < paths; q++) {
        if (f->fade.h_rows[q]) f->conn[q] = f->conn_new[q];
        f->connected += f->conn[q];
    }
    int rc = llz_fade_adopt(&f->fade, &f->d_h, paths, 2 * (size_t)f->P * (size_t)f->block, f->stream);
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_conn, f->conn, paths, f->stream);
    memset(f->h_ofade, 0, (size_t)f->outputs);
    return rc;
}

/* the product and the inverse of nblk blocks whose ring slots start at `head`: the fading pair exactly while a fade is pending
 * or in flight.  flush: the launch's block 0 is block j0 of the flush.  The caller moves the fade on */
static int firx_launch(firx_t *f, float *d_out, int nblk, int flush, int j0, int head, long n_out, long out_pitch)
{
    int rc;
    if (!f->fade.blocks) {
        rc = llzs_fir_matrix_mac_f32(f->block, f->d_h, f->d_ring, f->d_conn, f->d_y, f->inputs, f->outputs, nblk, flush, j0, f->P,
                                     f->R, head, f->G, f->gsize, f->stream);
        if (rc == LLZ_OK)
            rc = llzs_fir_matrix_inv_f32(f->block, f->d_y, f->d_tw, d_out, f->outputs, nblk, f->G, n_out, out_pitch, f->stream);
        return rc;
    }
    rc = llzs_fir_matrix_mac_fade_f32(f->block, f->d_h, f->fade.d_new, f->d_ring, f->d_conn, f->d_conn_new, f->fade.d_rows,
                                      f->d_ofade, f->d_y, f->d_yn, f->inputs, f->outputs, nblk, flush, j0, f->P, f->R, head, f->G,
                                      f->gsize, f->fade.done, f->fade.blocks, f->stream);
    if (rc == LLZ_OK)
        rc = llzs_fir_matrix_inv_fade_f32(f->block, f->d_y, f->d_yn, f->d_ofade, f->d_tw, d_out, f->outputs, nblk, j0, f->G, n_out,
                                          out_pitch, f->fade.done, f->fade.blocks, f->stream);
    return rc;
}

static int firx_process(firx_t *f, const float *in, float *out, int frame_len)
{
    if (frame_len != f->frame_len) {
        llzs_set_error("llz_fir_matrix_mc: frame_len %d != init frame_len %d", frame_len, f->frame_len);
        return LLZ_ERR_ARG;
    }
    if ((const float *)out == in) {
        llzs_set_error("llz_fir_matrix_mc: in-place filtering is not supported");
        return LLZ_ERR_ARG;
    }
    const size_t ibytes = sizeof(float) * (size_t)f->inputs * (size_t)frame_len;
    const size_t obytes = sizeof(float) * (size_t)f->outputs * (size_t)frame_len;
    const int in_dev = llzs_is_device_ptr(in), out_dev = llzs_is_device_ptr(out);
    if (in_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;            /* a buffer of another GPU: refused, message set */
    if (llz_refuse_device_overlap("llz_fir_matrix_mc", "in", in, ibytes, in_dev, "out", out, obytes, out_dev)) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = llz_stage_in(&f->st_in, in, ibytes, in_dev, f->stream, &rc);
    float *d_out = llz_stage_out(&f->st_out, out, obytes, out_dev, &rc);
    if (rc == LLZ_OK)
        rc = llzs_fir_matrix_fwd_f32(f->block, f->d_tw, f->d_ring, f->d_prev[f->cur], f->d_prev[f->cur ^ 1], d_in, f->inputs, f->k,
                                     0, frame_len, f->R, f->head, f->stream);
    if (rc == LLZ_OK) {
        /* the delay lines have moved on, whatever becomes of the rest of the call */
        const int head = f->head;
        f->head = (f->head + f->k) % f->R;
        f->cur ^= 1;
        rc = firx_launch(f, d_out, f->k, 0, 0, head, frame_len, frame_len);
        if (rc == LLZ_OK && f->fade.blocks) {
            f->fade.done += f->k;
            if (f->fade.done >= f->fade.blocks) rc = firx_adopt(f);
        }
    }
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, obytes, f->stream);
    return rc == LLZ_OK ? frame_len : rc;
}

int llz_fir_matrix_mc(unsigned long handle, const float *in, float *out, int frame_len)
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX) || !in || !out) {
        llzs_set_error("llz_fir_matrix_mc: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firx_t *f = (firx_t *)handle;
    const int prev = llzs_device_enter(f->device);       /* the handle's device, whatever the caller has current */
    const int rc = firx_process(f, in, out, frame_len);
    llzs_device_leave(prev);
    return rc;
}

static int firx_flush(firx_t *f, float *out)
{
    const int keep = f->flt_len - 1, B = f->block;
    if (keep == 0) {                                              /* nothing to emit; the handle still starts over */
        int rc0 = f->fade.blocks ? firx_adopt(f) : LLZ_OK;
        if (rc0 == LLZ_OK) rc0 = firx_clear(f);
        return rc0 == LLZ_OK ? 0 : rc0;
    }
    const size_t bytes = sizeof(float) * (size_t)f->outputs * (size_t)keep;
    const int out_dev = llzs_is_device_ptr(out);
    if (out_dev < 0) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    float *d_out = llz_stage_out(&f->st_out, out, bytes, out_dev, &rc);
    if (rc != LLZ_OK) return rc;
    /* behind the input only the spectrum of (last block, zeros) is new: it goes into slot `head`, which the reset below gives
     * up anyway; then the ceil(keep / block) zero blocks side by side, as many at a time as the scratch holds.  A fade pending
     * or in flight goes on through them -- flush block j is fade block done + j, whichever pass it falls in -- and the
     * handle starts over on the new taps */
    const int nblk = (keep + B - 1) / B;
    rc = llzs_fir_matrix_fwd_f32(B, f->d_tw, f->d_ring, f->d_prev[f->cur], NULL, NULL, f->inputs, 1, 1, 0, f->R, f->head, f->stream);
    for (int j0 = 0; j0 < nblk && rc == LLZ_OK; j0 += f->ycap) {
        const int nb = nblk - j0 < f->ycap ? nblk - j0 : f->ycap;
        const long left = (long)keep - (long)j0 * B, n_out = left < (long)nb * B ? left : (long)nb * B;
        rc = firx_launch(f, d_out + (size_t)j0 * (size_t)B, nb, 1, j0, f->head, n_out, keep);
    }
    if (rc == LLZ_OK && f->fade.blocks) rc = firx_adopt(f);
    if (rc == LLZ_OK) rc = firx_clear(f);
    if (rc == LLZ_OK && !out_dev) rc = llzs_d2h(out, d_out, bytes, f->stream);
    return rc == LLZ_OK ? keep : rc;
}

int llz_fir_matrix_mc_flush(unsigned long handle, float *out)
{
    /* one tap: nothing to emit, so out may be NULL */
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX) || (!out && ((firx_t *)handle)->flt_len > 1)) {
        llzs_set_error("llz_fir_matrix_mc_flush: bad handle or NULL buffer");
        return LLZ_ERR_ARG;
    }
    firx_t *f = (firx_t *)handle;
    const int prev = llzs_device_enter(f->device);
    const int rc = firx_flush(f, out);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_matrix_mc_reset(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX)) {
        llzs_set_error("llz_fir_matrix_mc_reset: bad handle");
        return LLZ_ERR_ARG;
    }
    firx_t *f = (firx_t *)handle;
    const int prev = llzs_device_enter(f->device);
    int rc = f->fade.blocks ? firx_adopt(f) : LLZ_OK;             /* a fade pending or in flight: the new taps at once */
    if (rc == LLZ_OK) rc = firx_clear(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_matrix_mc_set_taps(unsigned long handle, int out_first, int out_count, int in_first, int in_count, const float *taps)
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX) || !taps) {
        llzs_set_error("llz_fir_matrix_mc_set_taps: bad handle or NULL taps");
        return LLZ_ERR_ARG;
    }
    firx_t *f = (firx_t *)handle;
    if (out_first < 0 || out_count < 1 || out_first >= f->outputs || out_count > f->outputs - out_first) {
        llzs_set_error("llz_fir_matrix_mc_set_taps: outputs [%d, %d + %d) outside the handle's [0, %d)", out_first, out_first,
                       out_count, f->outputs);
        return LLZ_ERR_ARG;
    }
    if (in_first < 0 || in_count < 1 || in_first >= f->inputs || in_count > f->inputs - in_first) {
        llzs_set_error("llz_fir_matrix_mc_set_taps: inputs [%d, %d + %d) outside the handle's [0, %d)", in_first, in_first, in_count,
                       f->inputs);
        return LLZ_ERR_ARG;
    }
    if (llz_fade_refuse_set_taps(&f->fade, "llz_fir_matrix_mc_set_taps")) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    int rc = LLZ_OK;
    for (int o = 0; o < out_count && rc == LLZ_OK; o++)
        rc = firx_load_paths(f, out_first + o, in_first, in_count, taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len, 0);
    llzs_device_leave(prev);
    return rc;
}

/* the handle's own buffers and tables of a fade, at its first one, behind llz_fade.c's */
static int firx_fade_alloc(firx_t *f, const char *who)
{
    if (f->d_yn) return LLZ_OK;
    const size_t paths = (size_t)f->outputs * (size_t)f->inputs;
    const size_t ybytes = sizeof(float) * 2 * (size_t)f->G * (size_t)f->outputs * (size_t)f->ycap * (size_t)f->block;
    const int rc = llz_fade_reserve(&f->fade, who, "paths", paths, 2 * (size_t)f->P * (size_t)f->block);
    if (rc != LLZ_OK) return rc;
    float *yn = (float *)llzs_malloc(ybytes);
    unsigned char *dc = (unsigned char *)llzs_malloc(paths), *dof = (unsigned char *)llzs_malloc((size_t)f->outputs);
    unsigned char *hc = (unsigned char *)calloc(paths, 1), *hof = (unsigned char *)calloc((size_t)f->outputs, 1);
    if (!yn || !dc || !dof || !hc || !hof) {
        llzs_set_error("%s: no memory for the new taps' partial spectra and the tables of the fade: %zu B of device memory asked for "
                       "(%d groups x %d outputs x %d blocks x %d bins), and %zu B and %d B on the device and on the host", who,
                       ybytes, f->G, f->outputs, f->ycap, f->block, paths, f->outputs);
        llzs_free(yn); llzs_free(dc); llzs_free(dof); free(hc); free(hof);
        return LLZ_ERR_NOMEM;
    }
    f->d_yn = yn; f->d_conn_new = dc; f->d_ofade = dof; f->conn_new = hc; f->h_ofade = hof;
    return LLZ_OK;
}

int llz_fir_xfade_matrix_mc(unsigned long handle, int out_first, int out_count, int in_first, int in_count, const float *taps,
                            int fade_blocks)
{
    const char *who = "llz_fir_xfade_matrix_mc";
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX)) {
        llzs_set_error("%s: bad handle", who);
        return LLZ_ERR_ARG;
    }
    firx_t *f = (firx_t *)handle;
    if (!taps) {
        llzs_set_error("%s: no taps", who);
        return LLZ_ERR_ARG;
    }
    if (out_first < 0 || out_count < 1 || out_first >= f->outputs || out_count > f->outputs - out_first) {
        llzs_set_error("%s: outputs [%d, %d + %d) outside the handle's [0, %d)", who, out_first, out_first, out_count, f->outputs);
        return LLZ_ERR_ARG;
    }
    if (in_first < 0 || in_count < 1 || in_first >= f->inputs || in_count > f->inputs - in_first) {
        llzs_set_error("%s: inputs [%d, %d + %d) outside the handle's [0, %d)", who, in_first, in_first, in_count, f->inputs);
        return LLZ_ERR_ARG;
    }
    if (llz_fade_refuse(&f->fade, who, "paths", fade_blocks)) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const size_t paths = (size_t)f->outputs * (size_t)f->inputs;
    const size_t row = 2 * (size_t)f->P * (size_t)f->block;         /* floats of one path's spectra */
    int rc = firx_fade_alloc(f, who);
    /* the spectra as set_taps would upload them, on the stream behind the calls already issued: no launch reads these paths of
     * the new buffer before the tables below mark them */
    for (int o = 0; o < out_count && rc == LLZ_OK; o++) {
        const size_t first = (size_t)(out_first + o) * (size_t)f->inputs + (size_t)in_first;
        rc = llz_host_load_spectra(who, f->fade.d_new + first * row, row, in_count,
                                   taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len, f->flt_len, 2 * f->block, 1, 0, f->stream);
    }
    if (rc == LLZ_OK) {
        /* the tables are built aside and go up on the stream, behind the last launch that read them; the handle takes them
         * only when all three are up: the fade's own goes last, and with it the fade is committed */
        unsigned char *t = (unsigned char *)malloc(2 * paths + (size_t)f->outputs);
        if (!t) {
            llzs_set_error("%s: out of host memory (%zu B)", who, 2 * paths + (size_t)f->outputs);
            rc = LLZ_ERR_NOMEM;
        } else {
            unsigned char *tf = t, *tc = t + paths, *to = t + 2 * paths;
            memcpy(tf, f->fade.h_rows, paths);
            memcpy(tc, f->conn_new, paths);
            memcpy(to, f->h_ofade, (size_t)f->outputs);
            for (int o = 0; o < out_count; o++) {
                const size_t first = (size_t)(out_first + o) * (size_t)f->inputs + (size_t)in_first;
                const float *tp = taps + (size_t)o * (size_t)in_count * (size_t)f->flt_len;
                for (int i = 0; i < in_count; i++) {
                    tf[first + (size_t)i] = 1;
                    tc[first + (size_t)i] = (unsigned char)firx_row_connected(tp + (size_t)i * (size_t)f->flt_len, f->flt_len);
                }
                to[out_first + o] = 1;
            }
            rc = llzs_h2d(f->d_conn_new, tc, paths, f->stream);
            if (rc == LLZ_OK) rc = llzs_h2d(f->d_ofade, to, (size_t)f->outputs, f->stream);
            if (rc == LLZ_OK) rc = llz_fade_commit(&f->fade, tf, paths, fade_blocks, f->stream);
            if (rc == LLZ_OK) {
                memcpy(f->conn_new, tc, paths);
                memcpy(f->h_ofade, to, (size_t)f->outputs);
            }
            free(t);
        }
    }
    llzs_device_leave(prev);
    return rc;
}

int llz_fir_xfade_matrix_mc_left(unsigned long handle)
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX)) return LLZ_ERR_ARG;
    return llz_fade_left(&((const firx_t *)handle)->fade);
}

int llz_fir_matrix_mc_plan(unsigned long handle, int out[6])
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX) || !out) {
        llzs_set_error("llz_fir_matrix_mc_plan: bad handle or no out");
        return LLZ_ERR_ARG;
    }
    const firx_t *f = (const firx_t *)handle;
    out[0] = 2 * f->block; out[1] = f->P; out[2] = f->R; out[3] = f->k; out[4] = f->G; out[5] = f->connected;
    if (f->fade.blocks) {
        /* what a fading block reads: the paths connected under the old or the new taps */
        const size_t paths = (size_t)f->outputs * (size_t)f->inputs;
        out[5] = 0;
        for (size_t q = 0; q < paths; q++) out[5] += f->conn[q] || (f->fade.h_rows[q] && f->conn_new[q]);
    }
    return LLZ_OK;
}

int llz_fir_matrix_mc_flt_len(unsigned long handle)
{
    return LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX) ? ((firx_t *)handle)->flt_len : LLZ_ERR_ARG;
}

int llz_fir_matrix_mc_set_stream(unsigned long handle, void *stream)
{
    if (!LLZ_HANDLE_OK(handle, firx_t, LLZ_TAG_FIRX)) return LLZ_ERR_ARG;
    ((firx_t *)handle)->stream = stream;
    return LLZ_OK;
}
