/* llz_asrc_host.c -- include/llz_asrc.h: llz_asrc_mc, the arbitrary-ratio resampler (kernel K3r, asrc.hip).  Its own handle and
 * tag.  The prototype is llz_host_design's low-pass, the staged call and the overlap refusal are llz_util.c's, the history
 * behind a call is the FIR family's tail launch.  What is this file's own is the integer state of every channel: the position
 * of its next output in the next call's buffer, its step and its glide (llz_asrc_time.h, the code the kernels run too).  The
 * host copy answers out_len, the counts of a call and next_time without a word from the device; the device copy is moved by a
 * launch behind each call, and overwritten from the host copy -- ordered on the stream -- by set_step and reset. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "llz_host.h"
#include "../llz_asrc_time.h"
#include "../../../include/llz_resample.h"
#include "../../../include/llz_asrc.h"

typedef struct {
    int tag;                    /* LLZ_TAG_ASRC */
    int device;
    int channels, frame_len, T, phases, pitch, table_lds;
    float *h_table;             /* HOST [phases + 1][T]: G of the definition (get_table) */
    float *d_table;             /* [phases + 1][pitch]: its device image, rows zero padded */
    llz_asrc_state *h_state;    /* HOST [channels] */
    void *d_state;              /* its device copy, as of the calls issued */
    int *h_counts;              /* HOST [channels]: the counts of the call at hand */
    long long received;         /* input samples taken per channel since init or reset */
    float *d_hist[2];           /* [channels][T - 1], ping-pong */
    int cur;
    void *stream;
    llz_stage_t st_in, st_out;
} asrc_t;

static void asrc_destroy(asrc_t *f)
{
    if (!f) return;
    llzs_free(f->d_table); llzs_free(f->d_state); llzs_free(f->d_hist[0]); llzs_free(f->d_hist[1]);
    llz_stage_release(&f->st_in); llz_stage_release(&f->st_out);
    free(f->h_table); free(f->h_state); free(f->h_counts);
    f->tag = 0;
    free(f);
}

static asrc_t *asrc_handle(unsigned long h, const char *who)
{
    if (LLZ_HANDLE_OK(h, asrc_t, LLZ_TAG_ASRC)) return (asrc_t *)h;
    llzs_set_error("%s: bad handle", who);
    return NULL;
}

static int asrc_step_ok(double step) { return step >= 1.0 / LLZ_RATIO_MAX && step <= (double)LLZ_RATIO_MAX; }   /* a NaN fails both */

static int asrc_refuse(const char *who, int channels, int frame_len, int taps, int phases, double cutoff, double gain, win_t win,
                       double step)
{
    if (channels < 1 || channels > 65535) {
        llzs_set_error("%s: channels %d outside 1..65535", who, channels);
        return 1;
    }
    if (frame_len < 1 || frame_len > LLZ_ASRC_MAX_FRAME) {
        llzs_set_error("%s: frame_len %d outside 1..%d", who, frame_len, LLZ_ASRC_MAX_FRAME);
        return 1;
    }
    if (taps < LLZ_ASRC_MIN_TAPS || taps > LLZ_ASRC_MAX_TAPS || (taps & 1)) {
        llzs_set_error("%s: taps %d is not an even number in %d..%d", who, taps, LLZ_ASRC_MIN_TAPS, LLZ_ASRC_MAX_TAPS);
        return 1;
    }
    if (phases < LLZ_ASRC_MIN_PHASES || phases > LLZ_ASRC_MAX_PHASES || (phases & (phases - 1))) {
        llzs_set_error("%s: phases %d is not a power of two in %d..%d", who, phases, LLZ_ASRC_MIN_PHASES, LLZ_ASRC_MAX_PHASES);
        return 1;
    }
    if (!(cutoff > 0.0 && cutoff <= 1.0)) {
        llzs_set_error("%s: cutoff %g outside (0, 1] of the input's Nyquist frequency", who, cutoff);
        return 1;
    }
    if (!isfinite(gain) || gain == 0.0) {
        llzs_set_error("%s: gain %g is not a finite value other than 0", who, gain);
        return 1;
    }
    if (win != HAMMING && win != BLACKMAN && win != KAISER) {
        llzs_set_error("%s: unknown window %d (HAMMING %d, BLACKMAN %d, KAISER %d)", who, win, HAMMING, BLACKMAN, KAISER);
        return 1;
    }
    if (!asrc_step_ok(step)) {
        llzs_set_error("%s: step %g outside 1/%d..%d input samples per output", who, step, LLZ_RATIO_MAX, LLZ_RATIO_MAX);
        return 1;
    }
    return 0;
}

/* G[p][k] = float(gain phases h[k phases + p]), p <= phases, k < T, into the host table and its padded image */
static int asrc_build_table(asrc_t *f, const char *who, double cutoff, double gain, win_t win, float *image)
{
    const int T = f->T, phases = f->phases, n = phases * T + 1;
    double *h = NULL;
    if (llz_host_design(LLZ_KIND_LPF, &h, n, cutoff / phases, 0.0, win) != n) {
        llzs_set_error("%s: the design of the %d-tap prototype failed", who, n);
        return LLZ_ERR_NOMEM;
    }
    const double scale = gain * phases;
    for (int p = 0; p <= phases; p++)
        for (int k = 0; k < T; k++) {
            const long u = (long)k * phases + p;
            const float g = u < n ? (float)(h[u] * scale) : 0.f;
            f->h_table[(size_t)p * T + k] = g;
            image[(size_t)p * f->pitch + k] = g;
        }
    free(h);
    return LLZ_OK;
}

/* every channel at time 0 with its target as its step, the history zeros: ordered on the handle's stream */
static int asrc_restart(asrc_t *f)
{
    const size_t hbytes = sizeof(float) * (size_t)f->channels * (size_t)(f->T - 1);
    for (int c = 0; c < f->channels; c++) {
        llz_asrc_state *s = &f->h_state[c];
        s->pos = (unsigned long long)(f->T - 1) << 32;
        s->inc = s->target; s->dinc = 0; s->left = 0; s->pad = 0;
    }
    f->received = 0;
    int rc = llzs_memset(f->d_hist[f->cur], 0, hbytes, f->stream);
    if (rc == LLZ_OK) rc = llzs_h2d(f->d_state, f->h_state, sizeof(llz_asrc_state) * (size_t)f->channels, f->stream);
    return rc;
}

unsigned long llz_asrc_mc_init(int channels, int frame_len, int taps, int phases, double cutoff, double gain, win_t win, double step)
{
    const char *who = "llz_asrc_mc_init";
    if (asrc_refuse(who, channels, frame_len, taps, phases, cutoff, gain, win, step)) return LLZ_BAD_HANDLE;
    asrc_t *f = (asrc_t *)calloc(1, sizeof(*f));
    if (!f) {
        llzs_set_error("%s: no host memory for the handle (%zu B)", who, sizeof(*f));
        return LLZ_BAD_HANDLE;
    }
    f->tag = LLZ_TAG_ASRC;
    f->device = llzs_device_get();
    f->channels = channels; f->frame_len = frame_len; f->T = taps; f->phases = phases; f->pitch = LLZ_ASRC_PITCH(taps);
    const size_t rows = (size_t)phases + 1, tbytes = sizeof(float) * rows * (size_t)f->pitch;
    const size_t sbytes = sizeof(llz_asrc_state) * (size_t)channels, hbytes = sizeof(float) * (size_t)channels * (size_t)(taps - 1);
    f->table_lds = tbytes <= LLZ_ASRC_LDS_TABLE_BYTES && llzs_tune(LLZS_TUNE_ASRC_TABLE_GLOBAL) != 1;
    float *image = (float *)calloc(rows * (size_t)f->pitch, sizeof(float));
    f->h_table = (float *)malloc(sizeof(float) * rows * (size_t)taps);
    f->h_state = (llz_asrc_state *)calloc((size_t)channels, sizeof(llz_asrc_state));
    f->h_counts = (int *)calloc((size_t)channels, sizeof(int));
    int rc = LLZ_OK;
    if (!image || !f->h_table || !f->h_state || !f->h_counts) {
        llzs_set_error("%s: no host memory for the table (%zu B) and the state of %d channels", who, tbytes, channels);
        rc = LLZ_ERR_NOMEM;
    }
    if (rc == LLZ_OK) rc = asrc_build_table(f, who, cutoff, gain, win, image);
    if (rc == LLZ_OK) {
        f->d_table = (float *)llzs_malloc(tbytes);
        f->d_state = llzs_malloc(sbytes);
        f->d_hist[0] = (float *)llzs_malloc(hbytes);
        f->d_hist[1] = (float *)llzs_malloc(hbytes);
        if (!f->d_table || !f->d_state || !f->d_hist[0] || !f->d_hist[1]) {
            llzs_set_error("%s: no device memory for the table, the state and the history: %zu B, %zu B and 2 x %zu B asked for", who,
                           tbytes, sbytes, hbytes);
            rc = LLZ_ERR_NOMEM;
        }
    }
    if (rc == LLZ_OK) rc = llzs_h2d_table(f->d_table, image, tbytes);
    if (rc == LLZ_OK) {
        const unsigned long long inc = (unsigned long long)llround(ldexp(step, 32));
        for (int c = 0; c < channels; c++) f->h_state[c].target = inc;
        rc = asrc_restart(f);
    }
    if (rc == LLZ_OK) rc = llzs_sync(NULL);
    free(image);
    if (rc != LLZ_OK) {
        asrc_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_asrc_mc_uninit(unsigned long h)
{
    if (LLZ_HANDLE_OK(h, asrc_t, LLZ_TAG_ASRC)) {
        asrc_t *f = (asrc_t *)h;
        const int prev = llzs_device_enter(f->device);
        llzs_sync(f->stream);
        asrc_destroy(f);
        llzs_device_leave(prev);
    }
}

int llz_asrc_mc_set_stream(unsigned long h, void *stream)
{
    asrc_t *f = asrc_handle(h, "llz_asrc_mc_set_stream");
    if (!f) return LLZ_ERR_ARG;
    f->stream = stream;
    return LLZ_OK;
}

/* the counts a call of n_in samples delivers, from the host state alone, into f->h_counts; returns the largest */
static long asrc_counts(asrc_t *f, long n_in)
{
    const unsigned long long bound = (unsigned long long)(f->T - 1 + n_in - f->T / 2) << 32;
    long most = 0;
    for (int c = 0; c < f->channels; c++) {
        const unsigned int count = llz_asrc_count(&f->h_state[c], bound);
        f->h_counts[c] = (int)count;
        if ((long)count > most) most = (long)count;
    }
    return most;
}

static int asrc_n_in_ok(const asrc_t *f, const char *who, long n_in)
{
    if (n_in >= 0 && n_in <= f->frame_len) return 1;
    llzs_set_error("%s: n_in %ld outside 0..%d (the init's frame_len)", who, n_in, f->frame_len);
    return 0;
}

long llz_asrc_mc_out_len(unsigned long h, long n_in, int *counts)
{
    const char *who = "llz_asrc_mc_out_len";
    asrc_t *f = asrc_handle(h, who);
    if (!f || !asrc_n_in_ok(f, who, n_in)) return LLZ_ERR_ARG;
    const long most = asrc_counts(f, n_in);
    if (counts) memcpy(counts, f->h_counts, sizeof(int) * (size_t)f->channels);
    return most;
}

static long asrc_process(asrc_t *f, const float *in, long n_in, float *out, long out_pitch, int *counts)
{
    const char *who = "llz_asrc_mc";
    const int C = f->channels;
    if (!asrc_n_in_ok(f, who, n_in)) return LLZ_ERR_ARG;
    if (out_pitch < 0 || (n_in > 0 && !in)) {
        llzs_set_error("%s: out_pitch %ld is negative, or no input for n_in %ld", who, out_pitch, n_in);
        return LLZ_ERR_ARG;
    }
    const long most = asrc_counts(f, n_in);
    for (int c = 0; c < C; c++)
        if (f->h_counts[c] > out_pitch) {
            llzs_set_error("%s: channel %d delivers %d outputs for n_in %ld, out_pitch is %ld (llz_asrc_mc_out_len gives the counts)",
                           who, c, f->h_counts[c], n_in, out_pitch);
            return LLZ_ERR_ARG;
        }
    if (most > 0 && !out) {
        llzs_set_error("%s: no output buffer for %ld outputs", who, most);
        return LLZ_ERR_ARG;
    }
    if (counts) memcpy(counts, f->h_counts, sizeof(int) * (size_t)C);
    if (n_in == 0) return 0;                                    /* nothing arrives, nothing is due: the state stands */
    const size_t in_bytes = sizeof(float) * (size_t)C * (size_t)n_in;
    const size_t out_bytes = most ? sizeof(float) * ((size_t)(C - 1) * (size_t)out_pitch + (size_t)most) : 0;
    const int in_dev = llzs_is_device_ptr(in), out_dev = most ? llzs_is_device_ptr(out) : 0;
    if (in_dev < 0 || out_dev < 0) return LLZ_ERR_ARG;          /* a buffer of another GPU: refused, message set */
    if (llz_refuse_device_overlap(who, "in", in, in_bytes, in_dev, "out", out, out_bytes, out_dev)) return LLZ_ERR_ARG;
    int rc = LLZ_OK;
    const float *d_in = (const float *)llz_stage_in(&f->st_in, in, in_bytes, in_dev, f->stream, &rc);
    /* a staged output has rows of `most`: only each row's own count goes back to the caller */
    const long d_pitch = out_dev ? out_pitch : most;
    float *d_out = most ? (float *)llz_stage_out(&f->st_out, out, sizeof(float) * (size_t)C * (size_t)most, out_dev, &rc) : NULL;
    if (rc == LLZ_OK && most)
        rc = llzs_asrc_f32(d_in, d_out, f->d_hist[f->cur], f->d_table, f->d_state, C, n_in, n_in, d_pitch, f->T, f->phases,
                           f->table_lds, most, f->stream);
    if (rc == LLZ_OK)
        rc = llzs_fir_tail_f32(d_in, f->d_hist[f->cur], f->d_hist[f->cur ^ 1], C, n_in, n_in, f->T, f->stream);
    if (rc == LLZ_OK) rc = llzs_asrc_advance(f->d_state, C, n_in, f->T, f->stream);
    /* a launch that fails was not issued: until the advance, the last of the three, is on the stream neither copy of the state
     * has moved and the history written is not the current one -- the handle stands where it stood, whichever launch failed */
    if (rc != LLZ_OK) return rc;
    f->cur ^= 1;
    for (int c = 0; c < C; c++) llz_asrc_advance(&f->h_state[c], (unsigned int)f->h_counts[c], (unsigned long long)n_in);
    f->received += n_in;
    if (most && !out_dev) {
        int whole = out_pitch == most;
        for (int c = 0; c < C && whole; c++) whole = f->h_counts[c] == most;
        const size_t bytes = sizeof(float) * (size_t)C * (size_t)most;
        if (whole) {
            rc = llzs_d2h(out, d_out, bytes, f->stream);
        } else {                                                /* one copy into a bounce buffer, then each row's own count */
            float *bounce = (float *)malloc(bytes);
            if (!bounce) {
                llzs_set_error("%s: no host memory for %zu B of staged outputs (the handle has advanced; the outputs are lost)", who, bytes);
                return LLZ_ERR_NOMEM;
            }
            rc = llzs_d2h(bounce, d_out, bytes, f->stream);
            for (int c = 0; c < C && rc == LLZ_OK; c++)
                memcpy(out + (size_t)c * (size_t)out_pitch, bounce + (size_t)c * (size_t)most, sizeof(float) * (size_t)f->h_counts[c]);
            free(bounce);
        }
        if (rc != LLZ_OK) return rc;
    }
    return most;
}

long llz_asrc_mc(unsigned long h, const float *in, long n_in, float *out, long out_pitch, int *counts)
{
    asrc_t *f = asrc_handle(h, "llz_asrc_mc");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const long rc = asrc_process(f, in, n_in, out, out_pitch, counts);
    llzs_device_leave(prev);
    return rc;
}

/* the handle and a channel range inside it, or NULL with a message naming who */
static asrc_t *asrc_range(unsigned long h, const char *who, int first, int count, const void *buf)
{
    asrc_t *f = asrc_handle(h, who);
    if (!f) return NULL;
    if (!buf) {
        llzs_set_error("%s: NULL buffer", who);
        return NULL;
    }
    if (first < 0 || count < 1 || first >= f->channels || count > f->channels - first) {
        llzs_set_error("%s: channels [%d, %d + %d) outside the handle's [0, %d)", who, first, first, count, f->channels);
        return NULL;
    }
    return f;
}

int llz_asrc_mc_set_step(unsigned long h, int first, int count, const double *step, long ramp)
{
    const char *who = "llz_asrc_mc_set_step";
    asrc_t *f = asrc_range(h, who, first, count, step);
    if (!f) return LLZ_ERR_ARG;
    if (ramp < 0 || ramp > 2147483647L) {
        llzs_set_error("%s: ramp %ld outside 0..2147483647 outputs", who, ramp);
        return LLZ_ERR_ARG;
    }
    for (int c = 0; c < count; c++)
        if (!asrc_step_ok(step[c])) {
            llzs_set_error("%s: step %g of channel %d outside 1/%d..%d", who, step[c], first + c, LLZ_RATIO_MAX, LLZ_RATIO_MAX);
            return LLZ_ERR_ARG;
        }
    llz_asrc_state *next = (llz_asrc_state *)malloc(sizeof(llz_asrc_state) * (size_t)count);
    if (!next) {
        llzs_set_error("%s: no host memory for the state of %d channels", who, count);
        return LLZ_ERR_NOMEM;
    }
    for (int c = 0; c < count; c++) {
        llz_asrc_state s = f->h_state[first + c];
        s.target = (unsigned long long)llround(ldexp(step[c], 32));
        if (ramp == 0) {
            s.inc = s.target; s.dinc = 0; s.left = 0;
        } else {                                                /* a glide in flight hands over its current step */
            s.dinc = ((long long)s.target - (long long)s.inc) / (long long)ramp;
            s.left = (unsigned int)ramp;
        }
        next[c] = s;
    }
    const int prev = llzs_device_enter(f->device);
    const int rc = llzs_h2d((llz_asrc_state *)f->d_state + first, next, sizeof(llz_asrc_state) * (size_t)count, f->stream);
    llzs_device_leave(prev);
    if (rc == LLZ_OK) memcpy(f->h_state + first, next, sizeof(llz_asrc_state) * (size_t)count);
    free(next);
    return rc;
}

int llz_asrc_mc_get_step(unsigned long h, int first, int count, double *step, long *ramp_left)
{
    asrc_t *f = asrc_range(h, "llz_asrc_mc_get_step", first, count, step);
    if (!f) return LLZ_ERR_ARG;
    for (int c = 0; c < count; c++) {
        step[c] = ldexp((double)f->h_state[first + c].inc, -32);            /* a step is below 2^37: exact */
        if (ramp_left) ramp_left[c] = (long)f->h_state[first + c].left;
    }
    return LLZ_OK;
}

int llz_asrc_mc_next_time(unsigned long h, int first, int count, long long *whole, unsigned int *frac)
{
    asrc_t *f = asrc_range(h, "llz_asrc_mc_next_time", first, count, whole);
    if (!f) return LLZ_ERR_ARG;
    for (int c = 0; c < count; c++) {
        const unsigned long long pos = f->h_state[first + c].pos;
        whole[c] = (long long)(pos >> 32) + f->received - (f->T - 1);
        if (frac) frac[c] = (unsigned int)pos;
    }
    return LLZ_OK;
}

int llz_asrc_mc_get_table(unsigned long h, float *dst, int capacity)
{
    const char *who = "llz_asrc_mc_get_table";
    asrc_t *f = asrc_handle(h, who);
    if (!f) return LLZ_ERR_ARG;
    const int count = (f->phases + 1) * f->T;
    if (!dst || capacity < count) {
        llzs_set_error("%s: no buffer, or capacity %d < %d", who, capacity, count);
        return LLZ_ERR_ARG;
    }
    memcpy(dst, f->h_table, sizeof(float) * (size_t)count);
    return count;
}

int llz_asrc_mc_reset(unsigned long h)
{
    asrc_t *f = asrc_handle(h, "llz_asrc_mc_reset");
    if (!f) return LLZ_ERR_ARG;
    const int prev = llzs_device_enter(f->device);
    const int rc = asrc_restart(f);
    llzs_device_leave(prev);
    return rc;
}

int llz_asrc_mc_plan(unsigned long h, int out[4])
{
    asrc_t *f = asrc_handle(h, "llz_asrc_mc_plan");
    if (!f) return LLZ_ERR_ARG;
    if (!out) {
        llzs_set_error("llz_asrc_mc_plan: no out");
        return LLZ_ERR_ARG;
    }
    out[0] = f->T; out[1] = f->phases; out[2] = f->T - 1; out[3] = f->table_lds ? 0 : 1;
    return LLZ_OK;
}
