/* llz_spectra.c -- the host side of the frequency-domain FIR forms (llz_fir_host.c parts 2 to 4, llz_fir_stream_host.c,
 * llz_fir_matrix_host.c, llz_adapt_host.c): the quadrant-exact cos / sin table, the double-precision transform of a tap partition,
 * the two packings of its bins and the way back from a packed row to taps, the twiddles of the delay-line forms, the chunked
 * upload of tap rows and the double -> float copy of caller taps.
 * Shared and per-row handles build their spectra here, so equal taps give equal float32 entries (tests/fir_tables_driver.c). */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"

void llz_host_cs_table(double *cs, int N)
{
    for (int i = 0; i < N; i++) {
        /* exact quadrant values keep the table symmetric */
        const double ang = 2.0 * M_PI * (double)i / (double)N;
        cs[2 * i] = (i == N / 4 || i == 3 * N / 4) ? 0.0 : cos(ang);
        cs[2 * i + 1] = (i == 0 || i == N / 2) ? 0.0 : sin(ang);
    }
}

static int spectra_bitrev(int i, int bits)
{
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

/* entry e of the result is bin bitrev_N(e) (llz_host.h); also the chirp spectra of llz_dft_host.c */
void llz_host_dif_f64(double *z, int N, const double *cs)
{
    for (int span = N; span >= 2; span /= 2) {
        const int half = span / 2, step = N / span;
        for (int base = 0; base < N; base += span)
            for (int j = 0; j < half; j++) {
                double *a = z + 2 * (base + j), *b = a + 2 * half;
                const double wr = cs[2 * j * step], wi = -cs[2 * j * step + 1];
                const double dr = a[0] - b[0], di = a[1] - b[1];
                a[0] += b[0]; a[1] += b[1];
                b[0] = dr * wr - di * wi; b[1] = dr * wi + di * wr;
            }
    }
}

/* z = DFT_N(taps[p B .. p B + B), zero-padded), B = N / 2, by radix-2 decimation in frequency in double, in place and left in
 * that transform's output order: entry e is bin bitrev_N(e) */
static void spectra_partition(double *z, const float *taps, int flt_len, int p, int N, const double *cs)
{
    const int B = N / 2;
    for (int i = 0; i < N; i++) {
        const long t = (long)p * B + i;
        z[2 * i] = (i < B && t < flt_len) ? (double)taps[t] : 0.0;
        z[2 * i + 1] = 0.0;
    }
    llz_host_dif_f64(z, N, cs);
}

/* Row p = the whole transform / N, rounded to float once: the device's forward transform leaves its bins in the same order, and
 * the product is bin-wise.  33 x 8192 points at 131073 taps: milliseconds, where a direct DFT would sum 10^9 terms. */
void llz_host_part_spectra(float *dst, const float *taps, int flt_len, int N, const double *cs, double *z)
{
    const int B = N / 2, P = (flt_len + B - 1) / B;
    for (int p = 0; p < P; p++) {
        spectra_partition(z, taps, flt_len, p, N, cs);
        float *row = dst + 2 * (size_t)p * (size_t)N;
        for (int i = 0; i < 2 * N; i++) row[i] = (float)(z[i] / N);
    }
}

/* A bin k < block has a zero top bit, so it sits at the even entry 2 bitrev_block(k) of the transform: the packed row is the even
 * entries as they lie, and the Nyquist bin (k = block) is entry 1. */
void llz_host_stream_spectra(float *dst, const float *taps, int flt_len, int block, const double *cs, double *z)
{
    const int N = 2 * block, P = (flt_len + block - 1) / block;
    const double scale = 1.0 / (2.0 * (double)N);
    for (int p = 0; p < P; p++) {
        spectra_partition(z, taps, flt_len, p, N, cs);
        float *row = dst + 2 * (size_t)p * (size_t)block;
        row[0] = (float)(z[0] * scale);
        row[1] = (float)(z[2] * scale);
        for (int i = 1; i < block; i++) {
            row[2 * i] = (float)(z[4 * i] * scale);
            row[2 * i + 1] = (float)(z[4 * i + 1] * scale);
        }
    }
}

/* The way back from one packed row (llz_adapt_mc_get_taps): the row holds Z_k / (2 N), k = 0 .. block, of a real sequence's
 * N-point spectrum Z, so sample t = (1 / N) sum_k Z_k e^(+2 pi j k t / N) = 2 Re DFT_N(conj(row), mirrored to all N bins)[t].
 * The first `count` samples, rounded to float once. */
void llz_host_stream_taps(float *taps, int count, const float *row, int block, const double *cs, double *z)
{
    const int N = 2 * block;
    int bits = 0;
    while ((1 << bits) < block) bits++;
    z[0] = (double)row[0]; z[1] = 0.0;
    z[2 * block] = (double)row[1]; z[2 * block + 1] = 0.0;
    for (int i = 1; i < block; i++) {
        const int k = spectra_bitrev(i, bits);
        z[2 * k] = (double)row[2 * i]; z[2 * k + 1] = -(double)row[2 * i + 1];
        z[2 * (N - k)] = (double)row[2 * i]; z[2 * (N - k) + 1] = (double)row[2 * i + 1];
    }
    llz_host_dif_f64(z, N, cs);
    for (int t = 0; t < count; t++) taps[t] = (float)(2.0 * z[2 * spectra_bitrev(t, bits + 1)]);
}

/* the transform's twiddles W_block^m, m < block / 2, then the split twiddles by position: W_N^bitrev(i), i < block */
int llz_host_stream_twiddles(float *d_tw, int block)
{
    const int B = block, N = 2 * B;
    int bits = 0;
    while ((1 << bits) < B) bits++;
    const size_t count = (size_t)B / 2 + (size_t)B;
    float *tw = (float *)malloc(sizeof(float) * 2 * count);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (tw && cs) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc == LLZ_OK) {
        llz_host_cs_table(cs, N);
        for (int m = 0; m < B / 2; m++) {
            tw[2 * m] = (float)cs[2 * (2 * m)];
            tw[2 * m + 1] = (float)(-cs[2 * (2 * m) + 1]);
        }
        for (int i = 0; i < B; i++) {
            const int k = spectra_bitrev(i, bits);
            tw[2 * (B / 2 + i)] = (float)cs[2 * k];
            tw[2 * (B / 2 + i) + 1] = (float)(-cs[2 * k + 1]);
        }
        rc = llzs_h2d_table(d_tw, tw, sizeof(float) * 2 * count);
    }
    free(tw); free(cs);
    return rc;
}

/* host staging of the spectra: whole tap rows up to this many bytes at a time, one row at least (2.1 MB at 131073 taps and 8192
 * points) */
#define SPECTRA_STAGE_BYTES ((size_t)8 << 20)

int llz_host_load_spectra(const char *who, float *d_dst, size_t row, int count, const float *taps, int flt_len, int N, int packed,
                          int at_init, void *stream)
{
    size_t chunk = SPECTRA_STAGE_BYTES / (sizeof(float) * row);
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)count) chunk = (size_t)count;
    float *hp = (float *)malloc(sizeof(float) * row * chunk);
    double *cs = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    double *z = (double *)malloc(sizeof(double) * 2 * (size_t)N);
    int rc = (hp && cs && z) ? LLZ_OK : LLZ_ERR_NOMEM;
    if (rc != LLZ_OK) llzs_set_error("%s: no host memory for %zu B of tap spectra", who, sizeof(float) * row * chunk);
    if (rc == LLZ_OK) llz_host_cs_table(cs, N);
    for (size_t r0 = 0; r0 < (size_t)count && rc == LLZ_OK; r0 += chunk) {
        const size_t rows = (size_t)count - r0 < chunk ? (size_t)count - r0 : chunk;
        for (size_t r = 0; r < rows; r++) {
            const float *t = taps + (r0 + r) * (size_t)flt_len;
            if (packed) llz_host_stream_spectra(hp + r * row, t, flt_len, N / 2, cs, z);
            else llz_host_part_spectra(hp + r * row, t, flt_len, N, cs, z);
        }
        float *d_h = d_dst + r0 * row;
        rc = at_init ? llzs_h2d_table(d_h, hp, sizeof(float) * row * rows) : llzs_h2d(d_h, hp, sizeof(float) * row * rows, stream);
    }
    free(hp); free(cs); free(z);
    return rc;
}

float *llz_host_taps_f32(const char *who, const double *taps, size_t count)
{
    float *t = (float *)malloc(sizeof(float) * count);
    if (!t) {
        llzs_set_error("%s: no host memory for %zu taps", who, count);
        return NULL;
    }
    for (size_t i = 0; i < count; i++) t[i] = (float)taps[i];
    return t;
}
