/*
 * llz_tables.c -- the window, twiddle and MDCT tables of the transform and analysis family (llz_host.h), each built in ONE
 * place: libm and the reference's angle expressions in its operation order, so that the entries are the reference's to the last
 * bit, uploaded once per handle.  Compiled with -ffp-contract=off.
 */
#include <math.h>
#include <stdlib.h>
#include "llz_host.h"

int llz_host_window(double *w, int n, win_t win_type)
{
    switch (win_type) {                                            /* llz_asmodel.c:133-143 */
    case HAMMING:  llz_hamming(w, n);  return 1;
    case BLACKMAN: llz_blackman(w, n); return 1;
    case KAISER:   llz_kaiser(w, n);   return 1;
    default: return 0;
    }
}

void *llz_host_upload(const void *host, size_t bytes)
{
    void *dev = host ? llzs_malloc(bytes) : NULL;
    if (dev && llzs_h2d(dev, host, bytes, NULL) != LLZ_OK) { llzs_free(dev); dev = NULL; }
    return dev;
}

float *llz_host_upload_f32(const double *host, size_t count)
{
    float *t = (float *)malloc(sizeof(float) * count);
    for (size_t i = 0; t && i < count; i++) t[i] = (float)host[i];
    float *dev = (float *)llz_host_upload(t, sizeof(float) * count);
    free(t);
    return dev;
}

void *llz_host_zeros(size_t bytes)
{
    void *dev = llzs_malloc(bytes);
    if (dev && llzs_memset(dev, 0, bytes, NULL) != LLZ_OK) { llzs_free(dev); dev = NULL; }
    return dev;
}

short llz_host_q15(double v)
{
    const double t = v * (double)(1 << 15);
    const double r = (t > 0) ? floor(t + 0.5) : ceil(t - 0.5);
    int q = r > 2147483647.0 ? 2147483647 : r < -2147483648.0 ? (-2147483647 - 1) : (int)r;
    if (q > 32767) q = 32767;
    if (q < -32767) q = -32767;
    return (short)q;
}

/* how a table's double values become its entries: the three element types */
typedef void (*put_fn)(void *table, size_t i, double v);
static void put_f64(void *t, size_t i, double v) { ((double *)t)[i] = v; }
static void put_f32(void *t, size_t i, double v) { ((float *)t)[i] = (float)v; }
static void put_q15(void *t, size_t i, double v) { ((short *)t)[i] = llz_host_q15(v); }

static void *cs_table(int size, size_t elem, put_fn put)
{
    void *cs = malloc(elem * 2 * (size_t)size);
    for (int i = 0; cs && i < size; i++) {
        /* llz_fft.c:223-227, and llz_fft_fixed.c:243-247 (there without the cast, which changes nothing: the product is a double) */
        const double ang = (double)(2 * M_PI * i) / size;
        put(cs, (size_t)i, cos(ang));
        put(cs, (size_t)size + i, sin(ang));
    }
    void *dev = llz_host_upload(cs, elem * 2 * (size_t)size);
    free(cs);
    return dev;
}

double *llz_host_cs_f64(int size) { return (double *)cs_table(size, sizeof(double), put_f64); }
float  *llz_host_cs_f32(int size) { return (float *)cs_table(size, sizeof(float), put_f32); }
short  *llz_host_cs_q15(int size) { return (short *)cs_table(size, sizeof(short), put_q15); }

/* angle of entry k of a twiddle step's table; the expressions are the reference's (llz_mdct.c:418-441, :459-462; the same in
 * llz_mdct_fixed.c:335-366, :381-386), evaluated in its order, because the last bit of cos / sin -- and their Q15 rounding -- of
 * a differently rounded angle could differ */
static double mdct_angle(int quarter, int step, int k, int length)
{
    if (quarter) return -2 * M_PI * (k + 0.125) / length;
    const double n0 = ((double)length / 2 + 1) / 2;
    switch (step) {
    case LLZ_ROT_FWD_PRE:  return -(M_PI * k) / length;
    case LLZ_ROT_FWD_POST: return -2 * M_PI * n0 * (k + 0.5) / length;
    case LLZ_ROT_INV_PRE:  return (2 * M_PI * k * n0) / length;
    default:               return M_PI * (k + n0) / length;
    }
}

static void *rot_table(int quarter, int step, int count, int length, size_t elem, put_fn put)
{
    void *host = malloc(elem * 2 * (size_t)count);
    for (int k = 0; host && k < count; k++) {
        const double ang = mdct_angle(quarter, step, k, length);
        put(host, 2 * (size_t)k, cos(ang));
        put(host, 2 * (size_t)k + 1, sin(ang));
    }
    void *dev = llz_host_upload(host, elem * 2 * (size_t)count);
    free(host);
    return dev;
}

double *llz_host_mdct_rot_f64(int quarter, int step, int count, int length)
{
    return (double *)rot_table(quarter, step, count, length, sizeof(double), put_f64);
}

short *llz_host_mdct_rot_q15(int quarter, int step, int count, int length)
{
    return (short *)rot_table(quarter, step, count, length, sizeof(short), put_q15);
}

static int sums_tables(int N, void **d_fwd, void **d_inv, size_t elem, put_fn put)
{
    const int K = N >> 1;
    const size_t cnt = (size_t)K * N;
    void *fwd = malloc(elem * cnt), *inv = malloc(elem * cnt);
    if (fwd && inv) {
        for (int k = 0; k < K; k++)
            for (int n = 0; n < N; n++) {
                const double ang = (M_PI / (2 * N)) * (2 * n + 1 + K) * (2 * k + 1);   /* llz_mdct.c:392-399, llz_mdct_fixed.c:313-322 */
                put(fwd, (size_t)k * N + n, cos(ang));
                put(inv, (size_t)n * K + k, cos(ang));
            }
        *d_fwd = llz_host_upload(fwd, elem * cnt);
        *d_inv = llz_host_upload(inv, elem * cnt);
    }
    free(fwd); free(inv);
    return *d_fwd && *d_inv ? LLZ_OK : LLZ_ERR_NOMEM;
}

int llz_host_mdct_sums_f64(int N, double **fwd, double **inv)
{
    return sums_tables(N, (void **)fwd, (void **)inv, sizeof(double), put_f64);
}

int llz_host_mdct_sums_q15(int N, short **fwd, short **inv)
{
    return sums_tables(N, (void **)fwd, (void **)inv, sizeof(short), put_q15);
}

int llz_host_mdct_pretwiddles_f32(int N, float **tc, float **ts)
{
    const int N4 = N >> 2;
    float *tab = (float *)malloc(sizeof(float) * 2 * (size_t)N4);
    if (!tab) return LLZ_ERR_NOMEM;
    for (int k = 0; k < N4; k++) {
        tab[k] = (float)cos(mdct_angle(1, 0, k, N));                 /* llz_mdct.c:459-462 */
        tab[N4 + k] = (float)sin(mdct_angle(1, 0, k, N));
    }
    *tc = (float *)llz_host_upload(tab, sizeof(float) * (size_t)N4);
    *ts = (float *)llz_host_upload(tab + N4, sizeof(float) * (size_t)N4);
    free(tab);
    return *tc && *ts ? LLZ_OK : LLZ_ERR_NOMEM;
}
