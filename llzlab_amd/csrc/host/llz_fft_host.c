/*
 * llz_fft_host.c -- handle layer of the FFT path: reference symbols llz_fft_* (reference libllzfilter/llz_fft.c:142-249)
 * and llz_fft_fixed_* (llz_fft_fixed.c:152-268) plus the batched float32 / int32 entry points.  Twiddle tables are
 * built on the host exactly as the reference builds them (llz_tables.c) and uploaded once per handle.
 */
#include <stdlib.h>
#include <string.h>
#include "../../../include/llz_fft.h"
#include "../../../include/llz_fft_fixed.h"
#include "llz_host.h"

static int is_pow2_in_range(int size, int lo, int hi)
{
    return size >= lo && size <= hi && (size & (size - 1)) == 0;
}

/* ---- double, single transform ---- */

typedef struct {
    llz_head_t head;
    int size;
    double *d_cs;       /* size cos then size sin */
    double *d_data;     /* 2*size doubles */
} fft1_t;

static void fft1_destroy(void *p)
{
    fft1_t *f = (fft1_t *)p;
    llzs_free(f->d_cs); llzs_free(f->d_data);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_fft_init(int size)
{
    if (!is_pow2_in_range(size, 2, LLZS_FFT_MAX)) {
        llzs_set_error("llz_fft_init: size %d must be a power of two in 2..%d", size, LLZS_FFT_MAX);
        return LLZ_BAD_HANDLE;
    }
    fft1_t *f = (fft1_t *)llz_handle_new(sizeof(*f), LLZ_TAG_FFT1, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->size = size;
    f->d_cs = llz_host_cs_f64(size);
    f->d_data = (double *)llzs_malloc(sizeof(double) * 2 * (size_t)size);
    if (!f->d_cs || !f->d_data || f->head.device < 0) {
        fft1_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_fft_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_FFT1, fft1_destroy); }

static void fft1_run(unsigned long handle, double *data, int inverse)
{
    fft1_t *f = (fft1_t *)llz_handle(handle, LLZ_TAG_FFT1, NULL);
    if (!f || !data) {
        llzs_set_error("llz_fft/llz_ifft: bad handle or NULL data");
        return;                                                   /* void in the reference ABI */
    }
    const size_t bytes = sizeof(double) * 2 * (size_t)f->size;
    const int prev = llzs_device_enter(f->head.device);
    int rc = llzs_h2d(f->d_data, data, bytes, NULL);
    if (rc == LLZ_OK)   /* above 4096 points: outer passes over device memory around 4096-point blocks (fft_large.hip) */
        rc = f->size <= 4096 ? llzs_fft_f64(f->d_data, f->size, f->d_cs, inverse, NULL)
                             : llzs_fft_large_f64(f->d_data, f->size, f->d_cs, inverse, NULL);
    if (rc == LLZ_OK) (void)llzs_d2h(data, f->d_data, bytes, NULL);
    llzs_device_leave(prev);
}

void llz_fft(unsigned long handle, double *data)  { fft1_run(handle, data, 0); }
void llz_ifft(unsigned long handle, double *data) { fft1_run(handle, data, 1); }

/* ---- float32 batch ---- */

typedef struct {
    llz_head_t head;
    int size;
    float *d_cs;
    float *d_twb;       /* above 4096 points: the large path's LDS-block table in memory */
    llz_stage_t st;
} fftb_t;

static void fftb_destroy(void *p)
{
    fftb_t *f = (fftb_t *)p;
    llzs_free(f->d_cs);
    llzs_free(f->d_twb);
    llz_stage_release(&f->st);
    f->head.tag = 0;
    free(f);
}

/* the float32 batch on device memory: the register / LDS kernels of fft.hip up to 4096 points, fft_large.hip above */
static int fftb_launch(const fftb_t *f, float *d, int count, int inverse)
{
    return f->size <= 4096 ? llzs_fft_f32(d, count, f->size, f->d_cs, inverse, f->head.stream)
                           : llzs_fft_large_f32(d, count, f->size, f->d_cs, f->d_twb, inverse, f->head.stream);
}

unsigned long llz_fft_batch_init(int size)
{
    if (!is_pow2_in_range(size, 8, LLZS_FFT_MAX)) {
        llzs_set_error("llz_fft_batch_init: size %d must be a power of two in 8..%d", size, LLZS_FFT_MAX);
        return LLZ_BAD_HANDLE;
    }
    fftb_t *f = (fftb_t *)llz_handle_new(sizeof(*f), LLZ_TAG_FFTB, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->size = size;
    f->d_cs = llz_host_cs_f32(size);
    int ok = f->d_cs != NULL;
    const size_t twb = size > 4096 ? (size_t)llzs_fft_large_twb_bytes(size) : 0;
    if (ok && twb) {
        f->d_twb = (float *)llzs_malloc(twb);
        ok = f->d_twb && llzs_fft_large_twb(f->d_twb, size, f->d_cs, NULL) == LLZ_OK && llzs_sync(NULL) == LLZ_OK;
    }
    if (!ok) {
        fftb_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_fft_batch_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_FFTB, fftb_destroy); }

int llz_fft_batch_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_FFTB, "llz_fft_batch_set_stream", stream);
}

static int fftb_run(unsigned long handle, float *data, int count, int inverse)
{
    fftb_t *f = (fftb_t *)llz_handle(handle, LLZ_TAG_FFTB, NULL);
    if (!f || !data || count < 1) {
        llzs_set_error("llz_fft_batch: bad handle, NULL data or count %d", count);
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(float) * 2 * (size_t)f->size * (size_t)count;
    const int prev = llzs_device_enter(f->head.device);
    const int on_dev = llzs_is_device_ptr(data);
    int rc = on_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;
    float *d = (float *)llz_vec_stage_in(&f->st, data, bytes, on_dev, f->head.stream, &rc);
    if (rc == LLZ_OK) rc = fftb_launch(f, d, count, inverse);
    llz_vec_stage_back(data, d, bytes, on_dev, f->head.stream, &rc);
    llzs_device_leave(prev);
    return rc;
}

int llz_fft_batch(unsigned long handle, float *data, int count)  { return fftb_run(handle, data, count, 0); }
int llz_ifft_batch(unsigned long handle, float *data, int count) { return fftb_run(handle, data, count, 1); }

/* ---- fixed point ---- */

typedef struct {
    llz_head_t head;
    int size;
    short *d_cs;
    llz_stage_t st;
} fftx_t;

static void fftx_destroy(void *p)
{
    fftx_t *f = (fftx_t *)p;
    llzs_free(f->d_cs);
    llz_stage_release(&f->st);
    f->head.tag = 0;
    free(f);
}

unsigned long llz_fft_fixed_init(int size)
{
    if (!is_pow2_in_range(size, 2, 4096)) {
        llzs_set_error("llz_fft_fixed_init: size %d must be a power of two in 2..4096", size);
        return LLZ_BAD_HANDLE;
    }
    fftx_t *f = (fftx_t *)llz_handle_new(sizeof(*f), LLZ_TAG_FFTX, 1);
    if (!f) return LLZ_BAD_HANDLE;
    f->size = size;
    f->d_cs = llz_host_cs_q15(size);
    if (!f->d_cs) {
        fftx_destroy(f);
        return LLZ_BAD_HANDLE;
    }
    return (unsigned long)f;
}

void llz_fft_fixed_uninit(unsigned long handle) { llz_handle_retire(handle, LLZ_TAG_FFTX, fftx_destroy); }

int llz_fft_fixed_set_stream(unsigned long handle, void *stream)
{
    return llz_handle_set_stream(handle, LLZ_TAG_FFTX, "llz_fft_fixed_set_stream", stream);
}

static int fftx_run(unsigned long handle, int *data, int count, int inverse)
{
    fftx_t *f = (fftx_t *)llz_handle(handle, LLZ_TAG_FFTX, NULL);
    if (!f || !data || count < 1) {
        llzs_set_error("llz_fft_fixed: bad handle, NULL data or count %d", count);
        return LLZ_ERR_ARG;
    }
    const size_t bytes = sizeof(int) * 2 * (size_t)f->size * (size_t)count;
    const int prev = llzs_device_enter(f->head.device);
    const int on_dev = llzs_is_device_ptr(data);
    int rc = on_dev < 0 ? LLZ_ERR_ARG : LLZ_OK;
    int *d = (int *)llz_vec_stage_in(&f->st, data, bytes, on_dev, f->head.stream, &rc);
    if (rc == LLZ_OK) rc = llzs_fft_fixed(d, count, f->size, f->d_cs, inverse, f->head.stream);
    llz_vec_stage_back(data, d, bytes, on_dev, f->head.stream, &rc);
    llzs_device_leave(prev);
    return rc;
}

void llz_fft_fixed(unsigned long handle, int *data)  { (void)fftx_run(handle, data, 1, 0); }
void llz_ifft_fixed(unsigned long handle, int *data) { (void)fftx_run(handle, data, 1, 1); }
int llz_fft_fixed_batch(unsigned long handle, int *data, int count)  { return fftx_run(handle, data, count, 0); }
int llz_ifft_fixed_batch(unsigned long handle, int *data, int count) { return fftx_run(handle, data, count, 1); }
