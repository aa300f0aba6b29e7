/* llz_util.c -- small host helpers of the C layer */
#include <stdint.h>
#include "llz_host.h"

int llz_ranges_intersect(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    if (!a_bytes || !b_bytes) return 0;
    return pa < pb ? pb - pa < a_bytes : pa - pb < b_bytes;
}

int llz_refuse_device_overlap(const char *who, const char *in_name, const void *in, size_t in_bytes, int in_dev,
                              const char *out_name, const void *out, size_t out_bytes, int out_dev)
{
    if (in_dev != 1 || out_dev != 1 || !llz_ranges_intersect(in, in_bytes, out, out_bytes)) return LLZ_OK;
    llzs_set_error("%s: %s may not overlap %s (device memory)", who, out_name, in_name);
    return LLZ_ERR_ARG;
}

int llz_in_place(const void *p, int dev) { return dev == 1 && (uintptr_t)p % LLZ_VEC_ALIGN == 0; }

int llz_stage_load(void *d_stage, const void *user, size_t bytes, int user_dev, void *stream)
{
    return user_dev == 1 ? llzs_d2d(d_stage, user, bytes, stream) : llzs_h2d(d_stage, user, bytes, stream);
}

int llz_stage_store(void *user, const void *d_stage, size_t bytes, int user_dev, void *stream)
{
    return user_dev == 1 ? llzs_d2d(user, d_stage, bytes, stream) : llzs_d2h(user, d_stage, bytes, stream);
}

void *llz_stage_reserve(llz_stage_t *s, size_t bytes)
{
    if (s->bytes >= bytes && s->dev) return s->dev;
    if (s->dev) llzs_free(s->dev);
    s->dev = llzs_malloc(bytes);
    s->bytes = s->dev ? bytes : 0;
    return s->dev;
}

void *llz_stage_out(llz_stage_t *s, void *user, size_t bytes, int user_dev, int *rc)
{
    if (*rc != LLZ_OK || user_dev) return user;
    void *d = llz_stage_reserve(s, bytes);
    if (!d) *rc = LLZ_ERR_NOMEM;
    return d;
}

const void *llz_stage_in(llz_stage_t *s, const void *user, size_t bytes, int user_dev, void *stream, int *rc)
{
    if (*rc != LLZ_OK || user_dev) return user;
    void *d = llz_stage_out(s, NULL, bytes, 0, rc);
    if (d) *rc = llzs_h2d(d, user, bytes, stream);
    return d;
}

void llz_stage_release(llz_stage_t *s)
{
    if (s->dev) llzs_free(s->dev);
    s->dev = NULL;
    s->bytes = 0;
}
