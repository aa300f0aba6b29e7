/* llz_util.c -- small host helpers of the C layer */
#include <stdint.h>
#include <stdlib.h>
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

static int llz_stage_load(void *d_stage, const void *user, size_t bytes, int user_dev, void *stream)
{
    return user_dev == 1 ? llzs_d2d(d_stage, user, bytes, stream) : llzs_h2d(d_stage, user, bytes, stream);
}

static int llz_stage_store(void *user, const void *d_stage, size_t bytes, int user_dev, void *stream)
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

const void *llz_vec_stage_in(llz_stage_t *s, const void *user, size_t bytes, int user_dev, void *stream, int *rc)
{
    if (*rc != LLZ_OK || llz_in_place(user, user_dev)) return user;
    void *d = llz_vec_stage_out(s, NULL, bytes, 0, rc);
    if (d) *rc = llz_stage_load(d, user, bytes, user_dev, stream);
    return d;
}

void *llz_vec_stage_out(llz_stage_t *s, void *user, size_t bytes, int user_dev, int *rc)
{
    if (*rc != LLZ_OK || llz_in_place(user, user_dev)) return user;
    void *d = llz_stage_reserve(s, bytes);
    if (!d) *rc = LLZ_ERR_NOMEM;
    return d;
}

void llz_vec_stage_back(void *user, const void *d, size_t bytes, int user_dev, void *stream, int *rc)
{
    if (*rc == LLZ_OK && d != user) *rc = llz_stage_store(user, d, bytes, user_dev, stream);
}

/* ---- the one-shot calls' binder ---- */

int llz_bind(const char *who, llz_bind_t *b, int count, void *stream)
{
    for (int i = 0; i < count; i++) {
        b[i].dev = NULL; b[i].staged = 0;
        if (b[i].kind == LLZ_BIND_SCRATCH || !b[i].user || !b[i].bytes) { b[i].user = NULL; continue; }
        b[i].on_dev = llzs_is_device_ptr(b[i].user);
        if (b[i].on_dev < 0) return LLZ_ERR_ARG;                     /* memory of another GPU: refused, message set */
    }
    for (int i = 0; i < count; i++)
        for (int o = 0; o < count && b[i].user && b[i].kind == LLZ_BIND_IN; o++)
            if (b[o].user && b[o].kind == LLZ_BIND_OUT &&
                llz_refuse_device_overlap(who, b[i].name, b[i].user, b[i].bytes, b[i].on_dev, b[o].name, b[o].user, b[o].bytes,
                                          b[o].on_dev))
                return LLZ_ERR_ARG;
    for (int i = 0; i < count; i++) {
        if (!b[i].user) continue;
        b[i].dev = (void *)b[i].user;
        if (b[i].on_dev) continue;
        int twin = -1;                                               /* y == x, b == a: one copy, and the one-row kernels */
        for (int j = 0; j < i && b[i].kind == LLZ_BIND_IN; j++)
            if (b[j].kind == LLZ_BIND_IN && b[j].user == b[i].user) twin = j;
        if (twin >= 0) { b[i].dev = b[twin].dev; continue; }
        b[i].dev = llzs_malloc(b[i].bytes);
        if (!b[i].dev) return LLZ_ERR_NOMEM;
        b[i].staged = 1;
        if (b[i].kind == LLZ_BIND_IN) {
            const int rc = llzs_h2d(b[i].dev, b[i].user, b[i].bytes, stream);
            if (rc != LLZ_OK) return rc;
        }
    }
    return LLZ_OK;
}

void *llz_bind_scratch(llz_bind_t *b, size_t bytes, int *rc)
{
    if (*rc != LLZ_OK) return NULL;
    b->dev = llzs_malloc(bytes);
    b->staged = b->dev != NULL;
    if (!b->dev) *rc = LLZ_ERR_NOMEM;
    return b->dev;
}

int llz_bind_finish(llz_bind_t *b, int count, void *stream, int rc)
{
    int any = 0;
    for (int i = 0; i < count; i++) {
        any |= b[i].staged;
        if (rc == LLZ_OK && b[i].staged && b[i].kind == LLZ_BIND_OUT) rc = llzs_d2h((void *)b[i].user, b[i].dev, b[i].bytes, stream);
    }
    if (any) llzs_sync(stream);                                      /* nothing in flight reads the copies freed below */
    for (int i = 0; i < count; i++)
        if (b[i].staged) llzs_free(b[i].dev);
    return rc;
}

/* ---- the head of a handle ---- */

void *llz_handle_new(size_t size, int tag, int on_device)
{
    llz_head_t *h = (llz_head_t *)calloc(1, size);
    if (!h) return NULL;
    h->tag = tag;
    h->device = on_device ? llzs_device_get() : -1;
    return h;
}

void *llz_handle(unsigned long handle, int tag, const char *who)
{
    if (LLZ_HANDLE_OK(handle, llz_head_t, tag)) return (void *)handle;
    if (who) llzs_set_error("%s: bad handle", who);
    return NULL;
}

int llz_handle_set_stream(unsigned long handle, int tag, const char *who, void *stream)
{
    llz_head_t *h = (llz_head_t *)llz_handle(handle, tag, who);
    if (!h) return LLZ_ERR_ARG;
    h->stream = stream;
    return LLZ_OK;
}

void llz_handle_retire(unsigned long handle, int tag, void (*destroy)(void *))
{
    llz_head_t *h = (llz_head_t *)llz_handle(handle, tag, NULL);
    if (!h) return;
    const int prev = llzs_device_enter(h->device);
    llzs_sync(h->stream);
    destroy(h);
    llzs_device_leave(prev);
}
