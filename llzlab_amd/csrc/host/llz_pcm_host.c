/* llz_pcm_host.c -- host entry points of the PCM ingest / egress kernels (include/llz_pcm.h) */
#include "../../../include/llz_pcm.h"
#include "llz_host.h"

static int pcm_run(const char *who, int deint, const void *in, void *out, int channels, long n, float scale, void *stream)
{
    if (!in || !out || channels < 1 || n < 1) {
        llzs_set_error("llz_pcm_*: bad arguments");
        return LLZ_ERR_ARG;
    }
    const size_t count = (size_t)channels * (size_t)n;
    const size_t in_bytes = count * (deint ? sizeof(short) : sizeof(float));
    const size_t out_bytes = count * (deint ? sizeof(float) : sizeof(short));
    llz_bind_t b[2] = {{"in", in, in_bytes, LLZ_BIND_IN, NULL, 0, 0}, {"out", out, out_bytes, LLZ_BIND_OUT, NULL, 0, 0}};
    int rc = llz_bind(who, b, 2, stream);
    if (rc == LLZ_OK)
        rc = deint ? llzs_pcm_deinterleave_i16_f32((const short *)b[0].dev, (float *)b[1].dev, channels, n, scale, stream)
                   : llzs_pcm_interleave_f32_i16((const float *)b[0].dev, (short *)b[1].dev, channels, n, scale, stream);
    return llz_bind_finish(b, 2, stream, rc);
}

int llz_pcm_deinterleave_i16_f32(const short *in, float *out, int channels, long n, float scale, void *stream)
{
    return pcm_run("llz_pcm_deinterleave_i16_f32", 1, in, out, channels, n, scale, stream);
}

int llz_pcm_interleave_f32_i16(const float *in, short *out, int channels, long n, float scale, void *stream)
{
    return pcm_run("llz_pcm_interleave_f32_i16", 0, in, out, channels, n, scale, stream);
}
