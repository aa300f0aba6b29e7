// fir_bank.hip -- K4c: the 1024-point overlap-save FIR with a tap set PER CHANNEL (llz_fir_bank_mc).
//
// The walk is fir_ols.hip's segment walk (k_fir_ols_seg_f32), step for step (ols_walk.hpp): a half-wave owns a job of 1536 new samples,
// walks a segment of up to 16 jobs of one channel with the 256-sample overlap carried in registers, and requests the next
// job -- across segment boundaries the first job and the halo of its NEXT segment -- before it transforms the current one:
// every input sample is requested once, a half-wave instruction moves 128 contiguous bytes.  What differs is where the
// filter spectrum comes from.  There one 8 KB spectrum sits in LDS for the eight half-waves of a workgroup; here the two
// halves of a wave, and the eight half-waves of a workgroup, are in general on different channels, and the grid stride
// moves a half-wave to another channel with every segment.
//
// Form: ONE SPECTRUM IMAGE PER HALF-WAVE IN LDS, HALF A SPECTRUM EACH.  The taps are real, so H[1024 - k] = conj(H[k]):
// an image holds bins 0..512 (513 complex floats, 4.1 KB).  A lane reads bin k = l5 + 32 b (b = brev5(r), a literal after
// unrolling) as
//     b <  16:  image[k]                    lanes ascending, 256 contiguous bytes
//     b >= 16:  conj(image[1024 - k])       lanes descending, 256 contiguous bytes (b = 16, lane 0: bin 512 itself)
// The conjugate is the other cmul form (sign modifiers on the same FMAs), so the product costs what it costs in the shared
// kernel.  A ds_read_b64 serves a half-wave per pass, 32 lanes x 8 B over the 64 banks: 256 contiguous bytes meet every
// bank once whichever way the lanes run and wherever the image starts, so the mirrored reads add no conflict; the lanes
// need a second address register (ascending and descending base), which the kernel has.
// A half-wave refills its image when it starts a segment (16 jobs x 12 KB of stream per 4.1 KB of table: 0.2 % of the
// traffic, from L2 / Infinity Cache after the first touch).  The refill's loads are issued behind the segment's first
// job, which was requested one job earlier, so they wait for nothing that the job would not have waited for.  Only the
// half-wave itself reads and writes its image: no barrier, the LDS serves a wave's accesses in order.
// LDS per workgroup: 8 KB twiddles + 8 x 4.1 KB transpose buffers + 8 x 4.0 KB images = 73 KB, two workgroups per CU
// (146 of 160 KB) as in the shared kernel; whole 8 KB images would leave one.
//
// Forms measured against it or argued away (profiles/fir_bank/time_fir_bank.txt):
//   * every bin read from global memory (L2) per job, no image: the `bank_global_h` tune, k_fir_bank_ols_f32<true>.  32 more
//     loads in flight per lane and job on top of the 56 of the prefetch, and 8 KB of cache traffic per 12 KB of stream.
//   * a workgroup whose eight half-waves all work on one channel and share an 8 KB image: not built.  It needs two barriers
//     per channel change and ends the prefetch carried across segments at every one of them, which the shared kernel
//     measured at 3 % on the headline before any barrier cost (fir_ols.hip), and it idles seven half-waves wherever a
//     channel has fewer than eight segments (every batch of short frames).
#include "common.hpp"
#include "fft32.hpp"
#include "ols_walk.hpp"

namespace {

constexpr int BANK_BINS = LLZS_BANK_BINS;          // bins 0..512 of a channel's spectrum
constexpr int BANK_PITCH = LLZS_BANK_PITCH;        // complex floats per channel row of the device table
constexpr int BANK_IMG = 514;                      // complex floats per half-wave image in LDS
constexpr size_t BANK_LDS_COMMON = 1024 * sizeof(float2) + (size_t)OLS_WAVES * 2 * OLS_XBUF * sizeof(float);

// FFT -> multiply by the spectrum of this half-wave's channel -> IFFT.  h: bins 0..512 (LDS image or the channel's row in
// global memory); the upper half of the spectrum is the mirrored conjugate.
__device__ __forceinline__ void bank_filter(cf (&v)[32], cf (&u)[32], float *buf, const float2 *s_tw, const float2 *h, int l5,
                                            int col)
{
    ols_forward(v, buf, s_tw, l5, col);
    const float2 *up = h + l5, *dn = h - l5;
#pragma unroll
    for (int r = 0; r < 32; r++) {
        const int b = brev5(r);
        if (b < 16) {
            const float2 w = up[32 * b];
            u[b] = cmul<false>(v[r], cf{w.x, w.y});
        } else {
            const float2 w = dn[1024 - 32 * b];             // index 1024 - k >= 1
            u[b] = cmul<true>(v[r], cf{w.x, w.y});
        }
    }
    ols_inverse(u, buf, s_tw, l5, col);
}

// GLOBAL_H = false: the form described above.  true: the dropped form, kept for the A/B (tune bank_global_h).
template <bool GLOBAL_H>
__global__ void __launch_bounds__(OLS_THREADS, 2)
k_fir_bank_ols_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                   const float2 *__restrict__ hbank /* [channels][BANK_PITCH] */, const float2 *__restrict__ twid, ols_geom G)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *s_tw = reinterpret_cast<float2 *>(smem);                                      // [32][32] W_1024^(a*b)
    for (int i = threadIdx.x; i < 1024; i += OLS_THREADS) s_tw[i] = twid[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l5 = lane & 31;
    const ols_lane g = ols_lane_of(lane);
    const int slot = (threadIdx.x >> 6) * 2 + g.half;                                     // this half-wave in the workgroup
    float *buf = reinterpret_cast<float *>(s_tw + 1024) + slot * OLS_XBUF;                // its transpose buffer
    float2 *img = reinterpret_cast<float2 *>(smem + BANK_LDS_COMMON) + slot * BANK_IMG;   // its spectrum image
    const long halves_total = (long)gridDim.x * OLS_WAVES * 2;
    const long first = ((long)blockIdx.x * OLS_WAVES + wave) * 2;

    ols_seg cur[2] = {ols_locate(first, G), ols_locate(first + 1, G)};
    float halo[8];
    ols_raw raw;
    {
        const float *const row[2] = {in + (size_t)cur[0].c * G.in_pitch, in + (size_t)cur[1].c * G.in_pitch};
        const ols_seg own = g.half ? cur[1] : cur[0];
        ols_load_halo(halo, g.half ? row[1] : row[0], hist ? hist + (size_t)own.c * G.keep : nullptr, own.j0 * OLS_JOB,
                      g.col, G.keep, own.live);
        const int s0[2] = {cur[0].j0 * OLS_JOB, cur[1].j0 * OLS_JOB};
        const bool lv[2] = {cur[0].count > 0, cur[1].count > 0};
        ols_load(raw, row, s0, lv, g, G.n);
    }
    for (long sp = first; sp < G.total_segs; sp += halves_total) {
        const ols_seg nxt[2] = {ols_locate(sp + halves_total, G), ols_locate(sp + halves_total + 1, G)};
        const float *const row[2] = {in + (size_t)cur[0].c * G.in_pitch, in + (size_t)cur[1].c * G.in_pitch};
        float *const orow[2] = {out + (size_t)cur[0].c * G.out_pitch, out + (size_t)cur[1].c * G.out_pitch};
        const float *const nrow[2] = {in + (size_t)nxt[0].c * G.in_pitch, in + (size_t)nxt[1].c * G.in_pitch};
        const ols_seg nown = g.half ? nxt[1] : nxt[0];
        float halo_n[8];
#pragma unroll
        for (int i = 0; i < 8; i++) halo_n[i] = 0.f;

        // the spectrum of the channel this half-wave's segment belongs to (an idle half has none: nothing of it is stored)
        const ols_seg own = g.half ? cur[1] : cur[0];
        const float2 *hrow = hbank + (size_t)own.c * BANK_PITCH;
        if (!GLOBAL_H && own.live) {
#pragma unroll
            for (int i = 0; i < 16; i++) img[l5 + 32 * i] = hrow[l5 + 32 * i];
            if (l5 == 0) img[BANK_BINS - 1] = hrow[BANK_BINS - 1];
        }
        const float2 *h = GLOBAL_H ? hrow : img;

        const int jmax = max(cur[0].count, cur[1].count);
#pragma unroll 1
        for (int jj = 0; jj < jmax; jj++) {
            const int s[2] = {(cur[0].j0 + jj) * OLS_JOB, (cur[1].j0 + jj) * OLS_JOB};
            const bool live[2] = {jj < cur[0].count, jj < cur[1].count};
            cf v[32], u[32];
            ols_assemble(v, halo, raw);
            // next job of this segment pair, or (after the pair's last job) the first jobs and halos of the next pair.  A
            // half whose own segment has ended while its partner's has not requests nothing.
            const bool in_pair = jj + 1 < jmax;                                  // wave-uniform
            {
                const float *const lrow[2] = {in_pair ? row[0] : nrow[0], in_pair ? row[1] : nrow[1]};
                const int sn[2] = {in_pair ? s[0] + OLS_JOB : nxt[0].j0 * OLS_JOB,
                                   in_pair ? s[1] + OLS_JOB : nxt[1].j0 * OLS_JOB};
                const bool ln[2] = {in_pair ? jj + 1 < cur[0].count : nxt[0].count > 0,
                                    in_pair ? jj + 1 < cur[1].count : nxt[1].count > 0};
                ols_load(raw, lrow, sn, ln, g, G.n);
            }
            if (!in_pair)
                ols_load_halo(halo_n, g.half ? nrow[1] : nrow[0], hist ? hist + (size_t)nown.c * G.keep : nullptr,
                              nown.j0 * OLS_JOB, g.col, G.keep, nown.live);
            bank_filter(v, u, buf, s_tw, h, l5, g.col);
            ols_store(u, orow, s, live, g, G.n);
        }
        cur[0] = nxt[0];
        cur[1] = nxt[1];
#pragma unroll
        for (int i = 0; i < 8; i++) halo[i] = halo_n[i];
    }
}

// the plan is the shared 1024-point rung's (ols_plan_of): same job, same segments, same grid, same tunes
const ols_rung BANK_RUNGS[2] = {
    {1024, 1, "k_fir_bank_ols_f32", OLS_THREADS, 2 * OLS_WAVES, 2, true, 1.0,
     BANK_LDS_COMMON + (size_t)OLS_WAVES * 2 * BANK_IMG * sizeof(float2), false, false,
     1, {OLS_HALO}, {kfn(k_fir_bank_ols_f32<false>)}},
    {1024, 1, "k_fir_bank_ols_f32<global>", OLS_THREADS, 2 * OLS_WAVES, 2, true, 1.0,
     BANK_LDS_COMMON, false, false,
     1, {OLS_HALO}, {kfn(k_fir_bank_ols_f32<true>)}},
};

} // namespace

extern "C" int llzs_fir_bank_ols_f32(const float *hbank, const float *twid, const float *in, float *out, const float *hist,
                                     int channels, int n, long in_pitch, long out_pitch, int flt_len, void *stream)
{
    if (!hbank || !twid || !in || !out || channels <= 0 || n <= 0 || in_pitch < n || out_pitch < n) {
        llzs_set_error("fir_bank_ols_f32: bad arguments");
        return LLZ_ERR_ARG;
    }
    if (flt_len < 1 || flt_len - 1 > OLS_HALO) {
        llzs_set_error("fir_bank_ols_f32: flt_len %d outside 1..%d", flt_len, OLS_HALO + 1);
        return LLZ_ERR_RANGE;
    }
    const ols_rung &r = BANK_RUNGS[llzs_tune(LLZS_TUNE_BANK_GLOBAL_H) == 1 ? 1 : 0];
    ols_plan p = ols_plan_of(r, channels, n, in_pitch, out_pitch, flt_len);
    const float2 *hf = reinterpret_cast<const float2 *>(hbank), *tw = reinterpret_cast<const float2 *>(twid);
    void *args[6] = {&in, &out, &hist, &hf, &tw, &p.G};
    const void *kernel = r.kernel[0];
    if (r.lds_bytes > 64 * 1024)
        LLZ_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.lds_bytes));
    (void)hipLaunchKernel(kernel, dim3((unsigned)p.blocks), dim3(r.threads), args, r.lds_bytes, as_stream(stream));
    LLZ_LAUNCH_CHECK(r.name);
    return LLZ_OK;
}
