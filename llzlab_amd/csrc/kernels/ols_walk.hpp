// ols_walk.hpp -- the 1024-point overlap-save walk shared by fir_ols.hip (one tap set for every channel) and fir_bank.hip (a
// tap set per channel): the lane / segment geometry, the request, assemble, transform and store steps of a job, and the
// host-side launch plan.  fir_ols.hip describes the mapping.
#pragma once
#include "common.hpp"
#include "fft32.hpp"
#include "ols_superblock.h"

namespace {

constexpr int OLS_N = 1024;
constexpr int OLS_HALO = 256;                      // samples in front of a block: the overlap of the 1024-point rung
constexpr int OLS_VALID = OLS_N - OLS_HALO;        // 768
constexpr int OLS_JOB = 2 * OLS_VALID;             // 1536 new samples per complex transform
constexpr int OLS_WAVES = 4;
constexpr int OLS_THREADS = 64 * OLS_WAVES;
constexpr int OLS_SEG = 16;                        // jobs per segment at most (16 x 1536 samples of one channel)

// where a lane sits: which of the wave's two jobs it transforms and which column of the 32 x 32 decomposition it owns
struct ols_lane {
    int half, col;
};

__device__ __forceinline__ ols_lane ols_lane_of(int lane)
{
    ols_lane g;
    g.half = lane >> 5;
    g.col = lane & 31;
    return g;
}

// one segment of one half-wave: `count` consecutive jobs of channel c starting at job j0
struct ols_seg {
    bool live;
    int c, j0, count;
};

struct ols_geom {
    int n, keep, jobs_per_channel, segs_per_channel, seg_len;
    long total_segs, in_pitch, out_pitch;
};

__device__ __forceinline__ ols_seg ols_locate(long seg, const ols_geom &G)
{
    ols_seg g;
    g.live = seg < G.total_segs;
    g.c = g.live ? (int)(seg / G.segs_per_channel) : 0;
    g.j0 = g.live ? (int)(seg - (long)g.c * G.segs_per_channel) * G.seg_len : 0;
    g.count = g.live ? min(G.seg_len, G.jobs_per_channel - g.j0) : 0;
    return g;
}

// the 1536 new samples of a job, 48 registers per lane: a[r] / b[r] = row r of block A's / block B's new part, this
// lane's column
struct ols_raw {
    float a[24], b[24];
};

// request the 1536 new samples of the wave's two jobs (job h: row[h] + s[h], h = 0 lower / 1 upper half-wave); every
// lane takes its own job's column
__device__ __forceinline__ void ols_load(ols_raw &raw, const float *const (&row)[2], const int (&s)[2],
                                         const bool (&live)[2], const ols_lane &g, int n)
{
    const bool whole = live[0] && live[1] && s[0] + OLS_JOB <= n && s[1] + OLS_JOB <= n;   // wave-uniform
    const float *r = g.half ? row[1] : row[0];
    const int so = g.half ? s[1] : s[0];
    const bool lv = g.half ? live[1] : live[0];
    if (whole) {
#pragma unroll
        for (int i = 0; i < 24; i++) {
            raw.a[i] = __builtin_nontemporal_load(&r[so + 32 * i + g.col]);
            raw.b[i] = __builtin_nontemporal_load(&r[so + OLS_VALID + 32 * i + g.col]);
        }
    } else {
        // ragged last job of a row, or an idle half: addresses clamped into the row, samples outside [0, n) are zero
#pragma unroll
        for (int i = 0; i < 24; i++) {
            const int ia = so + 32 * i + g.col, ib = ia + OLS_VALID;
            const float xa = r[min(ia, n - 1)], xb = r[min(ib, n - 1)];
            raw.a[i] = (lv && ia < n) ? xa : 0.f;
            raw.b[i] = (lv && ib < n) ? xb : 0.f;
        }
    }
}

// the 256 samples in front of a segment, rows 0..7 of this lane's column: from the row (s > 0) or from the history
// (the previous call's last flt_len-1 samples) / zeros (s == 0)
__device__ __forceinline__ void ols_load_halo(float (&halo)[8], const float *row, const float *hrow, int s, int col,
                                              int keep, bool live)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int idx = s - OLS_HALO + 32 * i + col;
        float v = 0.f;
        if (live) {
            if (idx >= 0) v = row[idx];
            else if (hrow && idx >= -keep) v = hrow[keep + idx];
        }
        halo[i] = v;
    }
}

// The transform pair around the spectrum product, all in registers + one LDS transpose each way.  `col` is the lane's column
// n2 of the input / output decomposition n = 32 n1 + n2; between the transposes lane l5 owns bin row k1 = l5.
// forward: pass 1 over n1 (in registers), twiddle W^(k1 n2) + transpose, pass 2 over n2
// SKIP1: the twiddle row of ones is not multiplied with (transpose_twiddle)
template <bool SKIP1 = false>
__device__ __forceinline__ void ols_forward(cf (&v)[32], float *buf, const float2 *s_tw, int l5, int col)
{
    fft32<false>(v);
    transpose_twiddle<false, SKIP1>(v, buf, s_tw, col, l5);
    fft32<false>(v);                                        // v[r] = X[l5 + 32*brev5(r)]
}

// inverse, from bins in natural k2 order: pass over k2, conj twiddle + transpose, pass over k1
template <bool SKIP1 = false>
__device__ __forceinline__ void ols_inverse(cf (&u)[32], float *buf, const float2 *s_tw, int l5, int col)
{
    fft32<true>(u);
    transpose_twiddle<true, SKIP1>(u, buf, s_tw, l5, col);
    fft32<true>(u);                                         // u[r] = y[32*brev5(r) + col]
}

// FFT -> multiply by the filter spectrum s_h (1024 natural-order bins, the 1/1024 folded in) -> IFFT
// K > 0 (the 1024-point rung alone): the taps are symmetric about tap 32 K and s_h holds 1024 FLOATS, the real spectrum of the
// taps centred at index 0 (llz_shim.h, llzs_ols_tables) -- two multiplies per bin instead of a complex product, and the block
// comes out 32 K samples early: register row m is sample row m + K (ols_store, ols_sb_store).  Such a call also skips the
// product with the twiddle row of ones, which is the same bits on finite data.
template <int K = 0>
__device__ __forceinline__ void ols_filter(cf (&v)[32], cf (&u)[32], float *buf, const float2 *s_tw,
                                           const float2 *s_h, int l5, int col)
{
    ols_forward<(K > 0)>(v, buf, s_tw, l5, col);
    if constexpr (K > 0) {
        const float *s_g = reinterpret_cast<const float *>(s_h);
#pragma unroll
        for (int r = 0; r < 32; r++) {
            const float g = s_g[l5 + 32 * brev5(r)];
            u[brev5(r)] = cf{v[r].x * g, v[r].y * g};
        }
    } else {
#pragma unroll
        for (int r = 0; r < 32; r++) {
            const float2 h = s_h[l5 + 32 * brev5(r)];
            u[brev5(r)] = cmul<false>(v[r], cf{h.x, h.y});     // back to natural k2 order: renaming only
        }
    }
    ols_inverse<(K > 0)>(u, buf, s_tw, l5, col);
}

// keep the 768 valid samples of each block: sample rows n1 >= 8, in the order n1 = brev5(0), brev5(1), ...; sample row n1 is
// register row n1 - K
template <int K = 0>
__device__ __forceinline__ void ols_store(const cf (&u)[32], float *const (&orow)[2], const int (&s)[2],
                                          const bool (&live)[2], const ols_lane &g, int n)
{
    const bool whole = live[0] && live[1] && s[0] + OLS_JOB <= n && s[1] + OLS_JOB <= n;   // wave-uniform
    const bool lv = g.half ? live[1] : live[0];
    if (!lv) return;
    float *o = g.half ? orow[1] : orow[0];
    const int so = g.half ? s[1] : s[0];
    const int oa = so + g.col - OLS_HALO;                // + 32*n1
    const int ob = oa + OLS_VALID;
    if (whole) {
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int n1 = brev5(i), r = brev5((n1 - K) & 31);
            if (n1 >= 8) {
                __builtin_nontemporal_store(u[r].x, &o[oa + 32 * n1]);
                __builtin_nontemporal_store(u[r].y, &o[ob + 32 * n1]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int n1 = brev5(i), r = brev5((n1 - K) & 31);
            if (n1 >= 8) {
                if (oa + 32 * n1 < n) o[oa + 32 * n1] = u[r].x;
                if (ob + 32 * n1 < n) o[ob + 32 * n1] = u[r].y;
            }
        }
    }
}

// blocks A and B of a job from the carried overlap and the job's new samples; the new overlap is block B's last 256
__device__ __forceinline__ void ols_assemble(cf (&v)[32], float (&halo)[8], const ols_raw &raw)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i].x = halo[i];                         // block A [0,256)   = carried overlap
        v[i].y = raw.a[16 + i];                   // block B [0,256)   = block A [768,1024)
        halo[i] = raw.b[16 + i];                  // next overlap      = block B [768,1024)
    }
#pragma unroll
    for (int i = 0; i < 24; i++) {
        v[8 + i].x = raw.a[i];
        v[8 + i].y = raw.b[i];
    }
}

// ---- the super-block walk (ols_superblock.h has the geometry; fir_ols.hip's k_fir_ols_chain_f32 walks it) ----

// request ROWS rows of both sub-streams of the wave's two super-blocks: half h takes rows from sample s[h] of region 0 and
// from OLS_SB_REGION further on, the requests alternating between the two places.  whole (wave-uniform): both super-blocks lie
// inside their rows.
template <int ROWS>
__device__ __forceinline__ void ols_sb_load(ols_raw &raw, const float *const (&row)[2], const int (&s)[2], const bool (&live)[2],
                                            bool whole, const ols_lane &g, int n)
{
    const float *r = g.half ? row[1] : row[0];
    const int so = g.half ? s[1] : s[0];
    const bool lv = g.half ? live[1] : live[0];
    if (whole) {
        // one 64-bit address per sub-stream; the rows are 128 B apart and ride in the instructions' offsets (an int index per
        // request costs a sign extension and a 64-bit add every second load: LLZ_OLS_SB_INT_INDEX, the A/B form)
#ifdef LLZ_OLS_SB_INT_INDEX
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
            raw.a[i] = __builtin_nontemporal_load(&r[so + OLS_SB_ROW * i + g.col]);
            raw.b[i] = __builtin_nontemporal_load(&r[so + OLS_SB_REGION + OLS_SB_ROW * i + g.col]);
        }
#else
        const float *const pa = r + (so + g.col), *const pb = pa + OLS_SB_REGION;
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
            raw.a[i] = __builtin_nontemporal_load(&pa[OLS_SB_ROW * i]);
            raw.b[i] = __builtin_nontemporal_load(&pb[OLS_SB_ROW * i]);
        }
#endif
    } else {
        // a ragged last super-block (region 1 short or absent) or an idle half
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
            const int ia = so + OLS_SB_ROW * i + g.col;
            const ols_sb_ref ra = ols_sb_sample(ia, n, lv), rb = ols_sb_sample(ia + OLS_SB_REGION, n, lv);
            const float xa = r[ra.addr], xb = r[rb.addr];
            raw.a[i] = ra.use ? xa : 0.f;
            raw.b[i] = rb.use ? xb : 0.f;
        }
    }
}

// the 256 samples in front of both regions of the super-block at sample s: halo[0..7] region 0's (the row, or the history /
// zeros at s == 0), halo[8..15] region 1's (the tail of region 0)
__device__ __forceinline__ void ols_sb_load_halo(float (&halo)[16], const float *row, const float *hrow, int s, int col, int keep,
                                                 int n, bool live)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int idx = s - OLS_SB_HALO + OLS_SB_ROW * i + col;
        const ols_sb_href ha = ols_sb_halo_sample(idx, n, keep, live, hrow != nullptr);
        const ols_sb_href hb = ols_sb_halo_sample(idx + OLS_SB_REGION, n, keep, live, false);
        float va = 0.f, vb = 0.f;
        if (ha.src == OLS_SB_FROM_ROW) va = row[ha.addr];
        else if (ha.src == OLS_SB_FROM_HIST) va = hrow[ha.addr];
        if (hb.src == OLS_SB_FROM_ROW) vb = row[hb.addr];
        halo[i] = va;
        halo[8 + i] = vb;
    }
}

// keep the sample rows >= CARRY of both blocks (register rows >= CARRY - K: ols_filter); w[h] = the first sample of half h's
// block of region 0 (region 1's is OLS_SB_REGION on)
template <int CARRY, int K = 0>
__device__ __forceinline__ void ols_sb_store(const cf (&u)[32], float *const (&orow)[2], const int (&w)[2], const bool (&live)[2],
                                             bool whole, const ols_lane &g, int n)
{
    const bool lv = g.half ? live[1] : live[0];
    if (!lv) return;
    float *o = g.half ? orow[1] : orow[0];
    const int oa = (g.half ? w[1] : w[0]) + g.col;        // + 32*n1
    const int ob = oa + OLS_SB_REGION;
    if (whole) {
#ifdef LLZ_OLS_SB_INT_INDEX
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int n1 = brev5(i), r = brev5((n1 - K) & 31);
            if (n1 >= CARRY) {
                __builtin_nontemporal_store(u[r].x, &o[oa + OLS_SB_ROW * n1]);
                __builtin_nontemporal_store(u[r].y, &o[ob + OLS_SB_ROW * n1]);
            }
        }
#else
        float *const pa = o + oa, *const pb = pa + OLS_SB_REGION;          // as ols_sb_load: two addresses, the rows in the offsets
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int n1 = brev5(i), r = brev5((n1 - K) & 31);
            if (n1 >= CARRY) {
                __builtin_nontemporal_store(u[r].x, &pa[OLS_SB_ROW * n1]);
                __builtin_nontemporal_store(u[r].y, &pb[OLS_SB_ROW * n1]);
            }
        }
#endif
    } else {
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const int n1 = brev5(i), r = brev5((n1 - K) & 31);
            if (n1 >= CARRY) {
                if (oa + OLS_SB_ROW * n1 < n) o[oa + OLS_SB_ROW * n1] = u[r].x;
                if (ob + OLS_SB_ROW * n1 < n) o[ob + OLS_SB_ROW * n1] = u[r].y;
            }
        }
    }
}

// ---- launch plan (host) ----

// one overlap-save size: how its segments map onto workgroups, and the kernel instance built for each overlap
struct ols_rung {
    int nfft, min_taps;
    const char *name;
    int threads;                // per workgroup
    int segs_per_wg;            // segments a workgroup walks at once: half-waves (1024), waves (2048, 4096), wave pairs (8192)
    int wg_per_cu;              // resident workgroups per CU the grid is sized for (256 CUs)
    bool tuned;                 // the ols_wg_per_cu and ols_seg_len tune knobs apply
    double startup;             // segment-length cost: rounds x (length + startup)
    size_t lds_bytes;
    bool w2k, w4k;              // the kernel takes W_2048^n / W_4096^n
    int count;                  // overlaps instantiated, ascending: the launch takes the smallest that holds flt_len - 1
    int overlap[8];
    const void *kernel[8];
};

template <typename K> static const void *kfn(K k) { return reinterpret_cast<const void *>(k); }

struct ols_plan {
    int instance;               // index into the rung's overlaps
    long blocks, max_blocks;    // workgroups launched; one resident set
    bool large;                 // the batch fills the machine with full-length segments
    ols_geom G;
};

// the geometry of one call, on the host alone; flt_len is within the rung's range
static ols_plan ols_plan_of(const ols_rung &r, int channels, int n, long in_pitch, long out_pitch, int flt_len)
{
    ols_plan p;
    p.instance = 0;
    while (r.overlap[p.instance] < flt_len - 1) p.instance++;
    const int job = 2 * (r.nfft - r.overlap[p.instance]);     // new samples per transform: two blocks of nfft - overlap
    ols_geom &G = p.G;
    G.n = n;
    G.keep = flt_len - 1;
    G.in_pitch = in_pitch;
    G.out_pitch = out_pitch;
    G.jobs_per_channel = (n + job - 1) / job;
    // one resident set of workgroups, grid stride over the segments
    const int tuned_per_cu = r.tuned ? llzs_tune(LLZS_TUNE_OLS_WG_PER_CU) : -1;
    const long max_blocks = 256L * (tuned_per_cu > 0 ? tuned_per_cu : r.wg_per_cu);
    const long slots = max_blocks * r.segs_per_wg;
    // jobs per segment: a segment walks seg_len consecutive jobs of one channel (the overlap stays in registers), at most
    // OLS_SEG.  Small batches (BASELINE config 2: 64 channels) would leave segment slots idle or quantise badly into rounds
    // with the full length, so they take the length that minimises the cost in rounds.  Large batches keep the full length:
    // on 4096 channels a shorter segment measured 2.6 % slower (1024 points).
    int seg_len = OLS_SEG;
    p.max_blocks = max_blocks;
    p.large = (long)((G.jobs_per_channel + OLS_SEG - 1) / OLS_SEG) * channels >= 4 * slots;
    if (!p.large) {
        double best = 1e300;
        for (int sl = OLS_SEG; sl >= 1; sl--) {
            const long segs = (long)((G.jobs_per_channel + sl - 1) / sl) * channels;
            const double cost = (double)((segs + slots - 1) / slots) * (sl + r.startup);
            if (cost < best * 0.999) { best = cost; seg_len = sl; }
        }
    }
    if (r.tuned)
        if (const int v = llzs_tune(LLZS_TUNE_OLS_SEG_LEN); v >= 1 && v <= 1024) seg_len = v;
    G.seg_len = seg_len;
    G.segs_per_channel = (G.jobs_per_channel + seg_len - 1) / seg_len;
    G.total_segs = (long)G.segs_per_channel * channels;
    p.blocks = (G.total_segs + r.segs_per_wg - 1) / r.segs_per_wg;
    if (p.blocks > max_blocks) p.blocks = max_blocks;
    return p;
}

} // namespace
