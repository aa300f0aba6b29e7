// ols_superblock.h -- the geometry of the super-block walk of the 1024-point overlap-save FIR (fir_ols.hip,
// k_fir_ols_chain_f32): which job and row of which sub-stream covers a sample, what a job requests from memory, what it
// stores, and how the carried rows travel from job to job.  No HIP includes: the kernel builds its steps from these
// functions, and a host program can run the same functions on sample indices instead of samples (tests/test_ols_superblock_host.py).
//
// A half-wave owns a SUPER-BLOCK: 16384 consecutive samples of one channel (64 KB), aligned to 64 KB from the row start.  It is
// two REGIONS of 8192 samples (32 KB); sub-stream A walks region 0 and sub-stream B region 1, side by side: job i transforms
// block i of region 0 as the real and block i of region 1 as the imaginary part of one complex 1024-point transform.  A block
// is 32 rows of 32 samples, lane `col` holds column `col` of every row.
//   jobs 0..9   window [768 i - 256, 768 i + 768) of the region: 8 carried rows + 24 requested rows, rows >= 8 stored
//   job 10      window [7168, 8192): rows 0..7 zero (no stored sample needs them), the 8 carried rows as rows 8..15, 16 requested
//               rows, rows >= 16 stored
// so a region is 10 2/3 blocks of 768 new samples in 11 transforms, and every stored sample has its 256 predecessors in its
// block.  At a super-block's start both sub-streams fetch their 256-sample halo: region 0's from the row (or the history at
// sample 0), region 1's is the tail of region 0 (requested twice: 2 KB per 64 KB).
#pragma once

#if defined(__HIPCC__)
#define OLS_SB_FN __host__ __device__ static inline
#define OLS_SB_UNROLL _Pragma("unroll")
#else
#define OLS_SB_FN static inline
#define OLS_SB_UNROLL
#endif

constexpr int OLS_SB_UNIT = 16384;                 // samples of a super-block
constexpr int OLS_SB_REGION = 8192;                // samples of a region: sub-stream B runs this far in front of A
constexpr int OLS_SB_ROW = 32;                     // samples of a row
constexpr int OLS_SB_HALO = 256;                   // the overlap: 8 rows
constexpr int OLS_SB_VALID = 768;                  // new samples of a full block: 24 rows
constexpr int OLS_SB_FULL_JOBS = 10;
constexpr int OLS_SB_JOBS = 11;                    // per super-block, the short one last
constexpr long OLS_SB_ALIGN = 32 * 1024;           // bytes: row bases and pitches the walk is taken for

// rows of a job's block in front of the requested ones (not stored) / requested from memory
OLS_SB_FN constexpr int ols_sb_carry_rows(int job) { return job < OLS_SB_FULL_JOBS ? 8 : 16; }
OLS_SB_FN constexpr int ols_sb_new_rows(int job) { return 32 - ols_sb_carry_rows(job); }
// first sample of the job's block, relative to its region's start (-256 for job 0: the halo)
OLS_SB_FN constexpr int ols_sb_window(int job)
{
    return job < OLS_SB_FULL_JOBS ? job * OLS_SB_VALID - OLS_SB_HALO : OLS_SB_REGION - 1024;
}
// first sample the job requests = first sample it stores: rows >= ols_sb_carry_rows(job) are both requested and stored
OLS_SB_FN constexpr int ols_sb_request(int job) { return ols_sb_window(job) + OLS_SB_ROW * ols_sb_carry_rows(job); }
// the job and the row of its block that store sample x (0..8191) of a region
OLS_SB_FN constexpr int ols_sb_job_of(int x) { return x < OLS_SB_FULL_JOBS * OLS_SB_VALID ? x / OLS_SB_VALID : OLS_SB_FULL_JOBS; }
OLS_SB_FN constexpr int ols_sb_row_of(int x) { return (x - ols_sb_window(ols_sb_job_of(x))) / OLS_SB_ROW; }

// ---- the plan: super-blocks of a call, channel-major ----
OLS_SB_FN constexpr int ols_sb_units_per_channel(int n) { return (n - 1) / OLS_SB_UNIT + 1; }
OLS_SB_FN constexpr long ols_sb_total(int channels, int n) { return (long)ols_sb_units_per_channel(n) * channels; }
// a super-block that lies inside the row entirely takes unclamped requests and unbounded stores
OLS_SB_FN constexpr bool ols_sb_whole(int unit_start, int n) { return unit_start <= n - OLS_SB_UNIT; }
// the walk is taken only for rows whose bases and pitches keep every region 32 KB-aligned
OLS_SB_FN bool ols_sb_aligned(const void *in, const void *out, long in_pitch, long out_pitch)
{
    return (unsigned long long)in % OLS_SB_ALIGN == 0 && (unsigned long long)out % OLS_SB_ALIGN == 0 &&
           in_pitch * 4 % OLS_SB_ALIGN == 0 && out_pitch * 4 % OLS_SB_ALIGN == 0;
}

// ---- what a lane reads for sample idx of a row of n samples ----
// a requested sample outside the row (a ragged last super-block, a dead region 1) or of an idle half-wave is zero; its
// address is clamped into the row
struct ols_sb_ref {
    int addr;                   // index into the row, always inside [0, n)
    bool use;                   // false: the sample is zero whatever the load returned
};
OLS_SB_FN ols_sb_ref ols_sb_sample(int idx, int n, bool live)
{
    ols_sb_ref r = {idx < n ? idx : n - 1, live && idx < n};
    return r;
}
// a halo sample: from the row, from the history (the previous call's last `keep` samples: index keep + idx) or zero
enum { OLS_SB_ZERO = 0, OLS_SB_FROM_ROW, OLS_SB_FROM_HIST };
struct ols_sb_href {
    int src, addr;
};
OLS_SB_FN ols_sb_href ols_sb_halo_sample(int idx, int n, int keep, bool live, bool has_hist)
{
    ols_sb_href r = {OLS_SB_ZERO, 0};
    if (live && idx < n) {
        if (idx >= 0) { r.src = OLS_SB_FROM_ROW; r.addr = idx; }
        else if (has_hist && idx >= -keep) { r.src = OLS_SB_FROM_HIST; r.addr = keep + idx; }
    }
    return r;
}

// ---- how the rows travel: V is a complex value (.x = sub-stream A, .y = sub-stream B), T a sample (or, on the host, a sample
// index); raw.a[r] / raw.b[r] = requested row r of A / B; halo[0..7] / halo[8..15] = the 8 rows in front of A's / B's next block
template <class V, class T, class RAW>
OLS_SB_FN void ols_sb_assemble_full(V (&v)[32], T (&halo)[16], const RAW &raw)
{
    OLS_SB_UNROLL
    for (int i = 0; i < 8; i++) {
        v[i].x = halo[i];
        v[i].y = halo[8 + i];
        halo[i] = raw.a[16 + i];                  // the next overlap of each sub-stream = its block's last 256
        halo[8 + i] = raw.b[16 + i];
    }
    OLS_SB_UNROLL
    for (int i = 0; i < 24; i++) {
        v[8 + i].x = raw.a[i];
        v[8 + i].y = raw.b[i];
    }
}
// the short job: its stored rows (>= 16) have their 256 predecessors in rows 8..15, which is the carried overlap as it stands
// after job 9 (samples 7424..7679 of the region); rows 0..7 of the window reach no stored sample and are zero.  halo is free
// afterwards.
template <class V, class T, class RAW>
OLS_SB_FN void ols_sb_assemble_short(V (&v)[32], const T (&halo)[16], const RAW &raw)
{
    OLS_SB_UNROLL
    for (int i = 0; i < 8; i++) {
        v[i].x = 0;
        v[i].y = 0;
        v[8 + i].x = halo[i];
        v[8 + i].y = halo[8 + i];
    }
    OLS_SB_UNROLL
    for (int i = 0; i < 16; i++) {
        v[16 + i].x = raw.a[i];
        v[16 + i].y = raw.b[i];
    }
}
