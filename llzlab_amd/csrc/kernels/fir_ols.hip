// fir_ols.hip -- K4 / K4b: overlap-save FIR with register FFTs that never leave the CU.
//   k_fir_ols_chain_f32      up to 257 taps   1024-point transforms, a half-wave per job (described first, below;
//   k_fir_ols_seg_f32                         the super-block walk and the segment walk)
//   k_fir_ols2k_chain_f32<O> up to 1025 taps  2048-point transforms, a whole wave per job (one radix-2 step over the half-waves)
//   k_fir_ols4k_f32<O>       up to 3073 taps  4096-point transforms, a whole wave per job (two radix-2 steps)
//   k_fir_ols8k_f32<O>       up to 6145 taps  8192-point transforms, a pair of waves per job (one more radix-2 step, across the pair)
//
// New functionality relative to the reference (llz_fir.c is time-domain only); its end-to-end
// oracle is the time-domain llz_fir_filter (llz_fir.c:547-584), its FFT stage follows the sign/scale
// convention of llz_fft.c:61-130,142-198 (forward e^{-j}, unscaled; inverse e^{+j}, divided by N -- the 1/N is
// folded into the filter spectrum on the host).
//
// Why: 257 taps in the time domain is 514 flop per 8 B of HBM traffic -> VALU-bound at ~30 % of the HBM roofline.
// Overlap-save costs ~46 vector lane-operations per sample and is HBM-bound.
//
// Mapping to CDNA4 (wave64):
//   * job = one channel x 1536 new samples.  Two 1024-sample blocks (each: 256 overlap + 768 new) are
//     the real and imaginary part of ONE complex 1024-point transform -- the filter is real, so
//     IFFT(FFT(xa + j xb) H) = ya + j yb and nothing has to be untangled.
//   * a half-wave (32 lanes) owns a job: 1024 = 32 x 32, every lane keeps 32 complex values in registers.  A
//     transform is two passes of 32-point in-register FFTs (fft32.hpp) with one 32 x 32 transpose through LDS
//     between them (row pitch 33 floats).  Forward leaves bins digit-reversed in the register index, which is
//     free (register renaming), so FFT -> multiply by H -> IFFT needs no permutation pass at all.
//   * the walk, large batches of 32 KB-aligned rows (the headline; k_fir_ols_chain_f32, geometry in ols_superblock.h): a half-wave
//     owns a SUPER-BLOCK of 16384 consecutive samples of one channel (64 KB, aligned to 64 KB) as two 32 KB regions walked
//     side by side -- the real part of a transform is a block of region 0, the imaginary part the same block of region 1,
//     so the half-wave's requests alternate between two 32 KB-aligned runs exactly 32 KB apart.  One 256-sample overlap per
//     sub-stream is carried in registers from job to job; a region is 10 2/3 blocks of 768 new samples, so the 11th job of a
//     super-block is short (16 requested rows; its window ends at the region's end).  The next job's samples are requested
//     (into registers) before the current job is transformed, across super-blocks as well: the short job requests job 0 and
//     both halos of the half-wave's next super-block.  Region 1's halo is the tail of region 0: 2 KB per 64 KB are requested
//     twice, and 11 transforms do the work of 10 2/3.
//   * the walk, everything else (k_fir_ols_seg_f32; fir_bank.hip walks the same way): a half-wave walks a SEGMENT of up to 16
//     consecutive jobs of one channel -- a job is two CONSECUTIVE blocks, 1536 new samples -- with one carried overlap and the
//     same chain across segments; every input sample is requested exactly once.  Small batches take the segment length that
//     fills the machine (ols_plan_of), which 64 KB units cannot.
//     Why two walks: how fast this memory system streams depends on the length and the alignment of the run a half-wave reads
//     before it jumps (profiles/r02/ubench_walk_pairs.txt, ubench_walk_substreams.txt: two sub-streams exactly 32 KB apart copy
//     7..11 % faster than one 96 KB run, sub-streams at any distance that is no multiple of 16 KB slower than both).  Segments
//     are 96 KB at a 96 KB stride: never aligned, and no whole number of 6 KB jobs makes 32 KB.  The copy stand-in of both
//     shapes (tools/ubench/ols_io.hip sb, profiles/r04/ubench_ols_io_superblock.txt): 5.80 against 5.57 TB/s; the kernel:
//     6.28 against 6.40 ms on the headline, same box, alternating (profiles/r04/ab_ols_superblock.txt).
//   * the spectrum product, template parameter K of both 1024-point kernels (ols_filter<K>, ols_walk.hpp).  K = 0: the complex
//     product with DFT(taps) / 1024.  K = 1..4: taps that mirror bit for bit about tap c = 32 K (65, 129, 193, 257 taps: every
//     filter of such a length the library designs, the headline's among them) are centred at index 0 on the host, where their
//     spectrum is REAL (llzs_ols_tables.hreal: 1024 floats, the first 4 KB of the spectrum's LDS slot; the other 4 KB stay
//     unused): two multiplies and one ds_read_b32 per bin instead of a complex product and a ds_read_b64, and the block comes out
//     c samples early -- register row m is sample row m + K, the stores keep sample rows >= 8 (>= 16 in the short job) as
//     before, same addresses in the same order.  Valid because the circular product is the linear one for p in [c, 1023 - c],
//     i.e. for samples 2c..1023 of the block, and 2c <= 256.  Such a call also leaves register 0 out of the inter-pass twiddle
//     (transpose_twiddle<INV, true>: row 0 of W_1024^(ab) is all ones; the same bits on finite data).  The host decides K from
//     the float taps at init (llz_host_ols_real_rows), the launcher takes it per call (ols_real_rows; the ols_real_product tune:
//     0 = complex).  The transform block of the steady-state job: 1948 -> 1847 vector ALU instructions per wave and job.
//   * addresses of the super-block walk's requests and stores: one 64-bit address per sub-stream and job, the 24 rows (128 B
//     apart) in the instructions' offsets: 4 vector ALU instructions in the request block instead of 50 (a sign extension and
//     a 64-bit add every second load).  Same loads and stores, same order, same non-temporal hints.
//     Both together, parent against this, bench.py alternating on one box (profiles/headline_diet/ab_headline.txt): 6.47..6.50
//     -> 6.24..6.27 ms per step, ratio 0.963, on a second box 6.38..6.39 -> 6.10..6.14, ratio 0.960, every run of the one below
//     every run of the other; there, each part on its own: without the real product 6.28..6.29, without the addresses
//     6.19..6.21.  The instruction counts per block: profiles/headline_diet/isa_counts.txt (tools/isa_counts.py).
//   * not done: the 48 + 16 register copies at the back edge of the ten-job loop (the prefetched rows and the carried overlaps
//     moved to the registers the next iteration reads).  Requests are issued before the transform, so a request set's
//     registers must differ from the 64 the transform still reads; two sets that swap roles (five iterations of two jobs)
//     take the 48 x 2 copies of the rows that are used once away, but a row that is also the next job's overlap lives through
//     three requests, and ten jobs are no multiple of three: that loop compiles to 40 copies per two jobs, 254 VGPRs and
//     66 KB of code against 48 KB, and 6.12..6.13 ms against 6.10..6.14 without it on the second box: no gain, not kept.
//   * known and deliberately left alone: in the compiled job loop an s_waitcnt vmcnt(0) follows the prefetch requests directly,
//     before the transform's first instruction, so a wave does not overlap its own prefetch with its own transform; the other
//     wave of the SIMD does.  A third wave to hide that wait changed nothing (profiles/r02/ab_ols_no_prefetch_three_waves.txt).
//   * HBM access shape: one dword per lane, a half-wave instruction moves 128 contiguous bytes of its job.  Wider shapes
//     were built and measured and do not pay (profiles/r02/): a copy kernel in exactly this walk structure runs at the same
//     rate with 4, 8 or 16 bytes per lane (6.04 / 6.02 / 6.02 ms for 32 GiB), and an 8-byte form of this kernel (512
//     contiguous bytes per wave instruction, samples handed to their lanes by v_permlane16/32_swap transposes, commit
//     cda1552) was 7 % slower: the 96 extra vector instructions per job pair cost more than the shorter request stream saves.
//   * per workgroup (4 waves): LDS = 8 KB inter-pass twiddles W_1024^(a*b) + 8 KB filter spectrum + 8 x 4.1 KB
//     transpose buffers = 49 KB; two workgroups per CU (the prefetch registers allow two waves per SIMD).
// HBM traffic: 4 B read + 4 B written per sample; the super-block walk's halo re-reads measure +0.4 % (PMC:
// profiles/pmc_traffic.json, profiles/r04/rocprof_headline_before_after.txt).
// The steps of the 1024-point walk (geometry, request, assemble, transform, store) and the launch plan live in ols_walk.hpp:
// fir_bank.hip walks the same way with a spectrum per channel.
#include <stdlib.h>
#include "common.hpp"
#include "fft32.hpp"
#include "ols_walk.hpp"

namespace {

constexpr int OLS_OVERLAP = 256;                   // the 1024-point rung's overlap, as OLS_RUNGS names it
static_assert(OLS_OVERLAP == OLS_HALO, "ols_walk.hpp carries the same overlap");

struct ols_smem {
    float2 *tw, *h;
    float *buf;
};

// K > 0: hfreq is the real table (1024 floats, llzs_ols_tables.hreal), which takes the first half of the spectrum's 8 KB
template <int K>
__device__ __forceinline__ ols_smem ols_tables(char *smem, const float2 *__restrict__ hfreq, const float2 *__restrict__ twid)
{
    ols_smem m;
    m.tw = reinterpret_cast<float2 *>(smem);                 // [32][32]  W_1024^(a*b)
    m.h = m.tw + 1024;                                        // [1024]    FFT(taps)/1024, natural bins
    for (int i = threadIdx.x; i < 1024; i += OLS_THREADS) {
        m.tw[i] = twid[i];
        if constexpr (K > 0) reinterpret_cast<float *>(m.h)[i] = reinterpret_cast<const float *>(hfreq)[i];
        else m.h[i] = hfreq[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, half = (threadIdx.x >> 5) & 1;
    m.buf = reinterpret_cast<float *>(m.h + 1024) + (wave * 2 + half) * OLS_XBUF;     // per half-wave transpose buffer
    return m;
}

// The segment walk (small batches, rows or pitches that are not 32 KB-aligned; fir_bank.hip walks the same way).
// A half-wave runs one segment after the other (grid stride over segment pairs), with the prefetch carried ACROSS segments: the
// last job of a segment requests the first job and the halo of the half-wave's NEXT segment, so every load is used and no
// segment start waits on memory (a first form requested past the segment's end and discarded the data: 1/16 of the input
// fetched twice, 3 % slower on the headline; it was also slower on batches of a single round: 0.21 against 0.13 ms on 64
// channels x 63 taps).  Both halves of a wave step through their segments together (a segment that is short at the end of a
// channel idles its tail).  K: the spectrum product (ols_filter), 0 = complex.
template <int K>
__global__ void __launch_bounds__(OLS_THREADS, 2)
k_fir_ols_seg_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                    const float2 *__restrict__ hfreq, const float2 *__restrict__ twid, ols_geom G)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ols_smem S = ols_tables<K>(smem, hfreq, twid);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l5 = lane & 31;
    const ols_lane g = ols_lane_of(lane);
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
            ols_filter<K>(v, u, S.buf, S.tw, S.h, l5, g.col);
            ols_store<K>(u, orow, s, live, g, G.n);
        }
        cur[0] = nxt[0];
        cur[1] = nxt[1];
#pragma unroll
        for (int i = 0; i < 8; i++) halo[i] = halo_n[i];
    }
}

// The headline form: the SUPER-BLOCK walk (ols_superblock.h).  A half-wave owns 16384 consecutive samples of a channel, 64 KB
// aligned to 64 KB, as two 32 KB regions walked side by side: the real part of a transform is a block of region 0, the imaginary
// part the same block of region 1 (the two blocks packed into one complex transform can come from anywhere), so the half-wave's
// request stream is two sub-streams exactly 32 KB apart, each a 32 KB-aligned run of 32 KB -- the shape the walk-copy
// micro-benchmarks single out (profiles/r02/ubench_walk_substreams.txt, profiles/r04/ubench_ols_io_superblock.txt); the segment
// walk's runs are 96 KB at a 96 KB stride, never aligned.  11 jobs per super-block: ten full ones in one loop (8 carried + 24
// requested rows per sub-stream), then the short one, peeled (8 carried + 16 requested rows, 16 stored: a region is 10 2/3 blocks).  Two
// carried overlaps, one per sub-stream.  The chain across units is the segment walk's: the short job requests job 0 and both
// halos of the half-wave's next super-block; both halves of a wave step together; a ragged last super-block of a row runs all
// 11 jobs on clamped requests and bounded stores (a dead region 1 is an all-zero imaginary part).  The launcher takes this
// form only where rows and pitches keep the regions 32 KB-aligned and the batch fills the machine (ols_sb_applies).
template <int K>
__global__ void __launch_bounds__(OLS_THREADS, 2)
k_fir_ols_chain_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                    const float2 *__restrict__ hfreq, const float2 *__restrict__ twid, ols_geom G /* a segment = a super-block */)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ols_smem S = ols_tables<K>(smem, hfreq, twid);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l5 = lane & 31;
    const ols_lane g = ols_lane_of(lane);
    const long halves_total = (long)gridDim.x * OLS_WAVES * 2;
    const long first = ((long)blockIdx.x * OLS_WAVES + wave) * 2;

    ols_seg cur[2] = {ols_locate(first, G), ols_locate(first + 1, G)};           // j0 = the super-block's index in its channel
    float halo[16];
    ols_raw raw;
    {
        const float *const row[2] = {in + (size_t)cur[0].c * G.in_pitch, in + (size_t)cur[1].c * G.in_pitch};
        const ols_seg own = g.half ? cur[1] : cur[0];
        ols_sb_load_halo(halo, g.half ? row[1] : row[0], hist ? hist + (size_t)own.c * G.keep : nullptr, own.j0 * OLS_SB_UNIT,
                         g.col, G.keep, G.n, own.live);
        const int s0[2] = {cur[0].j0 * OLS_SB_UNIT, cur[1].j0 * OLS_SB_UNIT};
        const bool lv[2] = {cur[0].live, cur[1].live};
        ols_sb_load<24>(raw, row, s0, lv, lv[0] && lv[1] && ols_sb_whole(s0[0], G.n) && ols_sb_whole(s0[1], G.n), g, G.n);
    }
    for (long sp = first; sp < G.total_segs; sp += halves_total) {
        const ols_seg nxt[2] = {ols_locate(sp + halves_total, G), ols_locate(sp + halves_total + 1, G)};
        const float *const row[2] = {in + (size_t)cur[0].c * G.in_pitch, in + (size_t)cur[1].c * G.in_pitch};
        float *const orow[2] = {out + (size_t)cur[0].c * G.out_pitch, out + (size_t)cur[1].c * G.out_pitch};
        const int s[2] = {cur[0].j0 * OLS_SB_UNIT, cur[1].j0 * OLS_SB_UNIT};
        const bool live[2] = {cur[0].live, cur[1].live};
        const bool whole = live[0] && live[1] && ols_sb_whole(s[0], G.n) && ols_sb_whole(s[1], G.n);   // wave-uniform

#pragma unroll 1
        for (int jj = 0; jj < OLS_SB_FULL_JOBS; jj++) {
            cf v[32], u[32];
            ols_sb_assemble_full(v, halo, raw);
            // the next job of this super-block pair: a full one, or -- after job 9 -- the short one's 16 rows
            const int sn[2] = {s[0] + ols_sb_request(jj + 1), s[1] + ols_sb_request(jj + 1)};
            if (jj + 1 < OLS_SB_FULL_JOBS) ols_sb_load<24>(raw, row, sn, live, whole, g, G.n);
            else ols_sb_load<16>(raw, row, sn, live, whole, g, G.n);
            ols_filter<K>(v, u, S.buf, S.tw, S.h, l5, g.col);
            const int w[2] = {s[0] + ols_sb_window(jj), s[1] + ols_sb_window(jj)};
            ols_sb_store<8, K>(u, orow, w, live, whole, g, G.n);
        }
        {
            cf v[32], u[32];
            ols_sb_assemble_short(v, halo, raw);
            // job 0 and both halos of the half-wave's next super-block (an idle half requests nothing it uses)
            const float *const nrow[2] = {in + (size_t)nxt[0].c * G.in_pitch, in + (size_t)nxt[1].c * G.in_pitch};
            const ols_seg nown = g.half ? nxt[1] : nxt[0];
            const int sn[2] = {nxt[0].j0 * OLS_SB_UNIT, nxt[1].j0 * OLS_SB_UNIT};
            const bool ln[2] = {nxt[0].live, nxt[1].live};
            ols_sb_load<24>(raw, nrow, sn, ln, ln[0] && ln[1] && ols_sb_whole(sn[0], G.n) && ols_sb_whole(sn[1], G.n), g, G.n);
            ols_sb_load_halo(halo, g.half ? nrow[1] : nrow[0], hist ? hist + (size_t)nown.c * G.keep : nullptr, g.half ? sn[1] : sn[0],
                             g.col, G.keep, G.n, nown.live);
            ols_filter<K>(v, u, S.buf, S.tw, S.h, l5, g.col);
            const int w[2] = {s[0] + ols_sb_window(OLS_SB_FULL_JOBS), s[1] + ols_sb_window(OLS_SB_FULL_JOBS)};
            ols_sb_store<16, K>(u, orow, w, live, whole, g, G.n);
        }
        cur[0] = nxt[0];
        cur[1] = nxt[1];
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// 258 .. 1025 taps: the same walk on 2048-point transforms, a WHOLE WAVE per job.
//
// A 2048-point transform held by one half-wave needs 64 complex registers per lane and spills (round 1's kernel of that
// shape: 12.4 ms at 513 taps, 17 ms at 1025).  Here one radix-2 step splits it over the wave's two half-waves, each of which then runs the
// 1024-point machinery above unchanged:
//     forward (decimation in frequency):  X[2k]   = FFT_1024( a[n] + a[n+1024] )            -> lower half-wave
//                                         X[2k+1] = FFT_1024( (a[n] - a[n+1024]) W_2048^n ) -> upper half-wave
//     inverse (decimation in time):       y[n], y[n+1024] = S'[n] +- W_2048^-n D'[n],   S' / D' = the halves' inverse transforms
// A block is 64 rows of 32 samples; lane (half h, l5) owns the rows of parity h (2p + h, p < 32) at column l5, so rows p
// and p + 16 of a lane are 1024 samples apart: the butterflies are in-lane, and ONE v_permlane32_swap per register pair
// then hands all sums to the lower and all differences to the upper half-wave (and back after the inverse transforms).
// Because a row's parity survives the walk's shifts (the 512-sample overlap is 16 rows, a block advances by 48 rows), the
// carried overlap stays in the lane that needs it, and ols_assemble / ols_raw are the 1024-point kernel's.  Lower and upper
// lanes load adjacent rows: a wave instruction moves 256 contiguous bytes.  Job = two blocks (real / imaginary part) =
// 3072 new samples of one channel.
// Template parameter O = the overlap: 512 samples (16 rows, up to 513 taps, 1536 new samples per block) or 1024 (32 rows,
// up to 1025 taps, 1024 new samples per block).

template <int O>
__global__ void __launch_bounds__(OLS_THREADS, 2)
k_fir_ols2k_chain_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                     const float2 *__restrict__ hfreq2 /* [2][1024]: even bins, odd bins, / 2048 */,
                     const float2 *__restrict__ twid /* [32][32] W_1024^(ab) */, const float2 *__restrict__ tw2k /* [1024] W_2048^n */,
                     ols_geom G)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *s_tw = reinterpret_cast<float2 *>(smem);           // [1024]
    float2 *s_h = s_tw + 1024;                                  // [2][1024]
    float2 *s_w = s_h + 2048;                                   // [1024]
    for (int i = threadIdx.x; i < 1024; i += OLS_THREADS) {
        s_tw[i] = twid[i];
        s_h[i] = hfreq2[i];
        s_h[1024 + i] = hfreq2[1024 + i];
        s_w[i] = tw2k[i];
    }
    __syncthreads();
    constexpr int O2K_OVERLAP = O, O2K_VALID = 2048 - O, O2K_JOB = 2 * O2K_VALID;
    constexpr int HP = O / 64, NEW = 32 - HP;                       // a lane's carried and new rows per block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, l5 = lane & 31;
    float *buf = reinterpret_cast<float *>(s_w + 1024) + (wave * 2 + half) * OLS_XBUF;
    const float2 *my_h = s_h + half * 1024;
    const long waves_total = (long)gridDim.x * OLS_WAVES;
    const int rowoff = 32 * half + l5;                              // this lane inside a pair of rows

    // segment -> (channel row, first job, job count); a wave past the last segment gets an empty one
    struct segd { const float *row; float *orow; const float *hrow; int j0, count; };
    auto locate = [&](long seg) {
        segd d;
        const bool live = seg < G.total_segs;
        const int c = live ? (int)(seg / G.segs_per_channel) : 0;
        d.j0 = live ? (int)(seg - (long)c * G.segs_per_channel) * G.seg_len : 0;
        d.count = live ? min(G.seg_len, G.jobs_per_channel - d.j0) : 0;
        d.row = in + (size_t)c * G.in_pitch;
        d.orow = out + (size_t)c * G.out_pitch;
        d.hrow = hist ? hist + (size_t)c * G.keep : nullptr;
        return d;
    };
    const int n = G.n;
    // rows 2i + h (i < HP) in front of a segment: from the row, the history or zeros
    auto load_halo = [&](float (&halo)[HP], const segd &d) {
#pragma unroll
        for (int i = 0; i < HP; i++) {
            const int idx = d.j0 * O2K_JOB - O2K_OVERLAP + 64 * i + rowoff;
            float v = 0.f;
            if (d.count > 0) {
                if (idx >= 0) v = d.row[idx];
                else if (d.hrow && idx >= -G.keep) v = d.hrow[G.keep + idx];
            }
            halo[i] = v;
        }
    };
    ols_raw raw;
    auto load = [&](const float *row, int s, bool live) {          // the new samples of the job at s: 2 NEW per lane
        if (live && s + O2K_JOB <= n) {
#pragma unroll
            for (int i = 0; i < NEW; i++) {
                raw.a[i] = __builtin_nontemporal_load(&row[s + 64 * i + rowoff]);
                raw.b[i] = __builtin_nontemporal_load(&row[s + O2K_VALID + 64 * i + rowoff]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NEW; i++) {
                const int ia = s + 64 * i + rowoff, ib = ia + O2K_VALID;
                const float xa = row[min(ia, n - 1)], xb = row[min(ib, n - 1)];
                raw.a[i] = (live && ia < n) ? xa : 0.f;
                raw.b[i] = (live && ib < n) ? xb : 0.f;
            }
        }
    };

    long seg = (long)blockIdx.x * OLS_WAVES + wave;
    segd cur = locate(seg);
    float halo[HP];
    load_halo(halo, cur);
    load(cur.row, cur.j0 * O2K_JOB, cur.count > 0);
    for (; seg < G.total_segs; seg += waves_total) {
        const segd nxt = locate(seg + waves_total);
        float halo_n[HP];
#pragma unroll
        for (int i = 0; i < HP; i++) halo_n[i] = 0.f;
#pragma unroll 1
        for (int jj = 0; jj < cur.count; jj++) {
            const int s = (cur.j0 + jj) * O2K_JOB;
            const float *row = cur.row;
            float *orow = cur.orow;
            cf v[32], u[32];
            // v[p] = row 2p + h of blocks A (re) and B (im): block A's first HP positions are the carried overlap, block B's
            // are block A's last HP; the new overlap is block B's last HP
#pragma unroll
            for (int i = 0; i < HP; i++) {
                v[i].x = halo[i];
                v[i].y = raw.a[NEW - HP + i];
                halo[i] = raw.b[NEW - HP + i];
            }
#pragma unroll
            for (int i = 0; i < NEW; i++) {
                v[HP + i].x = raw.a[i];
                v[HP + i].y = raw.b[i];
            }
            // the next job of this segment, or -- after its last job -- the first job and the halo of the wave's next segment
            const bool in_seg = jj + 1 < cur.count;                  // wave-uniform
            load(in_seg ? row : nxt.row, in_seg ? s + O2K_JOB : nxt.j0 * O2K_JOB, in_seg || nxt.count > 0);
            if (!in_seg) load_halo(halo_n, nxt);
            // ---- radix-2 step down: rows p and p + 16 are 1024 samples apart.  Every lane twiddles the differences of its
            // own 16 rows BEFORE they move to the upper half-wave (half the multiplies the upper lanes alone would need)
            cf w[32];
#pragma unroll
            for (int p = 0; p < 16; p++) {
                cf sm = cadd(v[p], v[p + 16]);
                const float2 t = s_w[64 * p + rowoff];              // W_2048^n, n = 32 (2p + h) + l5
                cf df = cmul<false>(csub(v[p], v[p + 16]), cf{t.x, t.y});
                swap32(sm.x, df.x);                                 // lower: (s_2p, s_2p+1)   upper: (d_2p, d_2p+1)
                swap32(sm.y, df.y);
                w[2 * p] = sm;
                w[2 * p + 1] = df;
            }
            // ---- 1024 points per half-wave: forward, spectrum product, inverse
            ols_filter(w, u, buf, s_tw, my_h, l5, l5);              // u[r] = S' or D' at row brev5(r)
            // ---- radix-2 step up and the stores of the valid rows (positions >= HP)
            const bool whole = s + O2K_JOB <= n;
            const int oa = s - O2K_OVERLAP + rowoff, ob = oa + O2K_VALID;
#pragma unroll
            for (int p = 0; p < 16; p++) {
                cf P = u[brev5(2 * p)], Q = u[brev5(2 * p + 1)];
                swap32(P.x, Q.x);                                   // lower: (S_2p, D_2p)   upper: (S_2p+1, D_2p+1)
                swap32(P.y, Q.y);
                const float2 t = s_w[64 * p + rowoff];
                Q = cmul<true>(Q, cf{t.x, t.y});                    // W_2048^-n on the lane's own 16 differences
                const cf y0 = cadd(P, Q), y1 = csub(P, Q);          // rows 2p + h and 2p + h + 32 = positions p, p + 16
                if (whole) {
                    if (p >= HP) {
                        __builtin_nontemporal_store(y0.x, &orow[oa + 64 * p]);
                        __builtin_nontemporal_store(y0.y, &orow[ob + 64 * p]);
                    }
                    __builtin_nontemporal_store(y1.x, &orow[oa + 64 * (p + 16)]);
                    __builtin_nontemporal_store(y1.y, &orow[ob + 64 * (p + 16)]);
                } else {
                    if (p >= HP) {
                        if (oa + 64 * p < n) orow[oa + 64 * p] = y0.x;
                        if (ob + 64 * p < n) orow[ob + 64 * p] = y0.y;
                    }
                    if (oa + 64 * (p + 16) < n) orow[oa + 64 * (p + 16)] = y1.x;
                    if (ob + 64 * (p + 16) < n) orow[ob + 64 * (p + 16)] = y1.y;
                }
            }
        }
        cur = nxt;
#pragma unroll
        for (int i = 0; i < HP; i++) halo[i] = halo_n[i];
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// 514 .. 3073 taps: 4096-point transforms, again a whole wave per job, as radix-2 step + TWO 2048-point problems run one
// after the other through the split above (each of them: radix-2 step + a 1024-point transform per half-wave).
//     X[2k] = FFT_2048( a[n] + a[n+2048] ),   X[2k+1] = FFT_2048( (a[n] - a[n+2048]) W_4096^n );   back: E'[n] +- W_4096^-n O'[n]
// A block is 128 rows of 32 samples, a lane owns the 64 rows of its parity (positions p: row 2p + h), rows p and p + 32 are
// 2048 samples apart (in-lane butterflies).  The overlap O is 512 / 1024 / 2048 / 3072 samples by tap count (positions
// below O / 64 of a lane; with 2048 only the "minus" half of the last step is ever stored).  64 complex values per lane leave
// no room for a register prefetch or a carried overlap: a job's new dwords and those of block A's overlap (an L2 hit: the
// same wave read them one job ago) are requested when the job starts, and the second wave of the SIMD covers the wait.  A
// workgroup is 8 waves (one per CU: the four spectra planes, three twiddle tables and sixteen transpose buffers are 132 KB
// of LDS).
//
// The spectrum is split four ways: plane j = 2 half + sub holds H[4m + j] / 4096 (sub 0 = the even-bin problem E, 1 = the
// odd-bin problem O; inside a problem the lower half-wave has its even bins, the upper its odd bins).
// the lane id, formed afresh where it is needed: what the phases of a job derive from it (buffer addresses, the lane's twiddle)
// then lives inside that phase only -- carried across the 4096-point problem, which needs every register there is, each of
// them is a spill
__device__ __forceinline__ int o8k_lane()
{
    int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(l));
    return l;
}
constexpr int O4K_WAVES = 8, O4K_THREADS = 64 * O4K_WAVES;

// one 2048-point problem of the wave: v[p] = row 2p + h (p < 32) in, y[p] out (same ownership); see k_fir_ols2k_chain_f32
template <int WS = 1>                                                 // WS = 2: s_w is the W_4096^n table (every other entry)
__device__ __forceinline__ void ols2k_core(cf (&v)[32], cf (&y)[32], float *buf, const float2 *s_tw, const float2 *my_h,
                                           const float2 *s_w, int l5, int rowoff)
{
    cf w[32], u[32];
#pragma unroll
    for (int p = 0; p < 16; p++) {
        cf sm = cadd(v[p], v[p + 16]);
        const float2 t = s_w[WS * (64 * p + rowoff)];
        cf df = cmul<false>(csub(v[p], v[p + 16]), cf{t.x, t.y});
        swap32(sm.x, df.x);
        swap32(sm.y, df.y);
        w[2 * p] = sm;
        w[2 * p + 1] = df;
    }
    ols_filter(w, u, buf, s_tw, my_h, l5, l5);
#pragma unroll
    for (int p = 0; p < 16; p++) {
        cf P = u[brev5(2 * p)], Q = u[brev5(2 * p + 1)];
        swap32(P.x, Q.x);
        swap32(P.y, Q.y);
        const float2 t = s_w[WS * (64 * p + rowoff)];
        Q = cmul<true>(Q, cf{t.x, t.y});
        y[p] = cadd(P, Q);
        y[p + 16] = csub(P, Q);
    }
}

// O = overlap, a multiple of 64 that holds flt_len - 1 samples (512, 768, 1024, 1536, 2048, 2560, 3072); a job is two blocks =
// 2 (4096 - O) new samples.
// Lane position i (0..63) of a block is sample 64 i + rowoff; positions below O / 64 are overlap.
template <int O>
__global__ void __launch_bounds__(O4K_THREADS, 2)
k_fir_ols4k_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                const float2 *__restrict__ hfreq4 /* [4][1024] */, const float2 *__restrict__ twid /* [32][32] W_1024^(ab) */,
                const float2 *__restrict__ tw2k /* [1024] W_2048^n */, const float2 *__restrict__ tw4k /* [2048] W_4096^n */,
                ols_geom G)
{
    constexpr int V = 4096 - O, JOB = 2 * V, PO = O / 64, PV = V / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *s_tw = reinterpret_cast<float2 *>(smem);           // [1024]
    float2 *s_w2 = s_tw + 1024;                                 // [1024]
    float2 *s_w4 = s_w2 + 1024;                                 // [2048]
    float2 *s_h = s_w4 + 2048;                                  // [4][1024]
    for (int i = threadIdx.x; i < 1024; i += O4K_THREADS) {
        s_tw[i] = twid[i];
        s_w2[i] = tw2k[i];
        s_w4[i] = tw4k[i];
        s_w4[1024 + i] = tw4k[1024 + i];
#pragma unroll
        for (int j = 0; j < 4; j++) s_h[1024 * j + i] = hfreq4[1024 * j + i];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *s_buf = reinterpret_cast<float *>(s_h + 4096);
    const long waves_total = (long)gridDim.x * O4K_WAVES;
    const int n = G.n;

    for (long seg = (long)blockIdx.x * O4K_WAVES + wave; seg < G.total_segs; seg += waves_total) {
        const int c = (int)(seg / G.segs_per_channel);
        const int j0 = (int)(seg - (long)c * G.segs_per_channel) * G.seg_len;
        const int count = min(G.seg_len, G.jobs_per_channel - j0);
        const float *row = in + (size_t)c * G.in_pitch;
        float *orow = out + (size_t)c * G.out_pitch;
        const float *hrow = hist ? hist + (size_t)c * G.keep : nullptr;
#pragma unroll 1
        for (int jj = 0; jj < count; jj++) {
            const int s = (j0 + jj) * JOB;
            // block A (real parts) = [s - O, s + V), block B (imaginary parts) = [s + V - O, s + 2V).  Block A's overlap was
            // read by this wave one job ago: it is read again (from L2) rather than carried -- 32 more registers would spill.
            // Block B's first O samples are block A's last O.
            cf v[64];
            const bool whole = s >= O && s + JOB <= n;
            {
            const int rowoff = o8k_lane();
            if (whole) {
#pragma unroll
                for (int i = 0; i < PO; i++) v[i].x = row[s - O + 64 * i + rowoff];
#pragma unroll
                for (int i = PO; i < 64; i++) v[i].x = __builtin_nontemporal_load(&row[s - O + 64 * i + rowoff]);
#pragma unroll
                for (int i = PO; i < 64; i++) v[i].y = __builtin_nontemporal_load(&row[s + V - O + 64 * i + rowoff]);
            } else {
#pragma unroll
                for (int i = 0; i < 64; i++) {
                    const int ia = s - O + 64 * i + rowoff;
                    float xa = 0.f;
                    if (ia >= 0) xa = row[min(ia, n - 1)];
                    else if (hrow && ia >= -G.keep) xa = hrow[G.keep + ia];
                    v[i].x = ia < n ? xa : 0.f;
                }
#pragma unroll
                for (int i = PO; i < 64; i++) {
                    const int ib = s + V - O + 64 * i + rowoff;
                    const float xb = row[min(ib, n - 1)];
                    v[i].y = ib < n ? xb : 0.f;
                }
            }
            }
#pragma unroll
            for (int i = 0; i < PO; i++) v[i].y = v[i + PV].x;
            const int rowoff = o8k_lane(), half = rowoff >> 5, l5 = rowoff & 31;
            float *buf = s_buf + (wave * 2 + half) * OLS_XBUF;
            // ---- radix-2 step down: positions p and p + 32 are 2048 samples apart
            cf e[32], o[32];
#pragma unroll
            for (int p = 0; p < 32; p++) {
                e[p] = cadd(v[p], v[p + 32]);
                const float2 t = s_w4[64 * p + rowoff];             // W_4096^n, n = 32 (2p + h) + l5
                o[p] = cmul<false>(csub(v[p], v[p + 32]), cf{t.x, t.y});
            }
            // ---- the even-bin and the odd-bin 2048-point problems, one after the other
            cf ye[32], yo[32];
            ols2k_core(e, ye, buf, s_tw, s_h + (2 * half) * 1024, s_w2, l5, rowoff);
            ols2k_core(o, yo, buf, s_tw, s_h + (2 * half + 1) * 1024, s_w2, l5, rowoff);
            // ---- radix-2 step up: position p = E' + W^-n O', position p + 32 = E' - W^-n O'; positions >= O / 64 are outputs
            const bool all_out = s + JOB <= n;
#pragma unroll
            for (int p = 0; p < 32; p++) {
                if (p + 32 < PO) continue;
                const float2 t = s_w4[64 * p + rowoff];
                const cf q = cmul<true>(yo[p], cf{t.x, t.y});
                if (p >= PO) {
                    const cf y0 = cadd(ye[p], q);
                    const int oa = s + 64 * (p - PO) + rowoff, ob = oa + V;
                    if (all_out) {
                        __builtin_nontemporal_store(y0.x, &orow[oa]);
                        __builtin_nontemporal_store(y0.y, &orow[ob]);
                    } else {
                        if (oa < n) orow[oa] = y0.x;
                        if (ob < n) orow[ob] = y0.y;
                    }
                }
                const cf y1 = csub(ye[p], q);
                const int oa = s + 64 * (p + 32 - PO) + rowoff, ob = oa + V;
                if (all_out) {
                    __builtin_nontemporal_store(y1.x, &orow[oa]);
                    __builtin_nontemporal_store(y1.y, &orow[ob]);
                } else {
                    if (oa < n) orow[oa] = y1.x;
                    if (ob < n) orow[ob] = y1.y;
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// 2 .. 6145 taps (the library's choice from 1026 on): 8192-point transforms on a PAIR of waves.  With 3072 samples of overlap a 4096-point block yields 1024
// outputs (25 % of the transform), an 8192-point block 5120 (62.5 %) at 13/12 of the work per point.
//     X[2k] = FFT_4096( a[n] + a[n+4096] )  -> wave 0 of the pair,     X[2k+1] = FFT_4096( (a[n] - a[n+4096]) W_8192^n )  -> wave 1,
// each wave then runs the 4096-point problem of k_fir_ols4k_f32 (radix-2 step + two 2048-point problems); back:
// y[n] = E'[n] + W_8192^-n O'[n], y[n+4096] = E'[n] - W_8192^-n O'[n].
// A block is 128 rows of 64 samples (position i = samples 64 i + lane).  Wave w requests positions 32w .. 32w+31 and the
// same + 64 of both blocks (64 complex values per lane, as the 4096-point kernel), forms its 32 sums and 32 twiddled
// differences, and the two waves SWAP halves through LDS: wave 0 gives its differences for wave 1's sums.  On the way back
// wave 1 twiddles its results, the waves swap halves again and each forms and stores the outputs among "its" 64 positions.
// W_8192^(64 i + lane) = W_128^i (a literal after unrolling) x W_8192^lane (a 512-byte LDS table, read where it is used): no
// 32 KB table, and nothing lane-derived is carried across the 4096-point problem (o8k_lane()).
// Wave 1 keeps the two halves of its register array exchanged (slot j = position j + 32 mod 64), so that both waves keep slots
// 0..31 and swap slots 32..63 through one code path; the 4096-point problem is indifferent to it.
//
// The swap goes through the transpose buffers the two waves own anyway (8.25 KB per wave: two rounds of 16 values per lane),
// and the pair synchronises on four LDS words of its own instead of a workgroup barrier, so that the four pairs of a workgroup
// drift apart and one pair's memory wait is another's arithmetic -- a barrier would hold all eight waves in the same phase
// (64 complex values per lane leave no registers for a prefetch).  The pair is the two waves of ONE SIMD (waves p, p + 4): a
// wave that waits for its partner leaves the SIMD to exactly that partner.  Both waves of a pair run the same loop bounds, hence the
// same number of rounds; the waits are bounded (a pair out of step would produce wrong samples, which the tests see, never
// a hang).  LDS: W_1024^(ab) 8 KB, W_4096^n 16 KB (W_2048^n = every other entry), spectrum 8 x 8 KB, buffers 66 KB = 154 KB.
// O8K_TRACE (a measurement build only): shader-clock time of each phase of a job, summed per wave (tools/trace_ols8k.py)
#ifdef O8K_TRACE
__device__ unsigned long long o8k_trace_buf[2048 * 8];
#define O8K_T0() unsigned long long o8_t = __builtin_readcyclecounter(), o8_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define O8K_MARK(i) do { const unsigned long long now = __builtin_readcyclecounter(); o8_acc[i] += now - o8_t; o8_t = now; } while (0)
#define O8K_PIN(x) asm volatile("s_nop 0" ::"v"(x))
#define O8K_DUMP() do { if ((threadIdx.x & 63) == 0) { const unsigned wv_ = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & 2047u; \
    for (int i = 0; i < 8; i++) o8k_trace_buf[wv_ * 8 + i] = o8_acc[i]; } } while (0)
#else
#define O8K_T0() do { } while (0)
#define O8K_MARK(i) do { } while (0)
#define O8K_PIN(x) do { } while (0)
#define O8K_DUMP() do { } while (0)
#endif
struct w128_tab {
    float c[64], s[64];
};
constexpr double o8k_sin(double x)
{
    double term = x, sum = x;
    for (int k = 1; k < 16; k++) {
        term *= -x * x / (double)((2 * k) * (2 * k + 1));
        sum += term;
    }
    return sum;
}
constexpr double o8k_cos(double x)
{
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 16; k++) {
        term *= -x * x / (double)((2 * k - 1) * (2 * k));
        sum += term;
    }
    return sum;
}
constexpr w128_tab o8k_make_w128()
{
    w128_tab t{};
    for (int j = 0; j < 64; j++) {
        const double a = 3.14159265358979323846 * (double)j / 64.0;
        t.c[j] = j == 32 ? 0.f : (float)o8k_cos(a);
        t.s[j] = j == 0 ? 0.f : (float)o8k_sin(a);
    }
    return t;
}
__device__ constexpr w128_tab kW128 = o8k_make_w128();          // W_128^j = c[j] - i s[j]

constexpr int O8K_WAVES = 8, O8K_THREADS = 64 * O8K_WAVES, O8K_PAIRS = O8K_WAVES / 2;
#ifndef O8K_SPIN
#define O8K_SPIN (1 << 18)                 // (A/B builds: -DO8K_SPIN=0 takes the waiting out, with wrong samples)
#endif
constexpr int O8K_SPIN_LIMIT = O8K_SPIN;

typedef __attribute__((address_space(3))) volatile int *o8k_flag_p;          // 32-bit LDS addresses: generic pointers in the
typedef float o8k_f2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) o8k_f2 *o8k_box_p;                 // struct would become 64-bit flat accesses
struct o8k_pair {
    o8k_flag_p my_free, my_sent, pt_free, pt_sent;             // round counters, one writer each
    o8k_box_p my_box, pt_box;                                   // [16][64]: the wave's own transpose buffers (wave-uniform bases)
    int k;
};
__device__ __forceinline__ void o8k_signal(o8k_flag_p flag, int k)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // what this wave wrote / read before is done
    *flag = k;
}
__device__ __forceinline__ void o8k_wait(o8k_flag_p flag, int k)
{
    int spins = 0;
    while (__builtin_amdgcn_readfirstlane(*flag) < k && ++spins < O8K_SPIN_LIMIT) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
// the wave hands a[OFF .. OFF+31] to its partner and takes the partner's 32 values in their place
template <int OFF>
__device__ __forceinline__ void o8k_swap(cf (&a)[64], o8k_pair &ps)
{
    const int lane = o8k_lane();
    const o8k_box_p mine = ps.my_box + lane, theirs = ps.pt_box + lane;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        ps.k++;
        o8k_signal(ps.my_free, ps.k);                           // my buffers may take round k
        o8k_wait(ps.pt_free, ps.k);
#pragma unroll
        for (int i = 0; i < 16; i++) theirs[64 * i] = (o8k_f2){a[OFF + 16 * r + i].x, a[OFF + 16 * r + i].y};
        o8k_signal(ps.my_sent, ps.k);
        o8k_wait(ps.pt_sent, ps.k);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const o8k_f2 t = mine[64 * i];
            a[OFF + 16 * r + i] = cf{t[0], t[1]};
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the buffers go back to the transposes
}

// the 4096-point problem of one wave, in place: a[p] = position p (sample 64 p + lane of the 4096) in and out; h_e / h_o = the
// spectrum planes of its even-bin and odd-bin 2048-point problems for this half-wave
__device__ __forceinline__ void ols4k_core(cf (&a)[64], float *buf, const float2 *s_tw, const float2 *s_w4, const float2 *h_e,
                                           const float2 *h_o, int l5, int rowoff)
{
    cf e[32], o[32];
#pragma unroll
    for (int p = 0; p < 32; p++) {
        e[p] = cadd(a[p], a[p + 32]);
        const float2 t = s_w4[64 * p + rowoff];
        o[p] = cmul<false>(csub(a[p], a[p + 32]), cf{t.x, t.y});
    }
    cf ye[32], yo[32];
    ols2k_core<2>(e, ye, buf, s_tw, h_e, s_w4, l5, rowoff);
    ols2k_core<2>(o, yo, buf, s_tw, h_o, s_w4, l5, rowoff);
#pragma unroll
    for (int p = 0; p < 32; p++) {
        const float2 t = s_w4[64 * p + rowoff];
        const cf q = cmul<true>(yo[p], cf{t.x, t.y});
        a[p] = cadd(ye[p], q);
        a[p + 32] = csub(ye[p], q);
    }
}

// O = overlap, a multiple of 64 with flt_len - 1 <= O <= 6144; a job is two blocks = 2 (8192 - O) new samples of one channel
// (beyond 4096 block B starts in front of the row for the first job: the history serves it too, and rows 64 .. O/64 - 1 of a
// block are overlap as well)
template <int O>
__global__ void __launch_bounds__(O8K_THREADS, 2)
k_fir_ols8k_f32(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ hist,
                const float2 *__restrict__ hfreq8 /* [8][1024] */, const float2 *__restrict__ twid /* [32][32] W_1024^(ab) */,
                const float2 *__restrict__ tw4k /* [2048] W_4096^n */, ols_geom G)
{
    constexpr int V = 8192 - O, JOB = 2 * V, PO = O / 64;
    static_assert(O % 64 == 0 && O <= 6144, "at least 2048 new samples per block");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *s_tw = reinterpret_cast<float2 *>(smem);           // [1024]
    float2 *s_w4 = s_tw + 1024;                                 // [2048]
    float2 *s_h = s_w4 + 2048;                                  // [8][1024]
    float *s_buf = reinterpret_cast<float *>(s_h + 8192);       // [16][OLS_XBUF]
    int *s_flag = reinterpret_cast<int *>(s_buf + 2 * O8K_WAVES * OLS_XBUF);                      // [8][2]
    float2 *s_wl = reinterpret_cast<float2 *>(s_flag + 2 * O8K_WAVES);                            // [64] W_8192^lane
    for (int i = threadIdx.x; i < 1024; i += O8K_THREADS) {
        s_tw[i] = twid[i];
        s_w4[i] = tw4k[i];
        s_w4[1024 + i] = tw4k[1024 + i];
#pragma unroll
        for (int j = 0; j < 8; j++) s_h[1024 * j + i] = hfreq8[1024 * j + i];
    }
    if (threadIdx.x < 2 * O8K_WAVES) s_flag[threadIdx.x] = 0;
    if (threadIdx.x < 64) {
        float sn, cs;
        sincospif((float)threadIdx.x * (1.0f / 4096.0f), &sn, &cs);
        s_wl[threadIdx.x] = make_float2(cs, -sn);
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the pair = waves p and p + 4 of the workgroup: the two waves of ONE SIMD.  Whenever one of them waits for the other, the
    // other is the wave its SIMD runs, so the waits cost no issue slots anybody wanted; with neighbouring waves (two SIMDs)
    // a waiting wave leaves its SIMD to a wave of another pair, which may be waiting as well (12.23 against 11.42 ms at 3073
    // taps, same box: -DO8K_CROSS_SIMD)
#ifdef O8K_CROSS_SIMD
    const int w = wave & 1, pair = wave >> 1, partner = wave ^ 1;
#else
    const int w = wave >> 2, pair = wave & 3, partner = wave ^ 4;
#endif
    o8k_pair ps;
    ps.my_free = (o8k_flag_p)(s_flag + 2 * wave);
    ps.my_sent = (o8k_flag_p)(s_flag + 2 * wave + 1);
    ps.pt_free = (o8k_flag_p)(s_flag + 2 * partner);
    ps.pt_sent = (o8k_flag_p)(s_flag + 2 * partner + 1);
    ps.my_box = (o8k_box_p)(reinterpret_cast<o8k_f2 *>(s_buf + (wave * 2) * OLS_XBUF));
    ps.pt_box = (o8k_box_p)(reinterpret_cast<o8k_f2 *>(s_buf + (partner * 2) * OLS_XBUF));
    ps.k = 0;
    O8K_T0();
    const long pairs_total = (long)gridDim.x * O8K_PAIRS;
    const int n = G.n;
    const int pos0 = 32 * w;

    for (long seg = (long)blockIdx.x * O8K_PAIRS + pair; seg < G.total_segs; seg += pairs_total) {
        const int c = (int)(seg / G.segs_per_channel);
        const int j0 = (int)(seg - (long)c * G.segs_per_channel) * G.seg_len;
        const int count = min(G.seg_len, G.jobs_per_channel - j0);
        const float *row = in + (size_t)c * G.in_pitch;
        float *orow = out + (size_t)c * G.out_pitch;
        const float *hrow = hist ? hist + (size_t)c * G.keep : nullptr;
#pragma unroll 1
        for (int jj = 0; jj < count; jj++) {
            const int s = (j0 + jj) * JOB;
            // block A (real parts) = [s - O, s + V), block B (imaginary parts) = [s + V - O, s + 2V): B's first O samples are
            // A's last O, the same addresses (requested again: cache hits, the other wave may hold them)
            O8K_MARK(6);                                                 // loop overhead
            cf a[64];
            const bool whole = s >= O && s + JOB <= n;
            if (whole) {
                const float *ra = row + s - O + 64 * pos0 + o8k_lane(), *rb = ra + V;
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    a[j].x = __builtin_nontemporal_load(&ra[64 * j]);
                    a[32 + j].x = __builtin_nontemporal_load(&ra[64 * (j + 64)]);
                }
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    a[j].y = __builtin_nontemporal_load(&rb[64 * j]);
                    a[32 + j].y = __builtin_nontemporal_load(&rb[64 * (j + 64)]);
                }
            } else {
                const int lane = o8k_lane();
#pragma unroll
                for (int j = 0; j < 64; j++) {
                    const int pos = pos0 + (j < 32 ? j : j + 32);
                    const int ia = s - O + 64 * pos + lane, ib = ia + V;
                    float xa = 0.f;
                    if (ia >= 0) xa = row[min(ia, n - 1)];
                    else if (hrow && ia >= -G.keep) xa = hrow[G.keep + ia];
                    a[j].x = ia < n ? xa : 0.f;
                    float xb;
                    if (O > 4096 && ib < 0) xb = (hrow && ib >= -G.keep) ? hrow[G.keep + ib] : 0.f;
                    else xb = row[min(ib, n - 1)];
                    a[j].y = ib < n ? xb : 0.f;
                }
            }
            O8K_PIN(a[0].x); O8K_PIN(a[63].y); O8K_PIN(a[31].y); O8K_PIN(a[32].x);
            O8K_MARK(0);                                                 // requests, awaited
            // ---- radix-2 step down over the wave's 32 positions.  Wave 1 works with the halves of its arrays exchanged (slot j =
            // position j + 32 mod 64), so that BOTH waves keep slots 0..31 and swap slots 32..63 (one code path, no register
            // shuffles where two would join): the 4096-point problem is indifferent to it -- exchanged input halves flip the
            // sign of its odd-bin branch, which exchanges the output halves the same way.
            // (the twiddles are formed where they are used: hoisted out of the job loop they would be 192 more live registers)
            const float2 wd = s_wl[o8k_lane()];                          // W_8192^lane, times W_128^(32 w) = (-i)^w
            const cf wv = w ? cf{wd.y, -wd.x} : cf{wd.x, wd.y};
#pragma unroll
            for (int j = 0; j < 32; j++) {
                const cf sm = cadd(a[j], a[32 + j]), df = csub(a[j], a[32 + j]);
                const cf t = cmul<false>(cf{kW128.c[j], -kW128.s[j]}, wv);
                const cf dt = cmul<false>(df, t);
                a[j] = w ? dt : sm;                                      // kept: wave 0 its sums (positions 0..31), wave 1 its
                a[32 + j] = w ? sm : dt;                                 // differences (positions 32..63); the other 32 go over
            }
            O8K_PIN(a[0].x); O8K_PIN(a[63].y);
            O8K_MARK(1);                                                 // step down
            o8k_swap<32>(a, ps);
            O8K_PIN(a[32].x); O8K_PIN(a[63].y);
            O8K_MARK(2);                                                 // swap
            {
                const int ln = o8k_lane(), hf = ln >> 5;
                ols4k_core(a, s_buf + (wave * 2 + hf) * OLS_XBUF, s_tw, s_w4, s_h + (4 * hf + w) * 1024, s_h + (4 * hf + 2 + w) * 1024,
                           ln & 31, ln);
            }
            O8K_PIN(a[0].x); O8K_PIN(a[63].y); O8K_PIN(a[32].x);
            O8K_MARK(3);                                                 // the 4096-point problem
            // ---- back: wave 1 turns its results by W_8192^-n (slot j = position j + 32 mod 64), gives the 32 of positions 0..31
            // for wave 0's E' of positions 32..63, and position 32 w + j gets E' + q, position 32 w + j + 64 gets E' - q
            if (w) {
                const float2 wr = s_wl[o8k_lane()];
                const cf wu = cf{wr.x, wr.y};
#pragma unroll
                for (int p = 0; p < 64; p++) {
                    const cf t = cmul<false>(cf{kW128.c[p ^ 32], -kW128.s[p ^ 32]}, wu);
                    a[p] = cmul<true>(a[p], t);
                }
            }
            o8k_swap<32>(a, ps);
            O8K_PIN(a[32].x); O8K_PIN(a[63].y); O8K_PIN(a[0].x);
            O8K_MARK(4);                                                 // turn + swap
            const float sg = w ? -1.f : 1.f;                             // wave 0: a[j] = E', a[32 + j] = q; wave 1: the reverse
            const int lane = o8k_lane();
            const bool all_out = s + JOB <= n;
            const int jmin = PO - pos0;                                  // positions below PO are overlap
            float *oa0 = orow + s + 64 * (pos0 - PO) + lane;
#pragma unroll
            for (int j = 0; j < 32; j++) {
                const cf y0 = cadd(a[j], a[32 + j]), d1 = csub(a[j], a[32 + j]);
                const cf y1 = cf{d1.x * sg, d1.y * sg};
                const int oa = s + 64 * (pos0 + j - PO) + lane, ob = oa + V;
                if (all_out) {
                    if (j >= jmin) {
                        __builtin_nontemporal_store(y0.x, &oa0[64 * j]);
                        __builtin_nontemporal_store(y0.y, &oa0[64 * j + V]);
                    }
                    if (PO <= 64 || j >= jmin - 64) {
                        __builtin_nontemporal_store(y1.x, &oa0[64 * (j + 64)]);
                        __builtin_nontemporal_store(y1.y, &oa0[64 * (j + 64) + V]);
                    }
                } else {
                    if (j >= jmin) {
                        if (oa < n) orow[oa] = y0.x;
                        if (ob < n) orow[ob] = y0.y;
                    }
                    if (PO <= 64 || j >= jmin - 64) {
                        if (oa + 4096 < n) orow[oa + 4096] = y1.x;
                        if (ob + 4096 < n) orow[ob + 4096] = y1.y;
                    }
                }
            }
            O8K_MARK(5);                                                 // outputs formed, stores issued
#ifdef O8K_TRACE
            o8_acc[7]++;
#endif
        }
    }
    O8K_DUMP();
}

// ---- launch: every transform size is one row of OLS_RUNGS ----

const ols_rung OLS_RUNGS[] = {
    // two workgroups per CU: 49 KB of LDS and ~240 registers per lane
    {1024, 1, "k_fir_ols_f32", OLS_THREADS, 2 * OLS_WAVES, 2, true, 1.0,
     2 * 1024 * sizeof(float2) + (size_t)OLS_WAVES * 2 * OLS_XBUF * sizeof(float), false, false,
     1, {OLS_OVERLAP}, {kfn(k_fir_ols_seg_f32<0>)}},
    {2048, 2, "k_fir_ols2k_chain_f32", OLS_THREADS, OLS_WAVES, 2, false, 1.0,
     4 * 1024 * sizeof(float2) + (size_t)OLS_WAVES * 2 * OLS_XBUF * sizeof(float), true, false,
     2, {512, 1024}, {kfn(k_fir_ols2k_chain_f32<512>), kfn(k_fir_ols2k_chain_f32<1024>)}},
    // one 8-wave workgroup per CU
    {4096, 2, "k_fir_ols4k_f32", O4K_THREADS, O4K_WAVES, 1, false, 0.0,
     8 * 1024 * sizeof(float2) + (size_t)O4K_WAVES * 2 * OLS_XBUF * sizeof(float), true, true,
     7, {512, 768, 1024, 1536, 2048, 2560, 3072},
     {kfn(k_fir_ols4k_f32<512>), kfn(k_fir_ols4k_f32<768>), kfn(k_fir_ols4k_f32<1024>), kfn(k_fir_ols4k_f32<1536>),
      kfn(k_fir_ols4k_f32<2048>), kfn(k_fir_ols4k_f32<2560>), kfn(k_fir_ols4k_f32<3072>)}},
    // (a job costs 27 .. 31 us whatever the overlap between 2048 and 2560 -- 10.96 / 10.92 / 10.90 ms for 2048 / 2304 / 2560 on
    // the headline batch -- so the ladder is coarse there)
    {8192, 2, "k_fir_ols8k_f32", O8K_THREADS, O8K_PAIRS, 1, false, 0.0,
     (1024 + 2048 + 8192) * sizeof(float2) + (size_t)O8K_WAVES * 2 * OLS_XBUF * sizeof(float) + 2 * O8K_WAVES * sizeof(int) +
         64 * sizeof(float2), false, true,
     8, {1536, 2304, 2560, 3072, 3584, 4096, 5120, 6144},
     {kfn(k_fir_ols8k_f32<1536>), kfn(k_fir_ols8k_f32<2304>), kfn(k_fir_ols8k_f32<2560>), kfn(k_fir_ols8k_f32<3072>),
      kfn(k_fir_ols8k_f32<3584>), kfn(k_fir_ols8k_f32<4096>), kfn(k_fir_ols8k_f32<5120>), kfn(k_fir_ols8k_f32<6144>)}},
};

// The super-block walk is taken where it can be aligned and can fill the machine: row bases and pitches that are multiples of
// 32 KB, and a batch large by the test that keeps the segment walk at its full segment length (small batches -- BASELINE config
// 2 -- quantise badly into 64 KB units).  The ols_superblock tune: unset = this choice, 1 = also on small batches (never without
// the alignment), 0 = the segment walk.  An ols_seg_len tune asks for the segment walk as well.
bool ols_sb_applies(const ols_plan &p, const float *in, const float *out, long in_pitch, long out_pitch, int n)
{
    const int t = llzs_tune(LLZS_TUNE_OLS_SUPERBLOCK);
    if (t == 0 || !ols_sb_aligned(in, out, in_pitch, out_pitch) || n > INT32_MAX - 2 * OLS_SB_UNIT) return false;
    return t == 1 || (p.large && llzs_tune(LLZS_TUNE_OLS_SEG_LEN) < 0);
}

// a "segment" of the geometry becomes a super-block: one per ols_locate, numbered channel-major
void ols_sb_plan(ols_plan &p, int channels, int n)
{
    ols_geom &G = p.G;
    G.seg_len = 1;
    G.jobs_per_channel = G.segs_per_channel = ols_sb_units_per_channel(n);
    G.total_segs = ols_sb_total(channels, n);
    p.blocks = (G.total_segs + 2 * OLS_WAVES - 1) / (2 * OLS_WAVES);
    if (p.blocks > p.max_blocks) p.blocks = p.max_blocks;
}

// the 1024-point kernels by K (ols_filter): the segment walk and the super-block walk
const void *const OLS_SEG_BY_K[5] = {kfn(k_fir_ols_seg_f32<0>), kfn(k_fir_ols_seg_f32<1>), kfn(k_fir_ols_seg_f32<2>),
                                     kfn(k_fir_ols_seg_f32<3>), kfn(k_fir_ols_seg_f32<4>)};
const void *const OLS_CHAIN_BY_K[5] = {kfn(k_fir_ols_chain_f32<0>), kfn(k_fir_ols_chain_f32<1>), kfn(k_fir_ols_chain_f32<2>),
                                       kfn(k_fir_ols_chain_f32<3>), kfn(k_fir_ols_chain_f32<4>)};

// The real spectrum product is taken where the handle's tables carry it (the host decides from the taps: llzs_ols_tables) and
// the call's tap count is the one the table was centred for.  The ols_real_product tune: unset = this choice, 0 = the complex
// product.
int ols_real_rows(const llzs_ols_tables *t, int flt_len)
{
    if (!t->hreal || t->real_rows < 1 || t->real_rows > 4 || flt_len != 64 * t->real_rows + 1) return 0;
    return llzs_tune(LLZS_TUNE_OLS_REAL_PRODUCT) == 0 ? 0 : t->real_rows;
}

} // namespace

extern "C" int llzs_fir_ols_f32(int nfft, const llzs_ols_tables *t, const float *in, float *out, const float *hist, int channels,
                                int n, long in_pitch, long out_pitch, int flt_len, void *stream)
{
    const ols_rung *r = nullptr;
    for (const ols_rung &c : OLS_RUNGS)
        if (c.nfft == nfft) r = &c;
    if (!r || !t || !t->hfreq || !t->twid || (r->w2k && !t->tw2k) || (r->w4k && !t->tw4k) || !in || !out || channels <= 0 ||
        n <= 0 || in_pitch < n || out_pitch < n) {
        llzs_set_error("fir_ols_f32: bad arguments (%d points)", nfft);
        return LLZ_ERR_ARG;
    }
    if (flt_len < r->min_taps || flt_len - 1 > r->overlap[r->count - 1]) {
        llzs_set_error("fir_ols_f32: flt_len %d outside %d..%d (%d points)", flt_len, r->min_taps, r->overlap[r->count - 1] + 1,
                       nfft);
        return LLZ_ERR_RANGE;
    }
    ols_plan p = ols_plan_of(*r, channels, n, in_pitch, out_pitch, flt_len);
    const float2 *hf = reinterpret_cast<const float2 *>(t->hfreq), *tw = reinterpret_cast<const float2 *>(t->twid),
                 *w2 = reinterpret_cast<const float2 *>(t->tw2k), *w4 = reinterpret_cast<const float2 *>(t->tw4k);
    void *args[8] = {&in, &out, &hist, &hf, &tw};              // the kernels' parameters: w2 and w4 where the rung takes them
    int k = 5;
    if (r->w2k) args[k++] = &w2;
    if (r->w4k) args[k++] = &w4;
    args[k] = &p.G;
    const void *kernel = r->kernel[p.instance];
    if (r->nfft == 1024) {
        const int K = ols_real_rows(t, flt_len);
        if (K > 0) hf = reinterpret_cast<const float2 *>(t->hreal);
        kernel = OLS_SEG_BY_K[K];
        if (ols_sb_applies(p, in, out, in_pitch, out_pitch, n)) {
            ols_sb_plan(p, channels, n);
            kernel = OLS_CHAIN_BY_K[K];
        }
    }
    if (r->lds_bytes > 64 * 1024)
        LLZ_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r->lds_bytes));
    (void)hipLaunchKernel(kernel, dim3((unsigned)p.blocks), dim3(r->threads), args, r->lds_bytes, as_stream(stream));
    LLZ_LAUNCH_CHECK(r->name);
    return LLZ_OK;
}

extern "C" int llzs_fir_ols_superblock(const float *in, const float *out, int channels, int n, long in_pitch, long out_pitch,
                                       int flt_len)
{
    const ols_rung &r = OLS_RUNGS[0];
    if (channels <= 0 || n <= 0 || in_pitch < n || out_pitch < n || flt_len < r.min_taps || flt_len - 1 > r.overlap[r.count - 1])
        return 0;
    const ols_plan p = ols_plan_of(r, channels, n, in_pitch, out_pitch, flt_len);
    return ols_sb_applies(p, in, out, in_pitch, out_pitch, n) ? 1 : 0;
}

extern "C" int llzs_fir_ols_real_rows(const llzs_ols_tables *t)
{
    return t ? ols_real_rows(t, 64 * t->real_rows + 1) : 0;
}

#ifdef O8K_TRACE
extern "C" int llzs_o8k_trace_read(unsigned long long *dst, int count)
{
    LLZ_HIP_CHECK(hipDeviceSynchronize());
    LLZ_HIP_CHECK(hipMemcpyFromSymbol(dst, HIP_SYMBOL(o8k_trace_buf), sizeof(unsigned long long) * (size_t)count));
    return LLZ_OK;
}
#endif
