/* llz_asrc_time.h -- INTERNAL: the integer time of llz_asrc_mc (include/llz_asrc.h), shared by the host layer (llz_asrc_host.c, plain C) and
 * the kernels (kernels/asrc.hip): one piece of code decides on both sides when an output is taken and how many a call delivers, so the
 * host's counts and the device's state cannot drift apart.
 *
 * A channel's state, relative to the buffer of a call = [H history samples | n_in new samples]:
 *   pos     Q32.32 position of the next output (output 0 of the next call) in that buffer
 *   inc     the step that follows that output, Q32.32
 *   dinc    what the step grows by per output while a glide runs (signed), left = the glide's outputs still to come
 *   target  the step from output `left` on; left == 0 implies inc == target and dinc == 0
 *
 * Output j of the call is taken at  t_j = pos + j inc + dinc j (j - 1) / 2  for j <= left, and at t_left + (j - left) target behind
 * it.  Every step of a glide lies between the step it started from and its target (dinc truncates toward zero), so every step
 * is within [2^28, 2^36].  Every product and sum below may wrap modulo 2^64; the TRUE value of a t_j that is asked for stays
 * below 2^64 and the wrapped result is therefore the true one: asrc_count looks at j <= (bound - pos) / 2^28 + 1 <= 2^27 + 1 only
 * (bound - pos <= (2^22 + 128) 2^32 < 2^55, a step is at least 2^28), and t_j <= pos + j 2^36 < 2^55 + (2^27 + 1) 2^36 < 2^64;
 * the kernel asks for j below the count plus a tile of 1024 at most.  j (j - 1) / 2 itself is exact: j < 2^31.
 */
#ifndef LLZ_ASRC_TIME_H
#define LLZ_ASRC_TIME_H

#ifdef __HIPCC__
#define LLZ_ASRC_FN __host__ __device__ static inline
#else
#define LLZ_ASRC_FN static inline
#endif

#define LLZ_ASRC_MIN_TAPS 4
#define LLZ_ASRC_MAX_TAPS 128
#define LLZ_ASRC_MIN_PHASES 256
#define LLZ_ASRC_MAX_PHASES 4096
#define LLZ_ASRC_MAX_FRAME (1 << 22)
#define LLZ_ASRC_MIN_INC (1ull << 28)           /* step 1/16 */
#define LLZ_ASRC_MAX_INC (1ull << 36)           /* step 16 */

/* The device table: rows of `pitch` floats, pitch = 4 x an odd number >= T, the tail of a row zero (never multiplied: the
 * kernels stop at T).  A lane reads its two rows 16 bytes at a time; 16-byte reads bank on (address / 4) mod 64 within groups of
 * 16 lanes, so rows p and q meet on a bank only when (p - q) (pitch / 4) = 0 mod 16, and with pitch / 4 odd that is p = q mod 16:
 * the lanes of a group, whose phases differ arbitrarily, collide no more often than 16 random draws from 16 slots do, and
 * phases that run through consecutive values (steps near a multiple of 1 / phases) do not collide at all.  Measured against a
 * pitch of T = 32 floats at step 147/160, 1024 channels x 2^20 samples: 14.3 against 24.7 ms.  The table is kept in
 * LDS when its image is within LLZ_ASRC_LDS_TABLE_BYTES (the default 513 x 36 floats = 73872 B is; with the 66 KB input span
 * of a tile that is 140 KB of the CU's 160 KB), else it is read through the caches. */
#define LLZ_ASRC_PITCH(T) (4 * ((((T) + 3) / 4) | 1))
#define LLZ_ASRC_LDS_TABLE_BYTES (80 * 1024)

typedef struct {
    unsigned long long pos, inc, target;
    long long dinc;
    unsigned int left, pad;
} llz_asrc_state;

LLZ_ASRC_FN unsigned long long llz_asrc_time(const llz_asrc_state *s, unsigned long long j)
{
    const unsigned long long g = j <= s->left ? j : s->left;
    const unsigned long long t = s->pos + g * s->inc + (unsigned long long)s->dinc * (g * (g - 1) / 2);
    return t + (j - g) * s->target;
}

/* the outputs delivered by a call whose buffer ends at `bound` = (H + n_in - T / 2) 2^32: the j with t_j < bound, found by
 * bisection on the monotone t_j */
LLZ_ASRC_FN unsigned int llz_asrc_count(const llz_asrc_state *s, unsigned long long bound)
{
    if (s->pos >= bound) return 0;
    unsigned long long lo = 0, hi = ((bound - s->pos) >> 28) + 1;      /* t_lo < bound <= t_hi */
    while (hi - lo > 1) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (llz_asrc_time(s, mid) < bound) lo = mid; else hi = mid;
    }
    return (unsigned int)hi;
}

/* the state behind a call that delivered `count` outputs and took n_in samples */
LLZ_ASRC_FN void llz_asrc_advance(llz_asrc_state *s, unsigned int count, unsigned long long n_in)
{
    s->pos = llz_asrc_time(s, count) - (n_in << 32);
    if (count >= s->left) {
        s->inc = s->target; s->dinc = 0; s->left = 0;
    } else {
        s->inc += (unsigned long long)s->dinc * count;
        s->left -= count;
    }
}

#endif
