/*
 * include/llz_suppress_bands.h -- the stage between a subband echo canceller and the synthesis of its filter bank, C ABI of
 * libllzfilter_hip.so: llz_suppress_bands_mc, a real gain G for every (channel, bin, frame) of a batch of band signals, formed from
 * tracked powers, that takes out what a linear filter of K taps per band leaves behind -- the microphone's stationary noise and
 * the residual echo (the tail beyond K, the misalignment while the path moves, whatever is not linear).  It is MCRA noise tracking
 * (Cohen and Berdugo 2002) without smoothing across bins, a decision-directed Wiener gain and a peak-hold residual-echo estimate.
 * It consumes what llz_kalman_bands_mc (llz_kalman_bands.h) or llz_adapt_bands_mc produce, the error e and on request the echo
 * estimate y, in the same layout; without y it is a stand-alone noise suppressor for any band signal of the polyphase filter bank
 * or of llz_stft_mc.  The reference has no counterpart; the checker is a float64 model written from the definition below
 * (tests/suppress_bands_checks.py).  No terms across bins or channels.
 *
 * Signals: [channels][frames][bins] float32, re and im in arrays of their own; channels 1..65535, bins 1..4097, frames x bins at
 * most 2^31 - 1.  Inputs e and optionally y; outputs o = G e and optionally g = G (real, the same shape).
 *
 * The state of a (channel c, bin k), seven float32 values, [7][channels][bins] on the device:
 *   S     smoothed power of e                                   0 at init
 *   Smin  tracked minimum of S                                  0
 *   Stmp  the minimum's second window                           0
 *   q     smoothed probability that only noise is present       1
 *   N     noise power                                           0
 *   R     residual-echo power with its hold                     0
 *   Z     |o|^2 of the frame before                             0
 * and for the handle a 64-bit count of frames taken since init or reset.  Per channel: gmin, the gain floor, in [0, 1], 0.1 at
 * init; eta, the echo leakage, >= 0 and finite, 0 at init; an enable flag, on at init.
 *
 * The parameters (llz_suppress_cfg, fixed at init): window W, 2..65535 frames (128); as, aq, ad, beta, rho, each in [0, 1) (0.8,
 * 0.2, 0.95, 0.98, 0.6); thresholds 0 < t0 < t1, finite (2, 5); delta > 0 and finite, in units of |e|^2 (1e-6).  The host forms
 * these constants once, in float32: omas = 1 - as, omaq = 1 - aq, omad = 1 - ad, omb = 1 - beta, kt = 1 / (t1 - t0).
 *
 * For frame m of a call, n = count + m.  All arithmetic is float32; fma(a, b, c) = a b + c rounded once, every other operation
 * rounded on its own; 1 / x is the correctly rounded quotient; every selection is the comparison written (a < b ? a : b), so a NaN
 * fails it.
 *   pe = fma(e_im, e_im, e_re * e_re)          py = fma(y_im, y_im, y_re * y_re), or 0 without y
 *   start-up, n < W:   c = 1 / (float)(n + 1)
 *     sa   = c > omas ? c : omas               S = fma(sa, pe - S, S)          Smin = Stmp = S
 *     step = c > omad ? c : omad                                               q is left at its value
 *   running, n >= W:
 *     S = fma(omas, pe - S, S)
 *     n % W == 0:  Smin = S < Stmp ? S : Stmp;  Stmp = S
 *     else:        Smin = S < Smin ? S : Smin;  Stmp = S < Stmp ? S : Stmp
 *     rm = 1 / (Smin + delta)
 *     J  = (fma(t1, Smin, -S) * rm) * kt;   J < 0: J = 0;   J > 1: J = 1
 *     q  = fma(aq, q, omaq * J)                step = omad * q
 *   N = fma(step, pe - N, N)
 *   a = eta * py;  b = rho * R;  R = a > b ? a : b
 *   Q = (N + delta) + R;   rq = 1 / Q
 *   post = pe * rq;   ml = post - 1;   ml < 0: ml = 0
 *   prio = fma(beta, Z * rq, omb * ml)
 *   rg = 1 / (1 + prio);   G = prio * rg;   G < gmin: G = gmin;   G > 1: G = 1
 *   o_re = G * e_re;  o_im = G * e_im;   Z = fma(o_im, o_im, o_re * o_re)
 * THE FIRST W FRAMES BEHIND INIT OR RESET ARE TAKEN AS NOISE ONLY: S and N are running means there (c = 1 / (n + 1) until the
 * recursions' own constants are larger), no minimum is tracked and q stays.  A caller that cannot offer W frames without speech
 * chooses a smaller W; what speech the start-up holds is taken for noise until the minimum has fallen below it (within 2 W frames).
 * J is the probability of noise only as a ramp: 1 where S <= t0 Smin, 0 where S >= t1 Smin.  The state holds q = 1 - p, not the
 * speech probability p, so that the noise step omad q keeps its relative precision while speech freezes the estimate.
 * Every decision is a clamp, a min or a max of continuous quantities, never a threshold on a ratio: a rounding error moves a
 * result by a rounding error and cannot flip a branch.  The two that are not (n < W, n % W == 0) depend on the frame count alone.
 *
 * A DISABLED channel takes no step at all: o has e's bits, g = 1, its seven state values keep their bits; n still advances (it is
 * the handle's).
 *
 * What always holds (as long as nothing overflows: inf - inf is a NaN, and a NaN stays one):
 *   N >= 0.  N' = fma(step, pe - N, N) is the rounding of (1 - step) N + step pe, a convex combination of N >= 0 and pe >= 0 (a sum
 *     of squares) because 0 <= step <= 1: in the start-up step is c <= 1 or omad < 1, both > 0; running it is omad q with q in
 *     [0, 1] (q starts at 1 and fma(aq, q, omaq J) is the rounding of a convex combination of q and J in [0, 1]; aq + omaq may
 *     exceed 1 by 2^-24, which the rounding of omad q <= omad (1 + 2^-23) < 1 absorbs).  The exact value is >= 0 and rounding is
 *     monotone, so N' >= 0.  The same argument gives S >= 0, hence Smin, Stmp >= 0.
 *   Q >= delta > 0.  N + delta >= delta (N >= 0, rounding is monotone), R >= 0 (eta, py, rho >= 0, and the larger of two
 *     non-negative values), so (N + delta) + R >= delta.  Likewise Smin + delta >= delta: rm and rq are finite.
 *   0 <= G <= 1.  ml >= 0 by its clamp, Z >= 0, rq > 0, beta and omb >= 0: prio >= 0, so 1 + prio >= 1, 0 < rg <= 1 and
 *     G = prio rg >= 0.  prio rg <= 1 wherever rg is a normal number, by the argument llz_kalman_bands.h gives for c_q; where it is
 *     subnormal (prio above 2^126) its relative error is larger, and there the upper clamp holds the invariant, as c_q's clamp does
 *     in the Kalman filter.  Then gmin <= G (gmin in [0, 1]).  set_floor refuses anything else.
 * A NaN in e makes that bin's S and N (and with them G, o, Z) NaN until reset; it reaches no other bin and no other channel.
 *
 * On the fixed order rest the bitwise properties, llz_kalman_bands.h's: no bit of o, g or the state depends
 *   - on how the frames are grouped into calls, down to calls of one frame and empty calls, across n = W and a window swap;
 *   - on what any other (channel, bin) holds;
 *   - on whether the caller's pointers are host or device memory;
 *   - on whether g is asked for; and y passed with eta = 0 gives the bits of a call without y (a finite y);
 * and reset followed by the same input repeats a fresh handle's bits.
 *
 * One kernel launch per call, whatever its frames: a lane owns one (channel, bin) and walks the call's frames with its state in
 * registers.
 */
#ifndef LLZ_SUPPRESS_BANDS_H
#define LLZ_SUPPRESS_BANDS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct llz_suppress_cfg {
    int   window;       /* W: frames of one window of the minimum search, 2..65535; the start-up lasts W frames       (128)  */
    float as;           /* smoothing of S, [0, 1)                                                                    (0.8)  */
    float aq;           /* smoothing of q, [0, 1)                                                                    (0.2)  */
    float ad;           /* smoothing of N where only noise is present, [0, 1)                                        (0.95) */
    float t0, t1;       /* S / Smin at and below which a frame is noise only, at and above which it is not; 0 < t0 < t1 (2, 5) */
    float beta;         /* weight of the frame before in the decision-directed a-priori ratio, [0, 1)                (0.98) */
    float rho;          /* decay per frame of the residual-echo hold, [0, 1)                                         (0.6)  */
    float delta;        /* regularisation, > 0 and finite, in units of |e|^2                                         (1e-6) */
} llz_suppress_cfg;

enum {                  /* `which` of llz_suppress_bands_mc_get_state */
    LLZ_SUPPRESS_S = 0, LLZ_SUPPRESS_SMIN = 1, LLZ_SUPPRESS_STMP = 2, LLZ_SUPPRESS_Q = 3, LLZ_SUPPRESS_N = 4,
    LLZ_SUPPRESS_R = 5, LLZ_SUPPRESS_Z = 6, LLZ_SUPPRESS_STATES = 7
};

/* the defaults above into *cfg (a NULL cfg is ignored) */
void llz_suppress_bands_mc_default_cfg(llz_suppress_cfg *cfg);
/* channels 1..65535; bins 1..4097; cfg as above (NULL: the defaults).  Device memory: channels x bins x 28 bytes of state and
 * channels x 12 of floors, leakages and flags; when the allocation fails the message states the bytes asked for.  Every refusal
 * leaves a message of its own.  Returns the handle or (unsigned long)-1 (llz_hip_last_error() says why). */
unsigned long llz_suppress_bands_mc_init(int channels, int bins, const llz_suppress_cfg *cfg);
void llz_suppress_bands_mc_uninit(unsigned long h);
/* e (the canceller's error), y (its echo estimate; yre and yim both NULL or both set), o (out), g (the gain, out; NULL: not
 * wanted): [channels][frames][bins] float32, device memory (used in place, asynchronous on the handle's stream) or host memory
 * (staged, synchronous).  frames = 0 returns 0 and touches nothing.  Refused with LLZ_ERR_ARG, the handle left where it was: a
 * device range of an output that overlaps an input or another output, and frames x bins beyond 2^31 - 1.  Returns frames, or a
 * negative LLZ_ERR_* code. */
int  llz_suppress_bands_mc(unsigned long h, const float *ere, const float *eim, const float *yre, const float *yim,
                           float *ore, float *oim, float *g, int frames);
/* the gain floors of channels [first, first + count): gmin = HOST [count], each in [0, 1] (else refused, nothing changed);
 * ordered on the handle's stream behind the calls already issued */
int  llz_suppress_bands_mc_set_floor(unsigned long h, int first, int count, const float *gmin);
/* the echo leakages of channels [first, first + count): eta = HOST [count], each finite and >= 0 (else refused, nothing
 * changed): the share of |y|^2 taken for residual echo in e; 0 leaves the echo branch idle */
int  llz_suppress_bands_mc_set_leak(unsigned long h, int first, int count, const float *eta);
/* whether channels [first, first + count) are processed: on = HOST [count], 0 = disabled (o = e, g = 1, state kept), anything
 * else = enabled */
int  llz_suppress_bands_mc_set_enable(unsigned long h, int first, int count, const int *on);
/* state value `which` (LLZ_SUPPRESS_S .. LLZ_SUPPRESS_Z; every other value is refused) of channels [first, first + count): out =
 * HOST [count][bins], downloaded behind the calls already issued: the handle's own float32 values, bit for bit */
int  llz_suppress_bands_mc_get_state(unsigned long h, int which, int first, int count, float *out);
/* the state and the frame count back to init; flags, floors and leakages are kept */
int  llz_suppress_bands_mc_reset(unsigned long h);
/* *out = the frames taken since the init or the last reset */
int  llz_suppress_bands_mc_frames(unsigned long h, long long *out);
/* out = {the last call's form: 1 with y, 0 without (0 before the first call), threads per workgroup, workgroups, launches per
 * call}; nothing is launched */
int  llz_suppress_bands_mc_plan(unsigned long h, int out[4]);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int  llz_suppress_bands_mc_set_stream(unsigned long h, void *stream);

#ifdef __cplusplus
}
#endif
#endif
