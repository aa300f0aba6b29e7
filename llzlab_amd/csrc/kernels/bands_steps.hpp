// bands_steps.hpp -- what the four per-band kernels share: adapt_bands.hip (K4j, k_bands_nlms), adapt_bands_matrix.hip (K4k,
// k_bands_matrix_nlms), kalman_bands.hip (K4l, k_bands_kalman) and suppress_bands.hip (K4m, k_bands_suppress).  One plan serves
// them all: a lane owns one (row, bin), lane g = row bins + k, a workgroup is one wave, the lane's state lives in register arrays
// indexed by constants, and one launch walks a call's frames.  Here are the pieces of that plan that are the same text in every
// kernel -- the state's addressing behind a scalar base, the walk over the taps (or entries) that exist, the entries an instance
// takes for granted, the shift of the history -- and the launch arithmetic of their shims: the grid, the ceiling, the shape
// refusal and the tail of a plan.
//
// What is NOT here, because sharing it changes the instruction text of an instance (DESIGN.md, K4j-K4m "Shared code"): the output
// sum y = sum w[q] x[q], which as an inline function reorders its two fma chains in several instances of k_bands_kalman, and the
// epilogue's state store, which split per array reorders the stores and moves register counts.  Both stay written out.
//
// A fifth kernel stands on the same pieces: kalman_bands_matrix.hip (K4n, k_bands_matrix_kalman), K4l's recursion on K4k's plan.
#pragma once
#include <stdio.h>
#include "common.hpp"

namespace {

constexpr int BANDS_THREADS = 64;       // a workgroup is one wave: no lane shares anything with another

// the taps (entries) an instance of ceiling C can take for granted: more than C / 2 select it, and the instance of the SMALLEST
// ceiling takes whatever is left, FIRST at the least (one tap; the matrix kernel: one tap of each of its I inputs)
template <int C, int SMALLEST, int FIRST> struct bands_live {
    static constexpr int value = C == SMALLEST ? FIRST : C / 2 + 1;
};

// element `off` (a byte offset below 2^32) behind a scalar base: one 32-bit register of address per lane for the whole state.
// The base is pinned to scalar registers; left alone, the compiler folds the lane's offset into it and keeps a 64-bit address
// per load in vector registers (twice the registers of the state itself in the prologue).
__device__ __forceinline__ float bands_ld(const float *base, unsigned off)
{
    asm("" : "+s"(base));
    return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + off);
}
__device__ __forceinline__ void bands_st(float *base, unsigned off, float v)
{
    asm("" : "+s"(base));
    *reinterpret_cast<float *>(reinterpret_cast<char *>(base) + off) = v;
}

// an unrolled loop over the ages q of a ceiling of C that leaves at the first of the N taps (entries) that does not exist; LIVE,
// the caller's bands_live<>::value, needs no test.  The empty statement keeps the test a scalar branch (without it the compiler
// computes every tap of the ceiling and selects, at twice the registers).
#define BANDS_WALK(q, C, N)                                                                                               \
    _Pragma("unroll") for (int q = 0; q < C; q++)                                                                         \
        if (q >= LIVE && q >= N) break;                                                                                   \
        else if (bands_keep_branch(), true)
__device__ __forceinline__ void bands_keep_branch() { asm volatile(""); }

// the history moves on by one age, I registers (I inputs; 1 for one reference), dead ones included: they take older frames that
// nothing reads, and a plain chain of moves leaves the walks nothing to merge where they end.  The caller puts the frame at age 0.
template <int I, int C> __device__ __forceinline__ void bands_shift(float (&xr)[C], float (&xi)[C])
{
#pragma unroll
    for (int j = C - 1; j >= I; j--) {
        xr[j] = xr[j - I];
        xi[j] = xi[j - I];
    }
}

// ---- the shims' launch arithmetic ----
static unsigned bands_grid(int lanes) { return (unsigned)((lanes + BANDS_THREADS - 1) / BANDS_THREADS); }

// the instance of `n` taps (entries): the first power of two from `lowest` on that holds them, `highest` at the most
static int bands_ceiling(int n, int lowest, int highest)
{
    int c = lowest;
    while (c < highest && n > c) c *= 2;
    return c;
}

struct bands_dim {                      // one dimension of a shape: what the message calls it, its value and its upper limit
    const char *name;
    int value, max;
};

// every dimension in 1..max and whatever else the caller asks (`also`), or LLZ_ERR_ARG and "<who>: bad shape (name=value ...)"
static int bands_shape(const char *who, const bands_dim *dims, int count, bool also = true)
{
    bool ok = also;
    for (int i = 0; i < count; i++) ok = ok && dims[i].value >= 1 && dims[i].value <= dims[i].max;
    if (ok) return LLZ_OK;
    char text[128];
    int at = 0;
    for (int i = 0; i < count && at < (int)sizeof(text); i++)
        at += snprintf(text + at, sizeof(text) - (size_t)at, "%s%s=%d", i ? " " : "", dims[i].name, dims[i].value);
    llzs_set_error("%s: bad shape (%s)", who, text);
    return LLZ_ERR_ARG;
}

// a plan shim's refusal of a missing out
static int bands_no_out(const char *who, const int *out)
{
    if (out) return LLZ_OK;
    llzs_set_error("%s: no out", who);
    return LLZ_ERR_ARG;
}

// the tail of a plan: {what names the instance, threads per workgroup, workgroups, launches}
static void bands_plan_tail(int *out, int first, int lanes)
{
    out[0] = first;
    out[1] = BANDS_THREADS;
    out[2] = (int)bands_grid(lanes);
    out[3] = 1;
}

} // namespace
