// acf_fft.hip -- FFT autocorrelation (reference libllzfilter/llz_corr.c:155-177) fused into one launch, float32: real frame
// -> zero-padded transform -> power spectrum of the first n bins -> inverse transform -> r[k] = 2 Re, one read of the frame
// and p+1 floats written per frame.
//
//   k_acf_fused_f32   any fft length 8..4096 on the staged passes of fft_core.hpp
//   k_acf_sq_f32      fft length 128, 512 on square_core (fft_square.hpp): one half-size complex transform per direction
//   k_acf1024_f32     fft length 1024 on the half-wave machinery of fft32.hpp
//   k_acf2048_f32     fft length 2048 as one 1024-point complex transform per direction on a half-wave
//   k_acf4096_f32     fft length 4096 as one 2048-point complex transform per direction on a whole wave
#include "fft_square.hpp"

namespace {

// FFT autocorrelation (reference libllzfilter/llz_corr.c:155-177) fused in LDS: real frame -> zero-padded complex ->
// forward passes (bins end up bit-reversed, which is exactly the order the inverse DIT passes consume) -> power
// spectrum of the first n bins, everything else zero, 1/F folded in -> inverse passes -> r[k] = 2 Re.  One read of the
// frame and p+1 floats written per frame instead of five launches over a 2F-float buffer.
__global__ void __launch_bounds__(FFT_THREADS)
k_acf_fused_f32(const float *__restrict__ x, float *__restrict__ r, int frames, int n, int p, int size, int log2n,
                const float *__restrict__ cs, int tpw, unsigned groups)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cpx<float> *s = reinterpret_cast<cpx<float> *>(smem_raw);
    const int tid = threadIdx.x;
    const int tr0 = blockIdx.x * tpw;
    const int ntr = min(tpw, frames - tr0);
    const int tstride = fft_tstride(size);
    const int total = ntr << log2n;
    cpx<float> *tw = s + (size_t)tpw * tstride;
    fft_load_twiddles(tw, cs, size, tid);
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2n, i = e & (size - 1);
        cpx<float> v;
        v.re = i < n ? x[(size_t)(tr0 + tr) * n + i] : 0.f;
        v.im = 0.f;
        s[tr * tstride + fft_phys(i)] = v;
    }
    __syncthreads();
    fft_run<arith_f32, false>(s, ntr, size, log2n, tstride, tw, groups, tid);
    // position j holds bin brev(j): keep |X|^2 / F for bins < n (llz_corr.c:165-170; the 1/F of llz_ifft folded in)
    const float inv = 1.0f / (float)size;
    for (int e = tid; e < total; e += FFT_THREADS) {
        const int tr = e >> log2n, j = e & (size - 1);
        const int bin = (int)(__brev((unsigned)j) >> (32 - log2n));
        cpx<float> &v = s[tr * tstride + fft_phys(j)];
        const float pw = bin < n ? __builtin_fmaf(v.re, v.re, v.im * v.im) * inv : 0.f;
        v.re = pw;
        v.im = 0.f;
    }
    __syncthreads();
    fft_run<arith_f32, true>(s, ntr, size, log2n, tstride, tw, groups, tid);
    for (int e = tid; e < ntr * (p + 1); e += FFT_THREADS) {
        const int tr = e / (p + 1), k = e - tr * (p + 1);
        r[(size_t)(tr0 + tr) * (p + 1) + k] = s[tr * tstride + fft_phys(k)].re * 2.f;      // llz_corr.c:173
    }
}

// FFT autocorrelation for fft_len = 1024 (frames of 257..512 samples): the two transforms of llz_corr.c:155-177 as they
// stand (complex, zero imaginary parts) on the half-wave machinery -- twice the arithmetic of the real-input form above,
// but a half size of 512 = 2 x 16^2 has no single-group register transform with the mirrored bins in reach, and even so
// this is several times the staged kernel.  For p < 32 the second inverse pass is its bin 0 only.
__global__ void __launch_bounds__(256)
k_acf1024_f32(const float *__restrict__ x, float *__restrict__ r, int frames, int n, int p,
              const float *__restrict__ cs /* 1024 cos, then 1024 sin of 2 pi i / 1024 */)
{
    __shared__ float2 s_tw[1024];                                  // W_1024^(a*b), [a][b]
    __shared__ float bufs[8][OLS_XBUF];
    const int tid = threadIdx.x, hw = tid >> 5, l5 = tid & 31;
    load_tw1024(s_tw, cs, tid);
    __syncthreads();
    const long t = (long)blockIdx.x * 8 + hw;
    if (t >= frames) return;
    const float *g = x + t * n;
    float *buf = bufs[hw];
    cf v[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int i = l5 + 32 * j;
        v[j] = cf{(j < 16 && i < n) ? g[i] : 0.f, 0.f};            // n <= 512: the upper half is padding
    }
    fft32<false>(v);
    transpose_twiddle<false>(v, buf, s_tw, l5);
    fft32<false>(v);                                               // v[q] = X[l5 + 32 brev5(q)]
    cf u[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {                                 // bin l5 + 32 j sits in register brev5(j)
        const cf z = v[brev5(j)];
        const int bin = l5 + 32 * j;
        // |X|^2 / F of the first n bins, everything else zero (llz_corr.c:165-170; the 1/F of llz_ifft folded in)
        u[j] = cf{bin < n ? __builtin_fmaf(z.x, z.x, z.y * z.y) * (1.0f / 1024.0f) : 0.f, 0.f};
    }
    fft32<true>(u);
    transpose_twiddle<true>(u, buf, s_tw, l5);
    float *rr = r + t * (p + 1);
    if (p < 32) {                                                  // only g[l5] = the sum over the column index
        float acc = u[0].x;
#pragma unroll
        for (int q = 1; q < 32; q++) acc += u[q].x;
        if (l5 <= p) rr[l5] = 2.f * acc;                           // llz_corr.c:173
    } else {
        fft32<true>(u);                                            // u[q] = g[l5 + 32 brev5(q)]
#pragma unroll
        for (int q = 0; q < 32; q++) {
            const int k = l5 + 32 * brev5(q);
            if (k <= p) rr[k] = 2.f * u[q].x;
        }
    }
}

// FFT autocorrelation for fft_len = 2048 (frames of 513..1024 samples) on the half-wave machinery.  Both 2048-point
// transforms of llz_corr.c:155-177 act on real data, so each is ONE 1024-point complex transform:
//   forward: z[m] = x[2m] + j x[2m+1]; Z = FFT_1024(z); with Zm = Z[1024-k]: Xe = (Z[k] + conj(Zm))/2,
//            Xo = (Z[k] - conj(Zm))/(2j), T = W_2048^k Xo:  X[k] = Xe + T,  X[1024-k] = conj(Xe - T);
//   power:   P[b] = |X[b]|^2 / 2048 for b < n (the reference squares only the first n bins), else 0;
//   inverse: r[k] = 2 Re sum_{b<n} P[b] W^-bk is the real inverse transform of the symmetric spectrum S[b] = S[2048-b] =
//            P[b] (b >= 1), S[0] = 2 P[0], S[1024] = 0:  G[b] = (S[b] + S[1024-b]) + j conj(W^b) (S[b] - S[1024-b]),
//            g = IFFT_1024(G) unnormalised, r[2m] = Re g[m], r[2m+1] = Im g[m].
// The mirrored bin lives in lane (32 - l) of the same half-wave: one more LDS round trip per plane.  For p < 64 only
// g[0..31] is needed, i.e. bin 0 of the second register pass: 31 complex adds instead of a 32-point transform.
// (184 VGPRs as written: three waves per SIMD are asked for, 168 registers and a few spilled -- 0.73 -> 0.60 ms)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3)))
k_acf2048_f32(const float *__restrict__ x, float *__restrict__ r, int frames, int n, int p,
              const float *__restrict__ cs /* 2048 cos, then 2048 sin of 2 pi i / 2048 */)
{
    __shared__ float2 s_tw[1024];                                  // W_1024^(a*b), [a][b]
    __shared__ float2 s_w2[1024];                                  // W_2048^k, k < 1024
    __shared__ float bufs[8][OLS_XBUF];
    const int tid = threadIdx.x, hw = tid >> 5, l5 = tid & 31;
    for (int i = tid; i < 1024; i += 256) {
        const int m = (2 * (i >> 5) * (i & 31)) & 2047;
        s_tw[i] = make_float2(cs[m], -cs[2048 + m]);
        s_w2[i] = make_float2(cs[i], -cs[2048 + i]);
    }
    __syncthreads();
    const long t = (long)blockIdx.x * 8 + hw;
    if (t >= frames) return;
    const float *g = x + t * n;
    float *buf = bufs[hw];
    cf v[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {                                 // 2 m < 1024: the upper half of z is padding
        const int i0 = 2 * (l5 + 32 * j);
        v[j].x = i0 < n ? g[i0] : 0.f;
        v[j].y = i0 + 1 < n ? g[i0 + 1] : 0.f;
    }
#pragma unroll
    for (int j = 16; j < 32; j++) v[j] = cf{0.f, 0.f};
    fft32<false>(v);
    transpose_twiddle<false>(v, buf, s_tw, l5);
    fft32<false>(v);                                               // v[q] = Z[l5 + 32 brev5(q)]
    // mirrored bins: Z[1024 - k] sits in lane (32 - l5) & 31 at column index 31 - j (lane 0: (32 - j) & 31)
    const int lm = (32 - l5) & 31;
    float mx[32];
#pragma unroll
    for (int q = 0; q < 32; q++) buf[xaddr(brev5(q), l5)] = v[q].x;
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const int j = brev5(q);
        mx[q] = buf[l5 ? xaddr(31 - j, lm) : xaddr((32 - j) & 31, 0)];
    }
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 32; q++) buf[xaddr(brev5(q), l5)] = v[q].y;
    OLS_WAVE_SYNC();
    const float sc = 1.0f / (4.0f * 2048.0f);                      // the two halvings of (Xe, Xo) and llz_ifft's 1/N
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const int j = brev5(q);
        const int k = l5 + 32 * j;
        const float my = buf[l5 ? xaddr(31 - j, lm) : xaddr((32 - j) & 31, 0)];
        const float2 w = s_w2[k];                                  // (cos, -sin) of pi k / 1024
        const cf xe = {v[q].x + mx[q], v[q].y - my};               // 2 Xe
        const cf xo = {v[q].y + my, mx[q] - v[q].x};               // 2 Xo
        const cf T = cmul<false>(xo, cf{w.x, w.y});
        const cf a = cadd(xe, T), b = csub(xe, T);
        float sk = __builtin_fmaf(a.x, a.x, a.y * a.y) * sc, sm = __builtin_fmaf(b.x, b.x, b.y * b.y) * sc;
        if (k >= n) sk = 0.f;
        if (1024 - k >= n) sm = 0.f;
        if (k == 0) { sk *= 2.f; sm = 0.f; }                       // S[0] = 2 P[0]; the mirror of bin 0 is bin 1024: unused
        const float dk = sk - sm;
        v[q] = cf{__builtin_fmaf(w.y, dk, sk + sm), w.x * dk};     // (S + Sm) + j (c + j s) dk,  w.y = -s
    }
    OLS_WAVE_SYNC();
    cf u[32];
#pragma unroll
    for (int j = 0; j < 32; j++) u[j] = v[brev5(j)];               // bin order -> natural order: register renaming
    fft32<true>(u);
    transpose_twiddle<true>(u, buf, s_tw, l5);
    float *rr = r + t * (p + 1);
    if (p < 64) {                                                  // only g[l5] = the sum over the column index
        cf acc = u[0];
#pragma unroll
        for (int q = 1; q < 32; q++) acc = cadd(acc, u[q]);
        if (2 * l5 <= p) rr[2 * l5] = acc.x;
        if (2 * l5 + 1 <= p) rr[2 * l5 + 1] = acc.y;
    } else {
        fft32<true>(u);                                            // u[q] = g[l5 + 32 brev5(q)]
#pragma unroll
        for (int q = 0; q < 32; q++) {
            const int m = l5 + 32 * brev5(q);
            if (2 * m <= p) rr[2 * m] = u[q].x;
            if (2 * m + 1 <= p) rr[2 * m + 1] = u[q].y;
        }
    }
}

// FFT autocorrelation for fft_len = 4096 (frames of 1025..2048 samples): the real-input scheme of k_acf2048_f32 one size up --
// both 4096-point transforms are ONE 2048-point complex transform each, and that transform runs on a WHOLE WAVE as in
// fir_ols.hip (k_fir_ols2k_chain_f32): one radix-2 step splits it over the two half-waves, each of which runs the 1024-point
// machinery.  z[m] = x[2m] + j x[2m+1], m < 2048, and the frame is at most 2048 samples, so z[m] = 0 for m >= 1024:
//   forward (decimation in frequency):  Z[2k']   = FFT_1024( z[m] )            -> lower half-wave
//                                       Z[2k'+1] = FFT_1024( z[m] W_2048^m )   -> upper half-wave          (m < 1024)
//   a bin's mirror Z[2048 - k] has the parity of k, so it sits in the SAME half-wave: index (1024 - k') mod 1024 among the
//   even bins, 1023 - k' among the odd ones -- one LDS round trip per plane, as in k_acf2048_f32;
//   X[k] = Xe + W_4096^k Xo, power, symmetric spectrum and G[k] as there (4096 for 2048, 2048 for 1024);
//   inverse (decimation in time):  g[m], g[m + 1024] = S'[m] +- W_2048^-m D'[m],  S' / D' = IFFT_1024 of G's even / odd bins;
//   r[2m] = Re g[m], r[2m + 1] = Im g[m].
// Lane (half h, l5) owns the rows of parity h of the 64 x 32 sample block (row 2p + h, p < 32) at column l5: rows p and p + 16
// are 1024 samples apart, so the butterflies of both radix-2 steps are in-lane and one v_permlane32_swap per register pair
// sorts sums / differences to the lower / upper half-wave.
__global__ void __launch_bounds__(256, 2)
k_acf4096_f32(const float *__restrict__ x, float *__restrict__ r, int frames, int n, int p,
              const float *__restrict__ cs /* 4096 cos, then 4096 sin of 2 pi i / 4096 */)
{
    __shared__ float2 s_tw[1024];                                  // W_1024^(a*b), [a][b]
    __shared__ float2 s_w2[1024];                                  // W_2048^m, m < 1024
    __shared__ float2 s_w4[2048];                                  // W_4096^k, k < 2048
    __shared__ float bufs[8][OLS_XBUF];
    const int tid = threadIdx.x, l5 = tid & 31, half = (tid >> 5) & 1;
    for (int i = tid; i < 1024; i += 256) {
        const int m = (4 * (i >> 5) * (i & 31)) & 4095;
        s_tw[i] = make_float2(cs[m], -cs[4096 + m]);
        s_w2[i] = make_float2(cs[2 * i], -cs[4096 + 2 * i]);
        s_w4[i] = make_float2(cs[i], -cs[4096 + i]);
        s_w4[1024 + i] = make_float2(cs[1024 + i], -cs[4096 + 1024 + i]);
    }
    __syncthreads();
    const long t = (long)blockIdx.x * 4 + (tid >> 6);              // a wave per frame
    if (t >= frames) return;
    const float *g = x + t * n;
    float *buf = bufs[tid >> 5];
    const int rowoff = 32 * half + l5;
    // ---- this lane's rows of z (m = 64 q + rowoff < 1024; the upper half of z is padding) and the radix-2 step down
    cf w[32];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int i0 = 2 * (64 * q + rowoff);
        cf sm = {i0 < n ? g[i0] : 0.f, i0 + 1 < n ? g[i0 + 1] : 0.f};
        const float2 tw = s_w2[64 * q + rowoff];
        cf df = cmul<false>(sm, cf{tw.x, tw.y});
        swap32(sm.x, df.x);
        swap32(sm.y, df.y);
        w[2 * q] = sm;                                             // lower: z rows 2q, 2q+1; upper: the twiddled copies
        w[2 * q + 1] = df;
    }
    fft32<false>(w);
    transpose_twiddle<false>(w, buf, s_tw, l5);
    fft32<false>(w);                                               // w[q] = Z[2 k' + half], k' = l5 + 32 brev5(q)
    // ---- mirrored bins: even bins k' -> (1024 - k') mod 1024: lane (32 - l5) & 31, column 31 - j (lane 0: (32 - j) & 31);
    //      odd bins k' -> 1023 - k': lane 31 - l5, column 31 - j
    const int lm = half ? 31 - l5 : (32 - l5) & 31;
    const bool wrap = !half && l5 == 0;
    float mx[32];
#pragma unroll
    for (int q = 0; q < 32; q++) buf[xaddr(brev5(q), l5)] = w[q].x;
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const int j = brev5(q);
        mx[q] = buf[wrap ? xaddr((32 - j) & 31, 0) : xaddr(31 - j, lm)];
    }
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < 32; q++) buf[xaddr(brev5(q), l5)] = w[q].y;
    OLS_WAVE_SYNC();
    const float sc = 1.0f / (4.0f * 4096.0f);                      // the two halvings of (Xe, Xo) and llz_ifft's 1/N
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const int j = brev5(q);
        const int k = 2 * (l5 + 32 * j) + half;                    // this lane's bin, k < 2048
        const float my = buf[wrap ? xaddr((32 - j) & 31, 0) : xaddr(31 - j, lm)];
        const float2 tw = s_w4[k];                                 // (cos, -sin) of 2 pi k / 4096
        const cf xe = {w[q].x + mx[q], w[q].y - my};               // 2 Xe
        const cf xo = {w[q].y + my, mx[q] - w[q].x};               // 2 Xo
        const cf T = cmul<false>(xo, cf{tw.x, tw.y});
        const cf a = cadd(xe, T), b = csub(xe, T);
        float sk = __builtin_fmaf(a.x, a.x, a.y * a.y) * sc, sm = __builtin_fmaf(b.x, b.x, b.y * b.y) * sc;
        if (k >= n) sk = 0.f;
        if (2048 - k >= n) sm = 0.f;
        if (k == 0) { sk *= 2.f; sm = 0.f; }                       // S[0] = 2 P[0]; the mirror of bin 0 is bin 2048: unused
        const float dk = sk - sm;
        w[q] = cf{__builtin_fmaf(tw.y, dk, sk + sm), tw.x * dk};   // (S + Sm) + j conj(W^k) dk
    }
    OLS_WAVE_SYNC();
    // ---- inverse transforms of the even / odd bins, then the radix-2 step up
    cf u[32];
#pragma unroll
    for (int j = 0; j < 32; j++) u[j] = w[brev5(j)];               // bin order -> natural order: register renaming
    fft32<true>(u);
    transpose_twiddle<true>(u, buf, s_tw, l5);
    fft32<true>(u);                                                // u[q] = S' / D' [32 brev5(q) + l5]
    float *rr = r + t * (p + 1);
#pragma unroll
    for (int q = 0; q < 16; q++) {
        cf P = u[brev5(2 * q)], Q = u[brev5(2 * q + 1)];
        swap32(P.x, Q.x);
        swap32(P.y, Q.y);                                          // lane (half, l5): P = S', Q = D' at m = 64 q + rowoff
        const float2 tw = s_w2[64 * q + rowoff];
        Q = cmul<true>(Q, cf{tw.x, tw.y});
        const cf lo = cadd(P, Q), hi = csub(P, Q);
        const int m = 64 * q + rowoff;
        if (2 * m <= p) rr[2 * m] = lo.x;
        if (2 * m + 1 <= p) rr[2 * m + 1] = lo.y;
        if (2 * (m + 1024) <= p) rr[2 * (m + 1024)] = hi.x;
        if (2 * (m + 1024) + 1 <= p) rr[2 * (m + 1024) + 1] = hi.y;
    }
}

// FFT autocorrelation for fft_len = 2 E^2 (E = 8: 128, E = 16: 512): the real-input scheme of k_acf2048_f32 on square_core,
// a group of E lanes per frame.  tw2d: the table of the E^2-point transform.
template <int E>
__global__ void __launch_bounds__(256)
k_acf_sq_f32(const float *__restrict__ x, float *__restrict__ r, int frames, int n, int p,
             const float2 *__restrict__ tw2d, const float *__restrict__ cs /* 2H cos, then 2H sin of 2 pi i / (2H) */)
{
    constexpr int H = E * E, F = 2 * H, GROUPS = 256 / E, PITCH = E + 1;
    __shared__ float bufs[GROUPS][E * PITCH];
    const int tid = threadIdx.x, grp = tid / E, lg = tid % E;
    const long t = (long)blockIdx.x * GROUPS + grp;
    if (t >= frames) return;
    const float *g = x + t * n;
    float *buf = bufs[grp];
    cf v[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        const int i0 = 2 * (lg + E * j);
        v[j].x = (j < E / 2 && i0 < n) ? g[i0] : 0.f;              // 2 m < H: the upper half of z is padding
        v[j].y = (j < E / 2 && i0 + 1 < n) ? g[i0 + 1] : 0.f;
    }
    square_core<E, false>(v, buf, tw2d, lg);                       // v[q] = Z[lg + E brevE(q)]
    const int lm = (E - lg) % E;
    float mx[E];
#pragma unroll
    for (int q = 0; q < E; q++) buf[brevE<E>(q) * PITCH + lg] = v[q].x;
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int j = brevE<E>(q);
        mx[q] = buf[lg ? (E - 1 - j) * PITCH + lm : ((E - j) % E) * PITCH];
    }
    OLS_WAVE_SYNC();
#pragma unroll
    for (int q = 0; q < E; q++) buf[brevE<E>(q) * PITCH + lg] = v[q].y;
    OLS_WAVE_SYNC();
    const float sc = 1.0f / (4.0f * (float)F);
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int j = brevE<E>(q);
        const int k = lg + E * j;
        const float my = buf[lg ? (E - 1 - j) * PITCH + lm : ((E - j) % E) * PITCH];
        const float wc = cs[k], ws = -cs[F + k];                   // W_F^k = (cos, -sin)
        const cf xe = {v[q].x + mx[q], v[q].y - my};
        const cf xo = {v[q].y + my, mx[q] - v[q].x};
        const cf T = cmul<false>(xo, cf{wc, ws});
        const cf a = cadd(xe, T), b = csub(xe, T);
        float sk = __builtin_fmaf(a.x, a.x, a.y * a.y) * sc, sm = __builtin_fmaf(b.x, b.x, b.y * b.y) * sc;
        if (k >= n) sk = 0.f;
        if (H - k >= n) sm = 0.f;
        if (k == 0) { sk *= 2.f; sm = 0.f; }
        const float dk = sk - sm;
        v[q] = cf{__builtin_fmaf(ws, dk, sk + sm), wc * dk};
    }
    OLS_WAVE_SYNC();
    cf u[E];
#pragma unroll
    for (int j = 0; j < E; j++) u[j] = v[brevE<E>(j)];
    square_core<E, true>(u, buf, tw2d, lg);                        // u[q] = g[lg + E brevE(q)]
    float *rr = r + t * (p + 1);
#pragma unroll
    for (int q = 0; q < E; q++) {
        const int m = lg + E * brevE<E>(q);
        if (2 * m <= p) rr[2 * m] = u[q].x;
        if (2 * m + 1 <= p) rr[2 * m + 1] = u[q].y;
    }
}

} // namespace

// fused FFT autocorrelation of `frames` frames of n float32 samples: fft length size = 2^ceil(log2(2n)) <= 4096
extern "C" int llzs_acf_fused_f32(const float *x, float *r, int frames, int n, int p, int size, const float *cs,
                                  void *stream)
{
    int log2n = 0;
    while ((1 << log2n) < size) log2n++;
    if (!x || !r || !cs || frames < 1 || n < 1 || p < 0 || p >= size || size < 8 || size > 4096 ||
        (1 << log2n) != size || 2 * n > size) {
        llzs_set_error("acf_fused_f32: bad arguments (n=%d p=%d size=%d)", n, p, size);
        return LLZ_ERR_ARG;
    }
    if ((size == 128 || size == 512) && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {   // the same on square_core (E = 8, 16)
        const int E = size == 128 ? 8 : 16;
        const float2 *sq = nullptr;                                           // the E^2-point table from the 2 E^2-point cs
        const int rc = fft_derived_tables(4, size, E, 2, false, cs, stream, "acf twiddle table", &sq, nullptr);
        if (rc != LLZ_OK) return rc;
        const unsigned blocks = (unsigned)((frames + (256 / E) - 1) / (256 / E));
        fft_pick_e<8, 16>(E, [&](auto e) {
            hipLaunchKernelGGL(k_acf_sq_f32<e()>, dim3(blocks), dim3(256), 0, as_stream(stream), x, r, frames, n, p, sq, cs);
        });
        LLZ_LAUNCH_CHECK("k_acf_sq_f32");
        return LLZ_OK;
    }
    if (size == 1024 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {
        hipLaunchKernelGGL(k_acf1024_f32, dim3((unsigned)((frames + 7) / 8)), dim3(256), 0, as_stream(stream), x, r, frames,
                           n, p, cs);
        LLZ_LAUNCH_CHECK("k_acf1024_f32");
        return LLZ_OK;
    }
    if (size == 2048 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {              // two real 2048-point transforms = two complex 1024-point ones
        hipLaunchKernelGGL(k_acf2048_f32, dim3((unsigned)((frames + 7) / 8)), dim3(256), 0, as_stream(stream), x, r,
                           frames, n, p, cs);
        LLZ_LAUNCH_CHECK("k_acf2048_f32");
        return LLZ_OK;
    }
    if (size == 4096 && llzs_tune(LLZS_TUNE_FFT_GENERIC) < 1) {              // one complex 2048-point transform on a whole wave
        hipLaunchKernelGGL(k_acf4096_f32, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, as_stream(stream), x, r,
                           frames, n, p, cs);
        LLZ_LAUNCH_CHECK("k_acf4096_f32");
        return LLZ_OK;
    }
    const fft_plan pl = fft_make_plan<arith_f32>(size, frames);
    if (pl.lds >= 64 * 1024)
        LLZ_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_acf_fused_f32),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    hipLaunchKernelGGL(k_acf_fused_f32, dim3((unsigned)pl.blocks), dim3(FFT_THREADS), pl.lds, as_stream(stream), x, r,
                       frames, n, p, size, log2n, cs, pl.tpw, fft_groups(log2n));
    LLZ_LAUNCH_CHECK("k_acf_fused_f32");
    return LLZ_OK;
}
