// Shared device/host helpers for the mmfm HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <math.h>

#include "../../include/mmfm.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __bf16 bf16_t;

// ------------------------------------------------------------------ errors (host)
int mmfm_set_error(int code, const char* fmt, ...);

#define MMFM_REQUIRE(cond, ...)                      \
    do {                                             \
        if (!(cond)) return mmfm_set_error(-1, __VA_ARGS__); \
    } while (0)

#define MMFM_LAUNCH_CHECK(name)                                                         \
    do {                                                                                \
        hipError_t e__ = hipGetLastError();                                             \
        if (e__ != hipSuccess)                                                          \
            return mmfm_set_error((int)e__, "%s: launch failed: %s", name, hipGetErrorString(e__)); \
    } while (0)

// Dynamic-LDS opt-in above 64 KB (hipFuncAttributeMaxDynamicSharedMemorySize), remembered per (device, kernel): the attribute belongs
// to the pair, so a process that drives several GPUs opts in on each (api.hip).  `what` names the entry point in the error text.
int mmfm_lds_opt_in(const void* kern, size_t bytes, const char* what);

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------ live rows (mmfm_gemm_live; include/mmfm.h)
// What a GEMM kernel gets beside its descriptor: rec == NULL is the plain launch.  kdim: the record sizes the reduction (dY^T.X), else M.
struct LiveArg {
    const int32_t* rec;
    int B, T, kdim;
};
static const LiveArg kNoLive = {nullptr, 0, 0, 0};
// the descriptor of the compact row space: M, or K with the split ranges, from the record (uniform: scalar loads)
__device__ __forceinline__ void live_patch(mmfm_gemm_desc& d, const LiveArg& lv) {
    if (!lv.rec) return;
    const int rows = lv.B * lv.rec[0];
    if (!lv.kdim) {
        d.M = rows;
    } else if (rows != d.K) {
        d.kchunk = d.splits > 1 ? ((rows + d.splits - 1) / d.splits + 63) / 64 * 64 : rows;      // the host's rounding (Engine._dw_split)
        d.K = rows;
    }
}
// the original row of compact row m (m < B * T_live): what the dropout counter is made of
__device__ __forceinline__ int live_orig_row(const LiveArg& lv, int m) {
    if (!lv.rec) return m;
    const int tl = lv.rec[0], b = m / tl;
    return b * lv.T + lv.rec[4 + m - b * tl];
}

// ------------------------------------------------------------------ bf16 <-> f32
__device__ __forceinline__ float bf2f(uint16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
    bf16_t b = (bf16_t)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return *reinterpret_cast<uint16_t*>(&b);
}

// ------------------------------------------------------------------ streaming (non-temporal) stores
// Activation outputs are written once and read by a LATER kernel: a plain store write-allocates in the XCD's 4 MB L2 and
// evicts the operand panels co-resident workgroups are about to re-read.  Measured on the bf16 GEMM at B = 1024 (x.W^T,
// qkv): 201 -> 163 us with the output stored non-temporally; up-projection 133 -> 107 us.
typedef __attribute__((ext_vector_type(4))) unsigned int mmfm_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int mmfm_u32x2;
typedef __attribute__((ext_vector_type(4))) float mmfm_f32x4;
__device__ __forceinline__ void st_stream(uint4* p, uint4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(mmfm_u32x4, v), reinterpret_cast<mmfm_u32x4*>(p));
}
__device__ __forceinline__ void st_stream(uint2* p, uint2 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(mmfm_u32x2, v), reinterpret_cast<mmfm_u32x2*>(p));
}
__device__ __forceinline__ void st_stream(float4* p, float4 v) {
    __builtin_nontemporal_store(__builtin_bit_cast(mmfm_f32x4, v), reinterpret_cast<mmfm_f32x4*>(p));
}

template <typename T> struct io;
template <> struct io<float> {
    static __device__ __forceinline__ float ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
    static __device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
    static __device__ __forceinline__ void st4s(float* p, float4 v) { st_stream(reinterpret_cast<float4*>(p), v); }
};
template <> struct io<uint16_t> {  // bf16 storage
    static __device__ __forceinline__ float ld(const uint16_t* p) { return bf2f(*p); }
    static __device__ __forceinline__ void st(uint16_t* p, float v) { *p = f2bf(v); }
    static __device__ __forceinline__ float4 ld4(const uint16_t* p) {
        uint2 u = *reinterpret_cast<const uint2*>(p);
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                           __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    }
    static __device__ __forceinline__ void st4(uint16_t* p, float4 v) {
        uint2 u;
        u.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
        u.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
        *reinterpret_cast<uint2*>(p) = u;
    }
    static __device__ __forceinline__ void st4s(uint16_t* p, float4 v) {
        uint2 u;
        u.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
        u.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
        st_stream(reinterpret_cast<uint2*>(p), u);
    }
};

// ------------------------------------------------------------------ counter-based dropout RNG
// keep(idx) is a pure function of (state[0], state[1], site, idx): the backward pass regenerates
// the forward's mask instead of storing it.  `state` lives in device memory so a captured
// hipGraph sees a fresh stream every replay (mmfm_rng_advance bumps state[1]).
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
// One hash decides a PAIR of neighbouring elements (even index: low 16 bits, odd index: high 16 bits, each compared with
// the top 16 bits of the threshold: p is honoured to 2^-16).  The mixer is xorshift / 24-bit multiply: v_mul_u32_u24 issues at
// the full VALU rate, v_mul_lo_u32 at a quarter of it, and a step draws ~10^9 decisions.  (Round 1 used two murmur-style
// 32-bit finalisers per ELEMENT: 4 quarter-rate multiplies + 12 ops = ~110 cycles per decision at one wave per SIMD, which
// was 7k cycles of every 128x128 GEMM tile epilogue with dropout and 14k cycles of every fused-MLP row pass.)
struct Drop {
    uint32_t k0, k1, thresh, t16;
    float scale;
    __device__ __forceinline__ bool on() const { return thresh != 0; }
    __device__ __forceinline__ uint32_t hash(uint32_t pidx) const {
        uint32_t h = pidx ^ k0;
        h ^= h >> 16;
        // v_mul_u32_u24 sees bits 0..23 only: the top byte enters through its own multiply (an additive, non-cancelling term).
        // Without it hash(p) == hash(p ^ (d << 24 | d << 8)) for every d: tensors beyond 2^25 elements repeated their masks.
        h = __umul24(h, 0x7FEB35u) + (__umul24(h >> 24, 0x9E3779u) + k1);
        h ^= h >> 13;
        h = __umul24(h, 0x46CA6Bu) ^ (h >> 9);
        h ^= h >> 16;
        return h;
    }
    // hash of the pair that holds element idx (idx and idx ^ 1 share it)
    __device__ __forceinline__ uint32_t pair(uint64_t idx) const {
        return hash((uint32_t)(idx >> 1) + __umul24((uint32_t)(idx >> 33), 0x9E3779u));
    }
    __device__ __forceinline__ bool lo(uint32_t h) const { return (h & 0xffffu) >= t16; }     // even element of the pair
    __device__ __forceinline__ bool hi(uint32_t h) const { return (h >> 16) >= t16; }         // odd element
    __device__ __forceinline__ bool keep(uint64_t idx) const {
        const uint32_t h = pair(idx);
        return ((idx & 1) ? (h >> 16) : (h & 0xffffu)) >= t16;
    }
    __device__ __forceinline__ float apply(float v, uint64_t idx) const {
        return on() ? (keep(idx) ? v * scale : 0.f) : v;
    }
    // elements idx (even) and idx + 1 with one hash
    __device__ __forceinline__ void apply2(float& v0, float& v1, uint64_t idx_even) const {
        const uint32_t h = pair(idx_even);
        v0 = lo(h) ? v0 * scale : 0.f;
        v1 = hi(h) ? v1 * scale : 0.f;
    }
};
__device__ __forceinline__ Drop drop_init(mmfm_dropout d) {
    Drop r;
    if (d.p <= 0.f || d.state == nullptr) { r.k0 = r.k1 = r.thresh = r.t16 = 0; r.scale = 1.f; return r; }
    const uint32_t* s = reinterpret_cast<const uint32_t*>(d.state);
    r.k0 = mix32(s[0] + d.site * 0x9E3779B9u);
    r.k1 = mix32(s[1] ^ (d.site * 0x85EBCA6Bu + 0xC2B2AE35u));
    double t = (double)d.p * 4294967296.0;
    r.thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    r.t16 = r.thresh >> 16;
    r.scale = 1.f / (1.f - d.p);
    return r;
}

// ------------------------------------------------------------------ attention workgroup -> (batch, head)
// One workgroup per (b, head) reads dh-wide slices of [.., heads*dh] rows: with dh = 32 a 128-B line holds TWO heads, and the
// dispatcher deals consecutive workgroups round-robin over the 8 XCDs, so the heads of one sample landed on 8 different L2s and
// every line was fetched from HBM once per head that touches it (PMC round 1: 631 MB fetched for 315 MB of q/k/v).  The bijective
// XCD remap (cdna_hip_programming.md T1) gives every XCD a contiguous range of (b, head) ids: the heads of a sample run on one
// XCD, back to back, and share its L2.  MMFM_ATTN_NO_REMAP bit (flags & 0x100) restores the plain order for A/B runs.
__device__ __forceinline__ int attn_xcd_remap(int bid, int nwg, int flags) {
    if (flags & 0x100) return bid;
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ------------------------------------------------------------------ attention window (MMFM_ATTN_WINDOW)
// The general attention kernels take the window as a template flag plus a trailing argument pack (empty without a window, one
// mmfm_attn_window with it), the way the segment forms ride on the LayerNorm template: the instantiations without a window keep their
// argument list and their code.  win_stage puts the sample's pos row into LDS behind the mod_id bytes (4-byte aligned; the LDS formulas
// beside the kernels add attn_win_lds(L) for it) and hands back the row and the interval; the caller's barrier publishes it.
struct AttnWin { const int32_t* pos; int lo, hi; };     // pos == nullptr: no window (a literal in those instantiations: the term folds away)
inline size_t attn_win_lds(bool win, int L) { return win ? (size_t)4 * L + 4 : 0; }
template <bool WIN, typename... W>
__device__ __forceinline__ AttnWin win_stage(uint8_t* modl, int Lmx, int b, int L, int t, int nthreads, W... w) {
    if constexpr (WIN) {
        const mmfm_attn_window win[1] = {w...};
        int32_t* p = reinterpret_cast<int32_t*>(modl + ((Lmx + 3) & ~3));
        for (int i = t; i < L; i += nthreads) p[i] = win[0].pos[(size_t)b * L + i];
        return AttnWin{p, win[0].lo, win[0].hi};
    } else {
        return AttnWin{nullptr, 0, 0};
    }
}
__device__ __forceinline__ bool win_allows(const AttnWin& w, int q, int k) {
    const int dlt = w.pos[k] - w.pos[q];
    return dlt >= w.lo && dlt <= w.hi;
}

// ------------------------------------------------------------------ activations
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * __expf(-0.5f * x * x);
}
// bf16-mode GELU: Phi(x) = 0.5 + x~ P(x~^2), x~ = clamp(x, -4, 4), P a degree-9 near-minimax polynomial: no transcendental,
// every step is a packed fp32 op on a PAIR of values (v_pk_mul_f32 / v_pk_fma_f32).  |Phi error| <= 3.4e-5 everywhere
// (|gelu error| <= 1.9e-5 on [-4, 4], |x| * 3e-5 beyond), against the 2^-9 relative step of the bf16 value it feeds.
// erff + expf (gelu_erf / gelu_erf_grad below, kept for the fp32 parity kernels) are ~60 VALU ops and 2-3 quarter-rate
// transcendentals per element; this is 7 ops per element.  Measured: see DESIGN.md 3b.
typedef float mmfm_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ mmfm_f32x2 splat2(float v) { mmfm_f32x2 r; r.x = v; r.y = v; return r; }
__device__ __forceinline__ mmfm_f32x2 phi2(mmfm_f32x2 x) {
    mmfm_f32x2 xc;
    xc.x = __builtin_amdgcn_fmed3f(x.x, -4.f, 4.f);
    xc.y = __builtin_amdgcn_fmed3f(x.y, -4.f, 4.f);
    const mmfm_f32x2 t = xc * xc;
    mmfm_f32x2 p = splat2(-4.407132645e-12f);
    p = __builtin_elementwise_fma(p, t, splat2(4.129891984e-10f));
    p = __builtin_elementwise_fma(p, t, splat2(-1.754582968e-08f));
    p = __builtin_elementwise_fma(p, t, splat2(4.542657450e-07f));
    p = __builtin_elementwise_fma(p, t, splat2(-8.172721209e-06f));
    p = __builtin_elementwise_fma(p, t, splat2(1.105528936e-04f));
    p = __builtin_elementwise_fma(p, t, splat2(-1.176239806e-03f));
    p = __builtin_elementwise_fma(p, t, splat2(9.960514493e-03f));
    p = __builtin_elementwise_fma(p, t, splat2(-6.648434699e-02f));
    p = __builtin_elementwise_fma(p, t, splat2(3.989418149e-01f));
    return __builtin_elementwise_fma(xc, p, splat2(0.5f));
}
__device__ __forceinline__ mmfm_f32x2 gelu2(mmfm_f32x2 x) { return x * phi2(x); }
__device__ __forceinline__ mmfm_f32x2 gelu_grad2(mmfm_f32x2 x) {             // Phi(x) + x phi(x)
    const mmfm_f32x2 t = x * x * splat2(-0.72134752044448170f);
    mmfm_f32x2 e;
    e.x = __builtin_amdgcn_exp2f(t.x);
    e.y = __builtin_amdgcn_exp2f(t.y);
    return __builtin_elementwise_fma(x * splat2(0.39894228040143268f), e, phi2(x));
}
__device__ __forceinline__ void gelu_both2(mmfm_f32x2 x, mmfm_f32x2& g, mmfm_f32x2& dg) {     // gelu(x) and gelu'(x), one Phi
    const mmfm_f32x2 ph = phi2(x), t = x * x * splat2(-0.72134752044448170f);
    mmfm_f32x2 e;
    e.x = __builtin_amdgcn_exp2f(t.x);
    e.y = __builtin_amdgcn_exp2f(t.y);
    g = x * ph;
    dg = __builtin_elementwise_fma(x * splat2(0.39894228040143268f), e, ph);
}
__device__ __forceinline__ float gelu_poly(float x) { return gelu2(splat2(x)).x; }
__device__ __forceinline__ float gelu_poly_grad(float x) { return gelu_grad2(splat2(x)).x; }
// in place on an even-length array
template <int N> __device__ __forceinline__ void gelu_n(float* v) {
#pragma unroll
    for (int i = 0; i < N; i += 2) { mmfm_f32x2 a; a.x = v[i]; a.y = v[i + 1]; a = gelu2(a); v[i] = a.x; v[i + 1] = a.y; }
}
template <int N> __device__ __forceinline__ void mul_gelu_grad_n(float* v, const float* u) {      // v *= gelu'(u)
#pragma unroll
    for (int i = 0; i < N; i += 2) {
        mmfm_f32x2 a; a.x = u[i]; a.y = u[i + 1];
        a = gelu_grad2(a);
        v[i] *= a.x; v[i + 1] *= a.y;
    }
}
// ---- the other MLP activations (transformer.act): mmfm_gemm act 6-11, mmfm_mlp_desc.act (MMFM_MLP_*)
//   relu       max(u, 0)                      f' = 1 if u > 0 else 0 (0 at u = 0, as torch)
//   sigmoid    u s, s = sigmoid(b u)          f' = s + b u s (1 - s)          silu / swish (b = 1), quick_gelu (b = 1.702)
//   gelu_tanh  0.5 u (1 + t), t = tanh(z)     f' = 0.5 (1 + t) + 0.5 u (1 - t^2) z'(u),  z = k (u + c u^3), k = sqrt(2 / pi), c = 0.044715
// The derivatives are taken at a clamped argument (|b u| <= 200, |u| <= 20): beyond it s, t are exactly 0 / 1 / -1 in fp32, so f' is
// exactly 0 or 1 there, and the clamp keeps b u * s (1 - s) and u (1 - t^2) u^2 away from inf * 0 for every finite u.  The forwards
// multiply the unclamped u by the gate taken at the clamped argument (the same value).
constexpr float kActSigClamp = 200.f, kActTanhClamp = 20.f;
constexpr float kGeluTanhK = 0.79788456080286536f, kGeluTanhC = 0.044715f;
// fp32 parity kernels (gemm.hip) and the scalar bf16 epilogue: sigmoid(z) = rcp(1 + __expf(-z)) (v_exp_f32 / v_rcp_f32: about 1e-6
// relative, against the 1e-4 parity bound); tanh-GELU through 0.5 (1 + tanh z) = sigmoid(2 z), as the packed forms below.  (expf /
// tanhf: their library slow paths cost the fp32 GEMM kernels 320 B of scratch.)
template <int A> struct ActAcc;
template <> struct ActAcc<MMFM_MLP_GELU> {
    static __device__ __forceinline__ float f(float u, float) { return gelu_erf(u); }
    static __device__ __forceinline__ float grad(float u, float) { return gelu_erf_grad(u); }
};
template <> struct ActAcc<MMFM_MLP_RELU> {
    static __device__ __forceinline__ float f(float u, float) { return fmaxf(u, 0.f); }
    static __device__ __forceinline__ float grad(float u, float) { return u > 0.f ? 1.f : 0.f; }
};
template <> struct ActAcc<MMFM_MLP_SIGMOID> {
    static __device__ __forceinline__ float f(float u, float b) {
        return u * __builtin_amdgcn_rcpf(1.f + __expf(-__builtin_amdgcn_fmed3f(b * u, -kActSigClamp, kActSigClamp)));
    }
    static __device__ __forceinline__ float grad(float u, float b) {
        const float z = __builtin_amdgcn_fmed3f(b * u, -kActSigClamp, kActSigClamp), s = __builtin_amdgcn_rcpf(1.f + __expf(-z));
        return fmaf(z * s, 1.f - s, s);
    }
};
template <> struct ActAcc<MMFM_MLP_GELU_TANH> {
    static __device__ __forceinline__ float f(float u, float) {
        const float x = __builtin_amdgcn_fmed3f(u, -kActTanhClamp, kActTanhClamp);
        return u * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * kGeluTanhK * fmaf(kGeluTanhC * x * x, x, x)));
    }
    static __device__ __forceinline__ float grad(float u, float) {      // h + 2 u h (1 - h) z'(u), h = sigmoid(2 z)
        const float x = __builtin_amdgcn_fmed3f(u, -kActTanhClamp, kActTanhClamp), x2 = x * x;
        const float h = __builtin_amdgcn_rcpf(1.f + __expf(-2.f * kGeluTanhK * fmaf(kGeluTanhC * x2, x, x)));
        return fmaf(2.f * kGeluTanhK * x * h * (1.f - h), fmaf(3.f * kGeluTanhC, x2, 1.f), h);
    }
};
// mmfm_gemm act 6 / 7 -> MMFM_MLP_RELU, 8 / 9 -> _SIGMOID, 10 / 11 -> _GELU_TANH, 12 .. 25 (the embedder activations, below) -> kActEmbed
// (0 for every other act)
constexpr int kActEmbed = 4, kActEmbedFirst = 12, kActEmbedLast = 25, kActEmbedIdentityGrad = 13;
__host__ __device__ __forceinline__ int gemm_act_kind(int act) { return act >= kActEmbedFirst ? kActEmbed : (act >= 6 ? (act - 4) >> 1 : 0); }

// bf16-mode (packed, fast) forms: sigmoid(z) = 1 / (1 + 2^(-z log2 e)) through v_exp_f32 and v_rcp_f32 (1 ulp each); 2^x overflows to inf
// or underflows to 0 at the ends and rcp(inf) = 0, so s is exactly 0 or 1 there.  tanh-GELU uses 0.5 (1 + tanh(z)) = sigmoid(2 z) and
// 1 - t^2 = 4 h (1 - h), h = sigmoid(2 z): f = u h,  f' = h + 2 u h (1 - h) z'(u).  Error bounds: DESIGN.md 3g.
__device__ __forceinline__ mmfm_f32x2 clamp2(mmfm_f32x2 x, float c) {
    mmfm_f32x2 r;
    r.x = __builtin_amdgcn_fmed3f(x.x, -c, c);
    r.y = __builtin_amdgcn_fmed3f(x.y, -c, c);
    return r;
}
__device__ __forceinline__ mmfm_f32x2 sigmoid2(mmfm_f32x2 z) {
    const mmfm_f32x2 t = z * splat2(-1.4426950408889634f);
    mmfm_f32x2 r;
    r.x = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(t.x));
    r.y = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(t.y));
    return r;
}
// MlpAct<A>: f(u), f'(u) and both at once for a pair of values; b = the sigmoid kind's beta (unused by the others).
// MlpAct<MMFM_MLP_GELU> is the polynomial GELU above, unchanged.
template <int A> struct MlpAct;
template <> struct MlpAct<MMFM_MLP_GELU> {
    static __device__ __forceinline__ mmfm_f32x2 f(mmfm_f32x2 x, float) { return gelu2(x); }
    static __device__ __forceinline__ mmfm_f32x2 grad(mmfm_f32x2 x, float) { return gelu_grad2(x); }
    static __device__ __forceinline__ void both(mmfm_f32x2 x, float, mmfm_f32x2& g, mmfm_f32x2& dg) { gelu_both2(x, g, dg); }
};
template <> struct MlpAct<MMFM_MLP_RELU> {
    static __device__ __forceinline__ mmfm_f32x2 f(mmfm_f32x2 x, float) {
        mmfm_f32x2 r; r.x = fmaxf(x.x, 0.f); r.y = fmaxf(x.y, 0.f); return r;
    }
    static __device__ __forceinline__ mmfm_f32x2 grad(mmfm_f32x2 x, float) {
        mmfm_f32x2 r; r.x = x.x > 0.f ? 1.f : 0.f; r.y = x.y > 0.f ? 1.f : 0.f; return r;
    }
    static __device__ __forceinline__ void both(mmfm_f32x2 x, float b, mmfm_f32x2& g, mmfm_f32x2& dg) { g = f(x, b); dg = grad(x, b); }
};
template <> struct MlpAct<MMFM_MLP_SIGMOID> {
    static __device__ __forceinline__ void both(mmfm_f32x2 x, float b, mmfm_f32x2& g, mmfm_f32x2& dg) {
        const mmfm_f32x2 z = clamp2(x * splat2(b), kActSigClamp), s = sigmoid2(z);
        g = x * s;
        dg = s * __builtin_elementwise_fma(z, splat2(1.f) - s, splat2(1.f));
    }
    static __device__ __forceinline__ mmfm_f32x2 f(mmfm_f32x2 x, float b) { return x * sigmoid2(clamp2(x * splat2(b), kActSigClamp)); }
    static __device__ __forceinline__ mmfm_f32x2 grad(mmfm_f32x2 x, float b) { mmfm_f32x2 g, dg; both(x, b, g, dg); return dg; }
};
template <> struct MlpAct<MMFM_MLP_GELU_TANH> {
    static __device__ __forceinline__ void both(mmfm_f32x2 x, float, mmfm_f32x2& g, mmfm_f32x2& dg) {
        const mmfm_f32x2 xc = clamp2(x, kActTanhClamp), x2 = xc * xc;
        const mmfm_f32x2 h = sigmoid2(xc * __builtin_elementwise_fma(x2, splat2(2.f * kGeluTanhK * kGeluTanhC), splat2(2.f * kGeluTanhK)));
        g = x * h;
        const mmfm_f32x2 dz = __builtin_elementwise_fma(x2, splat2(6.f * kGeluTanhK * kGeluTanhC), splat2(2.f * kGeluTanhK));   // d(2z)/du
        dg = h * __builtin_elementwise_fma(xc * dz, splat2(1.f) - h, splat2(1.f));
    }
    static __device__ __forceinline__ mmfm_f32x2 f(mmfm_f32x2 x, float) {
        const mmfm_f32x2 xc = clamp2(x, kActTanhClamp), x2 = xc * xc;
        return x * sigmoid2(xc * __builtin_elementwise_fma(x2, splat2(2.f * kGeluTanhK * kGeluTanhC), splat2(2.f * kGeluTanhK)));
    }
    static __device__ __forceinline__ mmfm_f32x2 grad(mmfm_f32x2 x, float b) { mmfm_f32x2 g, dg; both(x, b, g, dg); return dg; }
};
// mmfm_gemm act 6..11 in the bf16 epilogues (kind A = gemm_act_kind(act)): in place on an even-length array / v *= f'(u)
template <int A, int N> __device__ __forceinline__ void mlp_act_n(float* v, float b) {
#pragma unroll
    for (int i = 0; i < N; i += 2) { mmfm_f32x2 a; a.x = v[i]; a.y = v[i + 1]; a = MlpAct<A>::f(a, b); v[i] = a.x; v[i + 1] = a.y; }
}
template <int A, int N> __device__ __forceinline__ void mul_mlp_act_grad_n(float* v, const float* u, float b) {
#pragma unroll
    for (int i = 0; i < N; i += 2) {
        if constexpr (A == MMFM_MLP_RELU) {           // a select, as torch's threshold backward
            v[i] = u[i] > 0.f ? v[i] : 0.f; v[i + 1] = u[i + 1] > 0.f ? v[i + 1] : 0.f;
        } else {
            mmfm_f32x2 a; a.x = u[i]; a.y = u[i + 1];
            a = MlpAct<A>::grad(a, b);
            v[i] *= a.x; v[i + 1] *= a.y;
        }
    }
}
// one element (the scalar epilogue of gemm_bf16.hip): f(v), and f'(u)
template <int A> __device__ __forceinline__ float mlp_act1(float v, float b) { return ActAcc<A>::f(v, b); }
template <int A> __device__ __forceinline__ float mlp_act_grad1(float u, float b) { return ActAcc<A>::grad(u, b); }
__device__ __forceinline__ float softsign_f(float x) { return x / (1.f + fabsf(x)); }
__device__ __forceinline__ float softsign_grad(float x) { float d = 1.f + fabsf(x); return 1.f / (d * d); }
// the same derivative from the activation's OUTPUT y = s * x / (1 + |x|):  1 / (1 + |x|) = 1 - |y| / s  (act 5: the tokeniser's
// backward reads the activation it needs anyway instead of a second, saved [rows, 1336] pre-activation tensor)
// Error bound (tests/test_kernels_gpu.py::test_gemm_act5_softsign_grad_from_output_error_bound): y is stored in bf16, so r = 1 - |y| / s carries
// an absolute error of up to 2^-9 and the factor r^2 a RELATIVE error of about 0.6 % x (1 + |x|) - 5 % at |x| = 8, the whole value beyond |x| ~ 170
// (y rounds to s, the gradient reads 0 where the true factor is < 4e-5).  Spike-count pre-activations of the tokenisers sit at |x| of a few units.
__device__ __forceinline__ float softsign_grad_from_out(float y, float inv_s) { const float r = 1.f - fabsf(y) * inv_s; return r * r; }

// ---- the embedder activations (embedder.act other than softsign): mmfm_gemm act 12 .. 25, forward (even) / gradient (odd) pairs
//   forward  v = f(v) * act_scale            gradient  v *= f'(u) * act_scale,  u = the saved pre-activation (gradmul_pre)
// f = (act - 12) >> 1:  0 identity (its gradient reads no u), 1 relu, 2 GELU (erf in fp32, the polynomial in bf16, as act 1 / 3),
// 3 u sigmoid(u) (silu / swish), 4 u sigmoid(1.702 u) (quick_gelu), 5 tanh-GELU, 6 tanh.  act_scale is the embedder's `scale` - acts 6-11
// spend it on beta - so the two sigmoid gates are codes of their own.  All of them run in ONE kernel instantiation per site (template
// kind kActEmbed, the function picked by a wave-uniform switch, embed_dispatch): the kernels of every other act keep their code.  They are the functions
// of acts 1 / 3 / 6-11; only tanh is new: (1 - e) / (1 + e), e = exp(-2 |u|) (fp32 kernels; absolute error ~1e-7) and 2 sigmoid(2 u) - 1
// in the packed bf16 forms, tanh' = 1 - t^2 = 4 h (1 - h), h = sigmoid(2 u): e / h saturate to exactly 0 / 1, no clamp is needed.
__device__ __forceinline__ float tanh_acc(float x) {
    const float e = __expf(-2.f * fabsf(x));
    return copysignf((1.f - e) * __builtin_amdgcn_rcpf(1.f + e), x);
}
// F is a compile-time constant inside the epilogues: embed_dispatch turns the wave-uniform act code into it ONCE per epilogue, outside the
// unrolled element loops (a switch inside them keeps hipcc from unrolling, and the accumulators it then indexes go to scratch)
template <int F> struct EmbedF { static constexpr int value = F; };
template <typename Fn> __device__ __forceinline__ void embed_dispatch(int act, Fn&& fn) {
    switch ((act - kActEmbedFirst) >> 1) {
    case 0: fn(EmbedF<0>{}); break;
    case 1: fn(EmbedF<1>{}); break;
    case 2: fn(EmbedF<2>{}); break;
    case 3: fn(EmbedF<3>{}); break;
    case 4: fn(EmbedF<4>{}); break;
    case 5: fn(EmbedF<5>{}); break;
    default: fn(EmbedF<6>{}); break;
    }
}
template <int F> constexpr float embed_beta() { return F == 4 ? 1.702f : 1.f; }
template <bool POLY, int F> __device__ __forceinline__ float embed_act1(float v) {
    if constexpr (F == 0) return v;
    else if constexpr (F == 1) return fmaxf(v, 0.f);
    else if constexpr (F == 2) return POLY ? gelu_poly(v) : gelu_erf(v);
    else if constexpr (F == 3 || F == 4) return ActAcc<MMFM_MLP_SIGMOID>::f(v, embed_beta<F>());
    else if constexpr (F == 5) return ActAcc<MMFM_MLP_GELU_TANH>::f(v, 1.f);
    else return tanh_acc(v);
}
// v * f'(u) (relu: a select, as torch's threshold backward; identity reads no u)
template <bool POLY, int F> __device__ __forceinline__ float embed_mul_grad1(float v, float u) {
    if constexpr (F == 0) return v;
    else if constexpr (F == 1) return u > 0.f ? v : 0.f;
    else if constexpr (F == 2) return v * (POLY ? gelu_poly_grad(u) : gelu_erf_grad(u));
    else if constexpr (F == 3 || F == 4) return v * ActAcc<MMFM_MLP_SIGMOID>::grad(u, embed_beta<F>());
    else if constexpr (F == 5) return v * ActAcc<MMFM_MLP_GELU_TANH>::grad(u, 1.f);
    else { const float t = tanh_acc(u); return v * fmaf(-t, t, 1.f); }
}
// the packed bf16-mode forms on an even-length array: v = f(v) * s in place / v *= f'(u) * s
template <int N, int F> __device__ __forceinline__ void embed_act_n(float* v, float s) {
    if constexpr (F == 1) mlp_act_n<MMFM_MLP_RELU, N>(v, 1.f);
    else if constexpr (F == 2) gelu_n<N>(v);
    else if constexpr (F == 3 || F == 4) mlp_act_n<MMFM_MLP_SIGMOID, N>(v, embed_beta<F>());
    else if constexpr (F == 5) mlp_act_n<MMFM_MLP_GELU_TANH, N>(v, 1.f);
    else if constexpr (F == 6) {
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            mmfm_f32x2 a; a.x = v[i]; a.y = v[i + 1];
            a = __builtin_elementwise_fma(sigmoid2(a * splat2(2.f)), splat2(2.f), splat2(-1.f));
            v[i] = a.x; v[i + 1] = a.y;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] *= s;
}
template <int N, int F> __device__ __forceinline__ void embed_mul_grad_n(float* v, const float* u, float s) {
    if constexpr (F == 1) mul_mlp_act_grad_n<MMFM_MLP_RELU, N>(v, u, 1.f);
    else if constexpr (F == 2) mul_gelu_grad_n<N>(v, u);
    else if constexpr (F == 3 || F == 4) mul_mlp_act_grad_n<MMFM_MLP_SIGMOID, N>(v, u, embed_beta<F>());
    else if constexpr (F == 5) mul_mlp_act_grad_n<MMFM_MLP_GELU_TANH, N>(v, u, 1.f);
    else if constexpr (F == 6) {
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            mmfm_f32x2 a; a.x = u[i]; a.y = u[i + 1];
            const mmfm_f32x2 h = sigmoid2(a * splat2(2.f));
            a = splat2(4.f) * h * (splat2(1.f) - h);
            v[i] *= a.x; v[i + 1] *= a.y;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] *= s;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
