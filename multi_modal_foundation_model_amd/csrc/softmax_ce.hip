// Softmax cross-entropy for categorical modalities (MMFM_LOSS_SOFTMAX_CE; include/mmfm.h), forward reduction and
// backward, and the arg-max confusion matrix of the evaluation metrics.  The first loss whose row elements are coupled (a log-sum-exp),
// so it has kernels of its own beside csrc/loss.hip's elementwise template:
//   t'[c] = (1 - eps) t[c] + eps / N      e[c] = w[c] t'[c] (lse(p) - p[c])      d/dp[j] = softmax(p)[j] sum_c w[c] t'[c] - w[j] t'[j]
// Rows are short (2 .. 16 classes is the usual case): a row is owned by a group of G lanes, G the smallest power of two >= min(N, 64),
// and 64 / G rows share a wavefront; for N > 64 (G = 64) the wavefront owns the row and its lanes stride over the columns, keeping up
// to 16 columns each in registers (the row is read once; wider rows are streamed pass by pass).  Maximum,
// exp-sum and the weight sum are reduced inside the group by xor-exchange in a fixed order; the maximum is subtracted before the
// exponential.  Un-masked rows are never read.  fp32 arithmetic with contraction off - every multiply-add that is fused is an
// explicit fmaf - so that the backward's recomputed row statistics are the forward's bits; fixed-order two-stage sum (bitwise
// reproducible), no allocation, no sync, no floating-point atomics.
#include "common.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace {

template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int G> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// what a kernel needs of the loss besides the row: class weights (NULL: 1) and the two smoothing constants
struct CeArgs {
    const float* cw;
    float k1, k0;          // t' = fmaf(k1, t, k0): k1 = 1 - eps, k0 = eps / N (eps == 0: t' is t, bit for bit)
    __device__ __forceinline__ float wt(const float* __restrict__ trow, int c) const {
        const float tp = fmaf(k1, trow[c], k0);
        return cw ? cw[c] * tp : tp;
    }
};

// A lane's share of its row.  K > 0: the lane keeps its K columns (col, col + G, ...) of logits and of w t' in registers - the row is
// read once, one memory latency per row instead of one per pass.  K == 0: rows wider than 64 * 16 columns are streamed, one pass per
// reduction (the re-reads hit the cache).  A slot without a column, or of an un-masked or absent row, holds (-inf, 0) and is never loaded.
template <typename T, int G, int K> struct RowRegs {
    float p[K > 0 ? K : 1], w[K > 0 ? K : 1];
    __device__ __forceinline__ void load(const CeArgs& a, const T* __restrict__ prow, const float* __restrict__ trow, bool on, int col, int N) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = col + k * G;
            const bool live = on && c < N;
            p[k] = live ? io<T>::ld(prow + c) : -INFINITY;
            w[k] = live ? a.wt(trow, c) : 0.f;
        }
    }
};

// (max, exp-sum, sum w t') of the row this lane's group owns; every lane of the wavefront calls it (the exchanges are outside the
// `on` branches), lanes of un-masked or absent rows contribute nothing and get nothing meaningful back
template <typename T, int G, int K>
__device__ __forceinline__ void row_stats(const CeArgs& a, const RowRegs<T, G, K>& r, const T* __restrict__ prow, const float* __restrict__ trow,
                                          bool on, int col, int N, float& m, float& s, float& swt) {
    m = -INFINITY;
    if constexpr (K > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) m = fmaxf(m, r.p[k]);
    } else if (on) {
        for (int c = col; c < N; c += G) m = fmaxf(m, io<T>::ld(prow + c));
    }
    m = group_max<G>(m);
    s = 0.f, swt = 0.f;
    if (on) {
        if constexpr (K > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {          // an empty slot adds exp(-inf) = 0 and w = 0: nothing
                s += __expf(r.p[k] - m);
                swt += r.w[k];
            }
        } else {
            for (int c = col; c < N; c += G) {
                s += __expf(io<T>::ld(prow + c) - m);
                swt += a.wt(trow, c);
            }
        }
    }
    s = group_sum<G>(s);
    swt = group_sum<G>(swt);
}

template <typename T, int G, int K>
__global__ __launch_bounds__(256) void ce_fwd_kernel(CeArgs a, const T* __restrict__ pred, const float* __restrict__ target,
                                                     const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                     float* __restrict__ part, float* __restrict__ rowstat) {
    constexpr int RPW = 64 / G;                    // rows per wavefront
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G, col = lane % G;
    float acc = 0.f;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * RPW; base < R; base += (int64_t)gridDim.x * 4 * RPW) {
        const int64_t row = base + sub;
        const bool on = row < R && rowmask[(row / Tn) * mask_ld + (row % Tn)] != 0;
        if (__ballot(on) == 0) continue;           // wave-uniform
        const T* prow = pred + (size_t)row * N;
        const float* trow = target + (size_t)row * N;
        RowRegs<T, G, K> r;
        r.load(a, prow, trow, on, col, N);
        float m, s, swt;
        row_stats<T, G, K>(a, r, prow, trow, on, col, N, m, s, swt);
        if (on) {
            const float ls = logf(s);              // s in [1, N]: lse - p = (m - p) + log s, every term of the row sum >= 0
            if constexpr (K > 0) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (col + k * G < N) acc += r.w[k] * ((m - r.p[k]) + ls);
            } else {
                for (int c = col; c < N; c += G) acc += a.wt(trow, c) * ((m - io<T>::ld(prow + c)) + ls);
            }
            if (rowstat && col == 0) { rowstat[2 * row] = m + ls; rowstat[2 * row + 1] = swt; }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void ce_sum_kernel(const float* __restrict__ part, int n, float* out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}

// SAVED: (lse, sum w t') come from the forward's rowstat - no reduction, every element on its own: the row is streamed (K unused, 0).
// Otherwise the statistics are the forward's computation again, on the forward's register form, to the same bits.
template <typename T, int G, int K, bool SAVED>
__global__ __launch_bounds__(256) void ce_bwd_kernel(CeArgs a, const T* __restrict__ pred, const float* __restrict__ target,
                                                     const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                     const float* __restrict__ rowstat, const float* __restrict__ grad_out,
                                                     const float* __restrict__ inv_n, T* __restrict__ dpred) {
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G, col = lane % G;
    const float g = grad_out[0] * inv_n[0];
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * RPW; base < R; base += (int64_t)gridDim.x * 4 * RPW) {
        const int64_t row = base + sub;
        const bool valid = row < R, on = valid && rowmask[(row / Tn) * mask_ld + (row % Tn)] != 0;
        const T* prow = pred + (size_t)row * N;
        const float* trow = target + (size_t)row * N;
        T* drow = dpred + (size_t)row * N;
        RowRegs<T, G, K> r;
        float lse = 0.f, swt = 0.f;
        if constexpr (SAVED) {
            if (on) { lse = rowstat[2 * row]; swt = rowstat[2 * row + 1]; }
        } else if (__ballot(on) != 0) {            // wave-uniform
            float m, s;
            r.load(a, prow, trow, on, col, N);
            row_stats<T, G, K>(a, r, prow, trow, on, col, N, m, s, swt);
            lse = m + logf(s);
        }
        if (!valid) continue;
        // un-masked rows: mask * g with mask = 0 - i.e. 0 normally, NaN when nothing at all is masked (g = grad / 0 = inf), as in loss.hip
        if constexpr (K > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = col + k * G;
                if (c < N) io<T>::st(drow + c, on ? g * (__expf(r.p[k] - lse) * swt - r.w[k]) : g * 0.f);
            }
        } else {
            for (int c = col; c < N; c += G)
                io<T>::st(drow + c, on ? g * (__expf(io<T>::ld(prow + c) - lse) * swt - a.wt(trow, c)) : g * 0.f);
        }
    }
}

// arg-max of pred and of target per (masked) row, the lowest index winning a tie in both; conf[target][pred] += 1
__device__ __forceinline__ void arg_better(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
template <int G> __device__ __forceinline__ int group_argmax(float v, int i) {
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o);
        const int i2 = __shfl_xor(i, o);
        arg_better(v, i, v2, i2);
    }
    return i;
}
template <typename T, int G>
__global__ __launch_bounds__(256) void argmax_confusion_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                               const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                               unsigned long long* __restrict__ conf) {
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G, col = lane % G;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * RPW; base < R; base += (int64_t)gridDim.x * 4 * RPW) {
        const int64_t row = base + sub;
        const bool on = row < R && (!rowmask || rowmask[(row / Tn) * mask_ld + (row % Tn)] != 0);
        if (__ballot(on) == 0) continue;
        // a lane without a column holds (-inf, N): it loses every comparison against a real column (non-finite logits are outside the contract)
        float pv = -INFINITY, tv = -INFINITY;
        int pi = N, ti = N;
        if (on)
            for (int c = col; c < N; c += G) {     // c ascends: `>` keeps the lowest index
                const float p = io<T>::ld(pred + (size_t)row * N + c), t = target[(size_t)row * N + c];
                if (p > pv || pi == N) { pv = p; pi = c; }
                if (t > tv || ti == N) { tv = t; ti = c; }
            }
        pi = group_argmax<G>(pv, pi);
        ti = group_argmax<G>(tv, ti);
        if (on && col == 0 && pi < N && ti < N) atomicAdd(conf + (size_t)ti * N + pi, 1ULL);
    }
}
__global__ void zero_u64_kernel(unsigned long long* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0ULL;
}

int group_lanes(int N) {
    int g = 1;
    while (g < N && g < 64) g <<= 1;
    return g;
}
// rows a workgroup of four wavefronts takes per grid step, and the grid: at most 2048 workgroups (the partial sums' count; eight
// wavefronts a SIMD on 256 CUs - the kernels wait on memory, not on registers)
int ce_blocks(int64_t R, int N) {
    const int64_t per = 4 * (64 / group_lanes(N));
    return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (R + per - 1) / per));
}
// register slots per lane of the loss kernels: 1 while the group holds the row, 4 / 16 up to 256 / 1024 columns, 0 (streamed) beyond
constexpr int kMaxSlots = 16;

template <int G, int K> struct lanes_tag {
    static constexpr int lanes = G;
    static constexpr int slots = K;
};
template <typename F> int with_group(int N, F&& f) {
    switch (group_lanes(N)) {
    case 1: return f(lanes_tag<1, 1>());
    case 2: return f(lanes_tag<2, 1>());
    case 4: return f(lanes_tag<4, 1>());
    case 8: return f(lanes_tag<8, 1>());
    case 16: return f(lanes_tag<16, 1>());
    case 32: return f(lanes_tag<32, 1>());
    default:
        if (N <= 64) return f(lanes_tag<64, 1>());
        if (N <= 64 * 4) return f(lanes_tag<64, 4>());
        if (N <= 64 * kMaxSlots) return f(lanes_tag<64, kMaxSlots>());
        return f(lanes_tag<64, 0>());
    }
}

bool shape_ok(int T, int64_t R, int N, int mask_ld) { return R > 0 && N > 0 && T > 0 && R % T == 0 && mask_ld >= T; }

}  // namespace

extern "C" int64_t mmfm_softmax_ce_workspace(int64_t R, int N) {
    if (R <= 0 || N <= 0) return 0;
    return (int64_t)ce_blocks(R, N) * sizeof(float);
}

extern "C" int mmfm_softmax_ce_fwd(int dtype, const void* pred, const float* target, const float* class_weight, float label_smoothing,
                                   const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, float* loss_sum, float* rowstat,
                                   void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && loss_sum, "mmfm_softmax_ce_fwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_softmax_ce_fwd: bad dtype %d", dtype);
    MMFM_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "mmfm_softmax_ce_fwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
    MMFM_REQUIRE(shape_ok(T, R, N, mask_ld), "mmfm_softmax_ce_fwd: bad arguments");
    MMFM_REQUIRE(workspace && workspace_bytes >= mmfm_softmax_ce_workspace(R, N), "mmfm_softmax_ce_fwd: workspace too small");
    const int nb = ce_blocks(R, N);
    hipStream_t st = (hipStream_t)stream;
    const CeArgs a = {class_weight, 1.f - label_smoothing, label_smoothing / (float)N};
    const int rc = with_group(N, [&](auto K) {
        constexpr int G = decltype(K)::lanes, Ks = decltype(K)::slots;
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((ce_fwd_kernel<float, G, Ks>), dim3(nb), dim3(256), 0, st, a, (const float*)pred, target, rowmask, mask_ld, T, R, N, (float*)workspace, rowstat);
        else
            hipLaunchKernelGGL((ce_fwd_kernel<uint16_t, G, Ks>), dim3(nb), dim3(256), 0, st, a, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, (float*)workspace, rowstat);
        MMFM_LAUNCH_CHECK("mmfm_softmax_ce_fwd");
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(ce_sum_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, nb, loss_sum);
    MMFM_LAUNCH_CHECK("mmfm_softmax_ce_fwd");
    return 0;
}

extern "C" int mmfm_softmax_ce_bwd(int dtype, const void* pred, const float* target, const float* class_weight, float label_smoothing,
                                   const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const float* rowstat, const float* grad_out,
                                   const float* inv_n, void* dpred, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && grad_out && inv_n && dpred, "mmfm_softmax_ce_bwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_softmax_ce_bwd: bad dtype %d", dtype);
    MMFM_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "mmfm_softmax_ce_bwd: label_smoothing %g outside [0, 1]", (double)label_smoothing);
    MMFM_REQUIRE(shape_ok(T, R, N, mask_ld), "mmfm_softmax_ce_bwd: bad arguments");
    const int nb = ce_blocks(R, N);
    hipStream_t st = (hipStream_t)stream;
    const CeArgs a = {class_weight, 1.f - label_smoothing, label_smoothing / (float)N};
    return with_group(N, [&](auto K) {
        constexpr int G = decltype(K)::lanes, Ks = decltype(K)::slots;
        const bool f32 = dtype == MMFM_F32;
        if (rowstat && f32)
            hipLaunchKernelGGL((ce_bwd_kernel<float, G, 0, true>), dim3(nb), dim3(256), 0, st, a, (const float*)pred, target, rowmask, mask_ld, T, R, N, rowstat, grad_out, inv_n, (float*)dpred);
        else if (rowstat)
            hipLaunchKernelGGL((ce_bwd_kernel<uint16_t, G, 0, true>), dim3(nb), dim3(256), 0, st, a, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, rowstat, grad_out, inv_n, (uint16_t*)dpred);
        else if (f32)
            hipLaunchKernelGGL((ce_bwd_kernel<float, G, Ks, false>), dim3(nb), dim3(256), 0, st, a, (const float*)pred, target, rowmask, mask_ld, T, R, N, rowstat, grad_out, inv_n, (float*)dpred);
        else
            hipLaunchKernelGGL((ce_bwd_kernel<uint16_t, G, Ks, false>), dim3(nb), dim3(256), 0, st, a, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, rowstat, grad_out, inv_n, (uint16_t*)dpred);
        MMFM_LAUNCH_CHECK("mmfm_softmax_ce_bwd");
        return 0;
    });
}

extern "C" int mmfm_argmax_confusion(int dtype, const void* pred, const float* target, const uint8_t* rowmask, int mask_ld, int T, int64_t R,
                                     int N, int64_t* conf, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && conf, "mmfm_argmax_confusion: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_argmax_confusion: bad dtype %d", dtype);
    MMFM_REQUIRE(shape_ok(T, R, N, mask_ld), "mmfm_argmax_confusion: bad arguments");
    const int nb = ce_blocks(R, N);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cf = reinterpret_cast<unsigned long long*>(conf);
    const int64_t cells = (int64_t)N * N;
    hipLaunchKernelGGL(zero_u64_kernel, dim3((unsigned)std::min<int64_t>(256, (cells + 255) / 256)), dim3(256), 0, st, cf, cells);
    MMFM_LAUNCH_CHECK("mmfm_argmax_confusion");
    return with_group(N, [&](auto K) {
        constexpr int G = decltype(K)::lanes;
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((argmax_confusion_kernel<float, G>), dim3(nb), dim3(256), 0, st, (const float*)pred, target, rowmask, mask_ld, T, R, N, cf);
        else
            hipLaunchKernelGGL((argmax_confusion_kernel<uint16_t, G>), dim3(nb), dim3(256), 0, st, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, cf);
        MMFM_LAUNCH_CHECK("mmfm_argmax_confusion");
        return 0;
    });
}
