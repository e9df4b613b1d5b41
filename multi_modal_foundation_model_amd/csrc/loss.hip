// Masked elementwise losses (mm.py:79-82,217-239), forward reduction and backward: Poisson-NLL (log or rate input, optional Stirling
// term), MSE, L1, smooth-L1, Huber and BCE on logits, each with torch's semantics (include/mmfm.h).
// One wavefront per (b,t) row; unmasked rows are skipped without touching their data, so the
// algorithmic bytes are (rows masked) * N * (sizeof(T) + 4).  fp32 accumulation, fixed-order
// two-stage reduction (bitwise reproducible); n_examples is an exact int64 from mmfm_mask_prep.
// The kind (and the Stirling flag) is a template parameter: the inner loop carries no per-element switch.
// mmfm_masked_loss_elem_*: the same walk under a per-element mask given as a base pointer and three element strides (input masking).
// mmfm_masked_loss_chan_*: the same walk under the product of a [B,T] row mask and a [B,N] channel mask (padded neurons).
#include "common.h"
#include <algorithm>
#include <type_traits>

namespace {

// a = the kind's parameter (eps / beta / delta).  Kinds 0 and 1 are the expressions the library has always used.
template <int KIND, bool FULL>
__device__ __forceinline__ float loss_elem(float p, float t, float a) {
    float v;
    if constexpr (KIND == MMFM_LOSS_POISSON_LOG) v = __expf(p) - t * p;     // PoissonNLLLoss(log_input=True)
    else if constexpr (KIND == MMFM_LOSS_MSE) { const float d = p - t; v = d * d; }
    else if constexpr (KIND == MMFM_LOSS_POISSON_RATE) v = p - t * logf(p + a);   // PoissonNLLLoss(log_input=False, eps=a)
    else if constexpr (KIND == MMFM_LOSS_BCE_LOGITS) v = fmaxf(p, 0.f) - p * t + log1pf(__expf(-fabsf(p)));
    else {
        const float d = p - t, ad = fabsf(d);
        if constexpr (KIND == MMFM_LOSS_L1) v = ad;
        else if constexpr (KIND == MMFM_LOSS_SMOOTH_L1) v = ad < a ? 0.5f * d * d / a : ad - 0.5f * a;   // a == 0: never quadratic = L1
        else v = ad <= a ? 0.5f * d * d : a * (ad - 0.5f * a);                                            // Huber
    }
    if constexpr (FULL) {                          // PoissonNLLLoss(full=True): Stirling's term where t > 1; it has no gradient in p
        if (t > 1.f) v += t * logf(t) - t + 0.5f * logf(6.283185307179586f * t);
    }
    return v;
}
template <int KIND>
__device__ __forceinline__ float loss_grad(float p, float t, float a) {
    if constexpr (KIND == MMFM_LOSS_POISSON_LOG) return __expf(p) - t;
    else if constexpr (KIND == MMFM_LOSS_MSE) return 2.f * (p - t);
    else if constexpr (KIND == MMFM_LOSS_POISSON_RATE) return 1.f - t / (p + a);
    else if constexpr (KIND == MMFM_LOSS_BCE_LOGITS) {                       // sigmoid(p) - t, from exp(-|p|) <= 1: no overflow
        const float e = __expf(-fabsf(p)), r = 1.f / (1.f + e);
        return (p >= 0.f ? r : e * r) - t;
    } else {
        const float d = p - t, ad = fabsf(d);
        const float sg = d != d ? d : (float)(d > 0.f) - (float)(d < 0.f);     // sign(d): 0 at d == 0, NaN stays NaN
        if constexpr (KIND == MMFM_LOSS_L1) return sg;
        else if constexpr (KIND == MMFM_LOSS_SMOOTH_L1) return ad < a ? d / a : sg;
        else return ad <= a ? d : a * sg;
    }
}

template <typename T, int KIND, bool FULL>
__global__ __launch_bounds__(256) void loss_fwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                       float* __restrict__ part) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        if (!rowmask[(row / Tn) * mask_ld + (row % Tn)]) continue;
        for (int c = lane; c < N; c += 64) s += loss_elem<KIND, FULL>(io<T>::ld(pred + (size_t)row * N + c), target[(size_t)row * N + c], a);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void loss_sum_kernel(const float* __restrict__ part, int n, float* out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}

__global__ void loss_finalize_kernel(const float* loss_sum, const int64_t* count, int M, float* loss, float* inv_n) {
    float tot = 0.f;
    int64_t n = 0;
    for (int m = 0; m < M; ++m) { tot += loss_sum[m]; n += count[m]; }
    loss[0] = tot / (float)n;          // 0/0 -> NaN exactly like the reference (mm.py:237)
    inv_n[0] = 1.f / (float)n;
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void loss_bwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                       const float* __restrict__ grad_out, const float* __restrict__ inv_n,
                                                       T* __restrict__ dpred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float g = grad_out[0] * inv_n[0];
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        const bool on = rowmask[(row / Tn) * mask_ld + (row % Tn)] != 0;
        for (int c = lane; c < N; c += 64) {
            const size_t o = (size_t)row * N + c;
            // unmasked rows: mask * g with mask = 0 - i.e. 0 normally, NaN when nothing at all is masked (g = grad / 0 = inf), which is
            // what upstream's (loss * mask).sum() / mask.sum() hands to autograd (mm.py:217-239): every gradient of that step is NaN there
            io<T>::st(dpred + o, on ? g * loss_grad<KIND>(io<T>::ld(pred + o), target[o], a) : g * 0.f);
        }
    }
}

// ---- per-element masks (MMFM_LOSS_ELEM): element (b, t, n) of the mask sits at base[b * sb + t * st + n * sn], any stride may be 0.
// Rows, lanes and columns are walked exactly as in loss_fwd_kernel / loss_bwd_kernel, so an all-ones mask and a [B,T,1] mask give those
// kernels' bits.  An element whose mask is 0 is never loaded.
struct ElemMask {
    const uint8_t* base;
    int64_t sb, st, sn;
};

template <typename T, int KIND, bool FULL>
__global__ __launch_bounds__(256) void loss_elem_fwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target, ElemMask mk,
                                                            int Tn, int64_t R, int N, float* __restrict__ part, int64_t* __restrict__ cpart) {
    __shared__ float red[4];
    __shared__ long long cred[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.f;
    long long cnt = 0;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        const uint8_t* mrow = mk.base + (row / Tn) * mk.sb + (row % Tn) * mk.st;
        for (int c = lane; c < N; c += 64) {
            if (!mrow[c * mk.sn]) continue;
            s += loss_elem<KIND, FULL>(io<T>::ld(pred + (size_t)row * N + c), target[(size_t)row * N + c], a);
            ++cnt;
        }
    }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { red[wave] = s; cred[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        cpart[blockIdx.x] = cred[0] + cred[1] + cred[2] + cred[3];
    }
}

// second stage: the float partials in loss_sum_kernel's order, the integer partials exactly
__global__ void loss_elem_sum_kernel(const float* __restrict__ part, const int64_t* __restrict__ cpart, int n, float* out, int64_t* count) {
    float s = 0.f;
    long long cnt = 0;
    for (int i = threadIdx.x; i < n; i += 64) { s += part[i]; cnt += cpart[i]; }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (threadIdx.x == 0) { out[0] = s; count[0] = cnt; }
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void loss_elem_bwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target, ElemMask mk,
                                                            int Tn, int64_t R, int N, const float* __restrict__ grad_out,
                                                            const float* __restrict__ inv_n, T* __restrict__ dpred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float g = grad_out[0] * inv_n[0];
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        const uint8_t* mrow = mk.base + (row / Tn) * mk.sb + (row % Tn) * mk.st;
        for (int c = lane; c < N; c += 64) {
            const size_t o = (size_t)row * N + c;
            // unset elements: g * 0 - 0 normally, NaN when nothing at all is set (g = grad / 0 = inf), as loss_bwd_kernel
            io<T>::st(dpred + o, mrow[c * mk.sn] ? g * loss_grad<KIND>(io<T>::ld(pred + o), target[o], a) : g * 0.f);
        }
    }
}

// ---- row mask x channel mask (MMFM_LOSS_CHAN): element (row, c) is set iff rowmask[b * mask_ld + t] && chanmask[b * chan_ld + c], either
// leading dimension may be 0 (one mask for all samples).  The walk is loss_fwd_kernel's, so an all-ones channel mask gives its bits, and
// loss_elem_fwd_kernel's on the expanded product.  An unmasked row costs its one mask byte; in a masked row a cleared channel is never loaded.
// Up to 32 columns per lane (N <= 2048) the lane's bits of the sample's channel-mask row are gathered into one register: bit k = column
// lane + 64 k.  Each byte is still read once per row; wider rows read their byte inside the walk.
constexpr int CHAN_BITS_MAX = 64 * 32;
__device__ __forceinline__ uint32_t chan_bits(const uint8_t* __restrict__ crow, int lane, int N) {
    uint32_t bits = 0;
    for (int c = lane, k = 0; c < N; c += 64, ++k) bits |= (crow[c] ? 1u : 0u) << k;
    return bits;
}

template <typename T, int KIND, bool FULL>
__global__ __launch_bounds__(256) void loss_chan_fwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target,
                                                            const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                            const uint8_t* __restrict__ chanmask, int chan_ld, float* __restrict__ part,
                                                            int64_t* __restrict__ cpart) {
    __shared__ float red[4];
    __shared__ long long cred[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.f;
    long long cnt = 0;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        const int64_t bi = row / Tn;
        if (!rowmask[bi * mask_ld + (row % Tn)]) continue;
        const uint8_t* crow = chanmask + bi * chan_ld;
        if (N <= CHAN_BITS_MAX) {             // the lane's channel bits first, in one batch of independent byte loads: no load of the walk waits for a mask byte
            const uint32_t bits = chan_bits(crow, lane, N);
            for (int c = lane, k = 0; c < N; c += 64, ++k) {
                if (!((bits >> k) & 1u)) continue;
                s += loss_elem<KIND, FULL>(io<T>::ld(pred + (size_t)row * N + c), target[(size_t)row * N + c], a);
                ++cnt;
            }
            continue;
        }
        for (int c = lane; c < N; c += 64) {
            if (!crow[c]) continue;
            s += loss_elem<KIND, FULL>(io<T>::ld(pred + (size_t)row * N + c), target[(size_t)row * N + c], a);
            ++cnt;
        }
    }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { red[wave] = s; cred[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        cpart[blockIdx.x] = cred[0] + cred[1] + cred[2] + cred[3];
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void loss_chan_bwd_kernel(float a, const T* __restrict__ pred, const float* __restrict__ target,
                                                            const uint8_t* __restrict__ rowmask, int mask_ld, int Tn, int64_t R, int N,
                                                            const uint8_t* __restrict__ chanmask, int chan_ld,
                                                            const float* __restrict__ grad_out, const float* __restrict__ inv_n,
                                                            T* __restrict__ dpred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float g = grad_out[0] * inv_n[0];
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R; row += (int64_t)gridDim.x * 4) {
        const int64_t bi = row / Tn;
        const uint8_t* crow = chanmask + bi * chan_ld;
        if (!rowmask[bi * mask_ld + (row % Tn)]) {          // g * 0: 0 normally, NaN when nothing at all is set, as loss_bwd_kernel
            for (int c = lane; c < N; c += 64) io<T>::st(dpred + (size_t)row * N + c, g * 0.f);
            continue;
        }
        if (N <= CHAN_BITS_MAX) {
            const uint32_t bits = chan_bits(crow, lane, N);
            for (int c = lane, k = 0; c < N; c += 64, ++k) {
                const size_t o = (size_t)row * N + c;
                io<T>::st(dpred + o, ((bits >> k) & 1u) ? g * loss_grad<KIND>(io<T>::ld(pred + o), target[o], a) : g * 0.f);
            }
            continue;
        }
        for (int c = lane; c < N; c += 64) {
            const size_t o = (size_t)row * N + c;
            io<T>::st(dpred + o, crow[c] ? g * loss_grad<KIND>(io<T>::ld(pred + o), target[o], a) : g * 0.f);
        }
    }
}

int loss_blocks(int64_t R) { return (int)std::max<int64_t>(1, std::min<int64_t>(1024, (R + 3) / 4)); }

template <int KIND, bool FULL> struct loss_tag {
    static constexpr int kind = KIND;
    static constexpr bool full = FULL;
};
// kind (checked by the caller) and the Stirling flag -> a compile-time tag, as with_act does in mlp_fused.hip
template <typename F> int with_loss(int kind, bool full, F&& f) {
    switch (kind) {
    case MMFM_LOSS_POISSON_LOG: return full ? f(loss_tag<MMFM_LOSS_POISSON_LOG, true>()) : f(loss_tag<MMFM_LOSS_POISSON_LOG, false>());
    case MMFM_LOSS_MSE: return f(loss_tag<MMFM_LOSS_MSE, false>());
    case MMFM_LOSS_POISSON_RATE: return full ? f(loss_tag<MMFM_LOSS_POISSON_RATE, true>()) : f(loss_tag<MMFM_LOSS_POISSON_RATE, false>());
    case MMFM_LOSS_L1: return f(loss_tag<MMFM_LOSS_L1, false>());
    case MMFM_LOSS_SMOOTH_L1: return f(loss_tag<MMFM_LOSS_SMOOTH_L1, false>());
    case MMFM_LOSS_HUBER: return f(loss_tag<MMFM_LOSS_HUBER, false>());
    default: return f(loss_tag<MMFM_LOSS_BCE_LOGITS, false>());
    }
}

// the kind's own argument rules; the shape rules are the entry points'
bool loss_kind_ok(int kind, float param, int flags) {
    const bool poisson = kind == MMFM_LOSS_POISSON_LOG || kind == MMFM_LOSS_POISSON_RATE;
    return kind >= MMFM_LOSS_POISSON_LOG && kind <= MMFM_LOSS_BCE_LOGITS && param >= 0.f && (flags & ~MMFM_LOSS_FULL) == 0 &&
           (flags == 0 || poisson);
}

// `what` = the entry point's name in the error text; arguments are checked by the caller
int launch_fwd(const char* what, int dtype, int kind, float param, int flags, const void* pred, const float* target, const uint8_t* rowmask,
               int mask_ld, int T, int64_t R, int N, float* loss_sum, void* workspace, mmfm_stream stream) {
    const int nb = loss_blocks(R);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != MMFM_F32 && dtype != MMFM_BF16) return mmfm_set_error(-1, "%s: bad dtype %d", what, dtype);
    const int rc = with_loss(kind, (flags & MMFM_LOSS_FULL) != 0, [&](auto K) {
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_fwd_kernel<float, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, st, param, (const float*)pred, target, rowmask, mask_ld, T, R, N, (float*)workspace);
        else
            hipLaunchKernelGGL((loss_fwd_kernel<uint16_t, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, st, param, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, (float*)workspace);
        MMFM_LAUNCH_CHECK(what);
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, nb, loss_sum);
    MMFM_LAUNCH_CHECK(what);
    return 0;
}

int launch_bwd(const char* what, int dtype, int kind, float param, const void* pred, const float* target, const uint8_t* rowmask, int mask_ld,
               int T, int64_t R, int N, const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream) {
    const int nb = loss_blocks(R);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != MMFM_F32 && dtype != MMFM_BF16) return mmfm_set_error(-1, "%s: bad dtype %d", what, dtype);
    return with_loss(kind, false, [&](auto K) {            // the Stirling term has no gradient: one backward per kind
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_bwd_kernel<float, Kd::kind>), dim3(nb), dim3(256), 0, st, param, (const float*)pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, (float*)dpred);
        else
            hipLaunchKernelGGL((loss_bwd_kernel<uint16_t, Kd::kind>), dim3(nb), dim3(256), 0, st, param, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, (uint16_t*)dpred);
        MMFM_LAUNCH_CHECK(what);
        return 0;
    });
}

}  // namespace

extern "C" int64_t mmfm_masked_loss_workspace(int64_t R, int N) { (void)N; return (int64_t)loss_blocks(R) * sizeof(float); }

extern "C" int mmfm_masked_loss_fwd(int dtype, int kind, const void* pred, const float* target, const uint8_t* rowmask, int mask_ld,
                                    int T, int64_t R, int N, float* loss_sum, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && loss_sum, "mmfm_masked_loss_fwd: null pointer");
    MMFM_REQUIRE((kind == 0 || kind == 1) && R > 0 && N > 0 && T > 0 && R % T == 0 && mask_ld >= T, "mmfm_masked_loss_fwd: bad arguments");
    MMFM_REQUIRE(workspace && workspace_bytes >= mmfm_masked_loss_workspace(R, N), "mmfm_masked_loss_fwd: workspace too small");
    return launch_fwd("mmfm_masked_loss_fwd", dtype, kind, 0.f, 0, pred, target, rowmask, mask_ld, T, R, N, loss_sum, workspace, stream);
}

extern "C" int mmfm_masked_loss_kind_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, float* loss_sum, void* workspace,
                                         int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && loss_sum, "mmfm_masked_loss_kind_fwd: null pointer");
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_kind_fwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(R > 0 && N > 0 && T > 0 && R % T == 0 && mask_ld >= T, "mmfm_masked_loss_kind_fwd: bad arguments");
    MMFM_REQUIRE(workspace && workspace_bytes >= mmfm_masked_loss_workspace(R, N), "mmfm_masked_loss_kind_fwd: workspace too small");
    return launch_fwd("mmfm_masked_loss_kind_fwd", dtype, kind, param, flags, pred, target, rowmask, mask_ld, T, R, N, loss_sum, workspace, stream);
}

extern "C" int mmfm_loss_finalize(const float* loss_sum, const int64_t* count, int M, float* loss, float* inv_n, mmfm_stream stream) {
    MMFM_REQUIRE(loss_sum && count && loss && inv_n && M > 0, "mmfm_loss_finalize: bad arguments");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss_sum, count, M, loss, inv_n);
    MMFM_LAUNCH_CHECK("mmfm_loss_finalize");
    return 0;
}

extern "C" int mmfm_masked_loss_bwd(int dtype, int kind, const void* pred, const float* target, const uint8_t* rowmask, int mask_ld,
                                    int T, int64_t R, int N, const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && grad_out && inv_n && dpred, "mmfm_masked_loss_bwd: null pointer");
    MMFM_REQUIRE((kind == 0 || kind == 1) && R > 0 && N > 0 && T > 0 && R % T == 0 && mask_ld >= T, "mmfm_masked_loss_bwd: bad arguments");
    return launch_bwd("mmfm_masked_loss_bwd", dtype, kind, 0.f, pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, dpred, stream);
}

extern "C" int mmfm_masked_loss_kind_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const float* grad_out,
                                         const float* inv_n, void* dpred, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && grad_out && inv_n && dpred, "mmfm_masked_loss_kind_bwd: null pointer");
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_kind_bwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(R > 0 && N > 0 && T > 0 && R % T == 0 && mask_ld >= T, "mmfm_masked_loss_kind_bwd: bad arguments");
    return launch_bwd("mmfm_masked_loss_kind_bwd", dtype, kind, param, pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, dpred, stream);
}

// ---- per-element masks.  workspace: loss_blocks(R) float partials, then (8-byte aligned) as many int64 count partials
namespace {
int64_t elem_cpart_offset(int64_t R) { return ((int64_t)loss_blocks(R) * (int64_t)sizeof(float) + 7) / 8 * 8; }
bool elem_shape_ok(int B, int T, int N, int64_t sb, int64_t st, int64_t sn) { return B > 0 && T > 0 && N > 0 && sb >= 0 && st >= 0 && sn >= 0; }
}  // namespace

extern "C" int64_t mmfm_masked_loss_elem_workspace(int64_t R, int N) {
    (void)N;
    return elem_cpart_offset(R) + (int64_t)loss_blocks(R) * (int64_t)sizeof(int64_t);
}

extern "C" int mmfm_masked_loss_elem_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* mask, int64_t sb, int64_t st, int64_t sn, int B, int T, int N, float* loss_sum,
                                         int64_t* count, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && mask && loss_sum && count, "mmfm_masked_loss_elem_fwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_masked_loss_elem_fwd: bad dtype %d", dtype);
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_elem_fwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(elem_shape_ok(B, T, N, sb, st, sn), "mmfm_masked_loss_elem_fwd: bad arguments");
    const int64_t R = (int64_t)B * T;
    MMFM_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= mmfm_masked_loss_elem_workspace(R, N),
                 "mmfm_masked_loss_elem_fwd: workspace too small or not 8-byte aligned");
    const int nb = loss_blocks(R);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    int64_t* cpart = (int64_t*)((char*)workspace + elem_cpart_offset(R));
    const ElemMask mk = {mask, sb, st, sn};
    const int rc = with_loss(kind, (flags & MMFM_LOSS_FULL) != 0, [&](auto K) {
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_elem_fwd_kernel<float, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, s, param, (const float*)pred, target, mk, T, R, N, part, cpart);
        else
            hipLaunchKernelGGL((loss_elem_fwd_kernel<uint16_t, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, s, param, (const uint16_t*)pred, target, mk, T, R, N, part, cpart);
        MMFM_LAUNCH_CHECK("mmfm_masked_loss_elem_fwd");
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(loss_elem_sum_kernel, dim3(1), dim3(64), 0, s, (const float*)part, (const int64_t*)cpart, nb, loss_sum, count);
    MMFM_LAUNCH_CHECK("mmfm_masked_loss_elem_fwd");
    return 0;
}

extern "C" int mmfm_masked_loss_elem_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* mask, int64_t sb, int64_t st, int64_t sn, int B, int T, int N,
                                         const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && mask && grad_out && inv_n && dpred, "mmfm_masked_loss_elem_bwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_masked_loss_elem_bwd: bad dtype %d", dtype);
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_elem_bwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(elem_shape_ok(B, T, N, sb, st, sn), "mmfm_masked_loss_elem_bwd: bad arguments");
    const int64_t R = (int64_t)B * T;
    const int nb = loss_blocks(R);
    hipStream_t s = (hipStream_t)stream;
    const ElemMask mk = {mask, sb, st, sn};
    return with_loss(kind, false, [&](auto K) {            // the Stirling term has no gradient: one backward per kind
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_elem_bwd_kernel<float, Kd::kind>), dim3(nb), dim3(256), 0, s, param, (const float*)pred, target, mk, T, R, N, grad_out, inv_n, (float*)dpred);
        else
            hipLaunchKernelGGL((loss_elem_bwd_kernel<uint16_t, Kd::kind>), dim3(nb), dim3(256), 0, s, param, (const uint16_t*)pred, target, mk, T, R, N, grad_out, inv_n, (uint16_t*)dpred);
        MMFM_LAUNCH_CHECK("mmfm_masked_loss_elem_bwd");
        return 0;
    });
}

// ---- row mask x channel mask.  The workspace is the per-element form's: float partials, then int64 count partials
namespace {
// shared by both entry points: everything but the pointers and the workspace
bool chan_shape_ok(int mask_ld, int T, int64_t R, int N, int chan_ld) {
    return R > 0 && N > 0 && T > 0 && R % T == 0 && (mask_ld == 0 || mask_ld >= T) && (chan_ld == 0 || chan_ld >= N);
}
}  // namespace

extern "C" int64_t mmfm_masked_loss_chan_workspace(int64_t R, int N) { return mmfm_masked_loss_elem_workspace(R, N); }

extern "C" int mmfm_masked_loss_chan_fwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const uint8_t* chanmask, int chan_ld,
                                         float* loss_sum, int64_t* count, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && chanmask && loss_sum && count, "mmfm_masked_loss_chan_fwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_masked_loss_chan_fwd: bad dtype %d", dtype);
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_chan_fwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(chan_shape_ok(mask_ld, T, R, N, chan_ld), "mmfm_masked_loss_chan_fwd: bad arguments");
    MMFM_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= mmfm_masked_loss_chan_workspace(R, N),
                 "mmfm_masked_loss_chan_fwd: workspace too small or not 8-byte aligned");
    const int nb = loss_blocks(R);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    int64_t* cpart = (int64_t*)((char*)workspace + elem_cpart_offset(R));
    const int rc = with_loss(kind, (flags & MMFM_LOSS_FULL) != 0, [&](auto K) {
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_chan_fwd_kernel<float, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, s, param, (const float*)pred, target, rowmask, mask_ld, T, R, N, chanmask, chan_ld, part, cpart);
        else
            hipLaunchKernelGGL((loss_chan_fwd_kernel<uint16_t, Kd::kind, Kd::full>), dim3(nb), dim3(256), 0, s, param, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, chanmask, chan_ld, part, cpart);
        MMFM_LAUNCH_CHECK("mmfm_masked_loss_chan_fwd");
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(loss_elem_sum_kernel, dim3(1), dim3(64), 0, s, (const float*)part, (const int64_t*)cpart, nb, loss_sum, count);
    MMFM_LAUNCH_CHECK("mmfm_masked_loss_chan_fwd");
    return 0;
}

extern "C" int mmfm_masked_loss_chan_bwd(int dtype, int kind, float param, int flags, const void* pred, const float* target,
                                         const uint8_t* rowmask, int mask_ld, int T, int64_t R, int N, const uint8_t* chanmask, int chan_ld,
                                         const float* grad_out, const float* inv_n, void* dpred, mmfm_stream stream) {
    MMFM_REQUIRE(pred && target && rowmask && chanmask && grad_out && inv_n && dpred, "mmfm_masked_loss_chan_bwd: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_masked_loss_chan_bwd: bad dtype %d", dtype);
    MMFM_REQUIRE(loss_kind_ok(kind, param, flags), "mmfm_masked_loss_chan_bwd: bad kind %d / param %g / flags %d", kind, (double)param, flags);
    MMFM_REQUIRE(chan_shape_ok(mask_ld, T, R, N, chan_ld), "mmfm_masked_loss_chan_bwd: bad arguments");
    const int nb = loss_blocks(R);
    hipStream_t s = (hipStream_t)stream;
    return with_loss(kind, false, [&](auto K) {            // the Stirling term has no gradient: one backward per kind
        using Kd = decltype(K);
        if (dtype == MMFM_F32)
            hipLaunchKernelGGL((loss_chan_bwd_kernel<float, Kd::kind>), dim3(nb), dim3(256), 0, s, param, (const float*)pred, target, rowmask, mask_ld, T, R, N, chanmask, chan_ld, grad_out, inv_n, (float*)dpred);
        else
            hipLaunchKernelGGL((loss_chan_bwd_kernel<uint16_t, Kd::kind>), dim3(nb), dim3(256), 0, s, param, (const uint16_t*)pred, target, rowmask, mask_ld, T, R, N, chanmask, chan_ld, grad_out, inv_n, (uint16_t*)dpred);
        MMFM_LAUNCH_CHECK("mmfm_masked_loss_chan_bwd");
        return 0;
    });
}
