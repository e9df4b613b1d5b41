// Per-session linear layers (MMFM_SESSION_LINEAR; include/mmfm.h): the read-in x[.., :n_s] . W_s -> [.., P], the read-out
// f . W_s^T -> [.., :n_s] (zeros beyond n_s) and their weight gradients, with the session of every sample, the session's extent n_s
// and the offsets of its weights read from DEVICE memory: launch geometry depends on (B, T, P, N_max) - and, for the weight
// gradient, on (S, chunk) - only, so one captured graph serves every session and every mix of sessions of a batch shape.
//
// One tile scheme serves the three products: a 256-thread workgroup owns a 64 x 64 output tile and walks the reduction in steps of
// 32 through two LDS tiles.  A workgroup never crosses a sample (forward kernels) or a chunk of samples of one session (weight
// gradient), so the session facts are workgroup-uniform scalars and every barrier is reached by the whole workgroup.
//   * staging: each thread moves 8 consecutive elements of the operand's contiguous direction, as one 16-byte (bf16) or two 16-byte
//     (fp32) loads where the tile's origin and the row stride are 16-byte aligned, element by element otherwise.  An element outside
//     the operand's LIVE extent (row >= rows left, column >= n_s) is NOT read: the register is set to zero, so the ragged tail
//     enters the product as 0 * 0 whatever the padding holds (NaN included) and nothing beyond the buffers is touched.
//   * bf16: LDS tiles [64][32] with 40-element rows (16-byte fragments, rows 80 bytes apart); each of the 4 waves owns a 32 x 32
//     quadrant, two v_mfma_f32_32x32x16_bf16 per step.  Lane l = (r = l & 31, h = l >> 5) holds A[row r][k = 8h + j] and
//     B[k = 8h + j][col r]; the accumulator has col = r and row = (reg & 3) + 8 (reg >> 2) + 4 h.
//   * fp32: LDS tiles [32][64] with 68-element rows; each thread owns a 4 x 4 block and runs a k-ordered FMA chain (gemm.hip's
//     choice for the parity path): the sum of every output element is taken in the order k = 0, 1, 2, ... on every launch.
// Nothing here is atomic and no sum depends on the grid: the same inputs give the same bits on every call, and permuting the samples
// of a batch permutes the rows of the forward outputs bit for bit (a row's sum never looks at another sample).
//
// Weight gradient: the host groups the samples by session (order[B]) and cuts each session's run into chunks of `chunk` samples
// (tests and the engine pass the table; csrc never reads it back).  grid.z runs over the chunk table's fixed capacity; an entry beyond
// the live ones returns before any load.  A session of ONE chunk writes its [n_s][P] span (and bias span) directly; a longer run
// writes one fp32 slab per chunk and a second kernel sums the slabs of a session in chunk order.  The span of a session without a
// sample in the batch is never written; slabs need no memset (the reducer reads exactly what the chunks of that session wrote).
#include "common.h"

namespace {

constexpr int TM = 64, TN = 64, KS = 32, NT = 256;
constexpr int MAX_BATCH_SESSIONS = 64;          // distinct sessions in one batch (the host refuses more, naming the eids)

struct SessArgs {
    int B, T, P, N_max, S, ld_pad, ld_p;
    const int32_t* sid;
    const int32_t* n;
    const int64_t* w_off;
    const int64_t* b_off;
    int64_t w_elems, b_elems;
};

template <typename T> struct Lds;
template <> struct Lds<uint16_t> {
    static constexpr int RS = 40, SIZE = TM * RS;
    static __device__ __forceinline__ int idx(int m, int k) { return m * RS + k; }
};
template <> struct Lds<float> {
    static constexpr int RS = 68, SIZE = KS * RS;
    static __device__ __forceinline__ int idx(int m, int k) { return k * RS + m; }
};

template <typename T> __device__ __forceinline__ bool aligned16(const T* p, int64_t ld) {
    return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)(ld * (int64_t)sizeof(T))) & 15) == 0;
}

// One [64 (m)] x [32 (k)] tile into LDS.  KC: element (m, k) lives at src[m * ld + k] (k contiguous), else at src[k * ld + m].
// Live extent: m < mv, k < kv (either may exceed the tile); everything else becomes 0 without a load.
template <typename T, bool KC>
__device__ __forceinline__ void stage(T* lds, const T* src, int64_t ld, int mv, int kv, bool vec, int tid) {
    const int o = KC ? tid >> 2 : tid >> 3;                     // index along the strided direction: m (KC) or k
    const int i0 = KC ? (tid & 3) * 8 : (tid & 7) * 8;          // first index along the contiguous direction: k (KC) or m
    const int ov = KC ? mv : kv, iv = KC ? kv : mv;
    const T* p = src + (int64_t)o * ld + i0;
    __attribute__((aligned(16))) T v[8];
    if (vec && o < ov && i0 + 8 <= iv) {
        if constexpr (sizeof(T) == 2) {
            *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(p);
        } else {
            *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p);
            *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(p + 4);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (o < ov && i0 + j < iv) ? p[j] : T(0);
    }
    if constexpr (sizeof(T) == 2) {
        if constexpr (KC) {
            *reinterpret_cast<uint4*>(lds + Lds<T>::idx(o, i0)) = *reinterpret_cast<uint4*>(v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) lds[Lds<T>::idx(i0 + j, o)] = v[j];
        }
    } else {
        if constexpr (KC) {
#pragma unroll
            for (int j = 0; j < 8; ++j) lds[Lds<T>::idx(o, i0 + j)] = v[j];
        } else {
            *reinterpret_cast<float4*>(lds + Lds<T>::idx(i0, o)) = *reinterpret_cast<float4*>(v);
            *reinterpret_cast<float4*>(lds + Lds<T>::idx(i0 + 4, o)) = *reinterpret_cast<float4*>(v + 4);
        }
    }
}

typedef __attribute__((ext_vector_type(8))) __bf16 opnd;

template <typename T> struct Acc;
template <> struct Acc<uint16_t> {
    f32x16 c;
    int r, h, m0, n0;
    __device__ __forceinline__ Acc(int tid) {
        const int lane = tid & 63, w = tid >> 6;
        r = lane & 31; h = lane >> 5; m0 = (w >> 1) * 32; n0 = (w & 1) * 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = 0.f;
    }
    __device__ __forceinline__ void step(const uint16_t* As, const uint16_t* Bs) {
#pragma unroll
        for (int kk = 0; kk < KS; kk += 16) {
            const opnd a = *reinterpret_cast<const opnd*>(As + Lds<uint16_t>::idx(m0 + r, kk + 8 * h));
            const opnd b = *reinterpret_cast<const opnd*>(Bs + Lds<uint16_t>::idx(n0 + r, kk + 8 * h));
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
        }
    }
    template <typename Fn> __device__ __forceinline__ void each(Fn&& fn) const {
#pragma unroll
        for (int i = 0; i < 16; ++i) fn(m0 + (i & 3) + 8 * (i >> 2) + 4 * h, n0 + r, c[i]);
    }
};
template <> struct Acc<float> {
    float c[4][4];
    int tx, ty;
    __device__ __forceinline__ Acc(int tid) {
        tx = tid & 15; ty = tid >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[i][j] = 0.f;
    }
    __device__ __forceinline__ void step(const float* As, const float* Bs) {
#pragma unroll 8
        for (int k = 0; k < KS; ++k) {
            const float4 a4 = *reinterpret_cast<const float4*>(As + Lds<float>::idx(ty * 4, k));
            const float4 b4 = *reinterpret_cast<const float4*>(Bs + Lds<float>::idx(tx * 4, k));
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) c[i][j] = fmaf(a[i], b[j], c[i][j]);
        }
    }
    template <typename Fn> __device__ __forceinline__ void each(Fn&& fn) const {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) fn(ty * 4 + i, tx * 4 + j, c[i][j]);
    }
};

// acc += A[64 x K] . B[K x 64] over the reduction range [0, K).  cs_tile (As, Bs or nullptr): threads 0..63 also add the k-ordered sum
// of their row of that tile into cs (the bias gradient: a column sum of one operand).  K and cs_tile are workgroup-uniform.
template <typename T, bool AKC, bool BKC>
__device__ __forceinline__ void mma_range(Acc<T>& acc, T* As, T* Bs, const T* A, int64_t lda, int mvA, const T* B, int64_t ldb, int mvB,
                                          int K, int tid, const T* cs_tile, float& cs) {
    const bool vecA = aligned16(A, lda), vecB = aligned16(B, ldb);
    for (int k0 = 0; k0 < K; k0 += KS) {
        stage<T, AKC>(As, AKC ? A + k0 : A + (int64_t)k0 * lda, lda, mvA, K - k0, vecA, tid);
        stage<T, BKC>(Bs, BKC ? B + k0 : B + (int64_t)k0 * ldb, ldb, mvB, K - k0, vecB, tid);
        __syncthreads();
        acc.step(As, Bs);
        if (cs_tile && tid < TM) {
#pragma unroll 8
            for (int k = 0; k < KS; ++k) cs += io<T>::ld(cs_tile + Lds<T>::idx(tid, k));
        }
        __syncthreads();
    }
}

// the session of sample b: n = 0 for a session index or a weight span outside the tables (nothing of it is then read)
struct Sess { int n; int64_t woff, boff; };
__device__ __forceinline__ Sess sess_of(const SessArgs& a, int s, int bias_len_is_n, bool has_bias) {
    Sess r = {0, 0, 0};
    if (s < 0 || s >= a.S) return r;
    const int n = a.n[s];
    const int64_t wo = a.w_off[s];
    if (n <= 0 || n > a.N_max || wo < 0 || wo + (int64_t)n * a.P > a.w_elems) return r;
    if (has_bias) {
        const int64_t bo = a.b_off[s];
        if (bo < 0 || bo + (bias_len_is_n ? n : a.P) > a.b_elems) return r;
        r.boff = bo;
    }
    r.n = n; r.woff = wo;
    return r;
}

// y[b, t, p] = sum_{c < n_s} x[b, t, c] W_s[c, p] (+ bias_s[p]);  grid (ceil(P / 64), ceil(T / 64), B)
template <typename T>
__global__ __launch_bounds__(NT) void session_reduce_kernel(SessArgs a, const T* __restrict__ x, const T* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) T As[Lds<T>::SIZE];
    __shared__ __attribute__((aligned(16))) T Bs[Lds<T>::SIZE];
    const int tid = threadIdx.x, b = blockIdx.z, t0 = blockIdx.y * TM, p0 = blockIdx.x * TN;
    const Sess s = sess_of(a, a.sid[b], 0, bias != nullptr);
    Acc<T> acc(tid);
    float cs = 0.f;
    const int64_t row0 = (int64_t)b * a.T + t0;
    mma_range<T, true, false>(acc, As, Bs, x + row0 * a.ld_pad, a.ld_pad, a.T - t0, w + s.woff + p0, a.P, a.P - p0, s.n, tid, nullptr, cs);
    const float* bs = (bias && s.n) ? bias + s.boff : nullptr;
    acc.each([&](int m, int nn, float v) {
        if (t0 + m < a.T && p0 + nn < a.P) io<T>::st(y + (row0 + m) * a.ld_p + p0 + nn, bs ? v + bs[p0 + nn] : v);
    });
}

// y[b, t, c] = sum_p f[b, t, p] W_s[c, p] (+ bias_s[c]) for c < n_s, 0 for n_s <= c < N_max;  grid (ceil(N_max / 64), ceil(T / 64), B)
template <typename T>
__global__ __launch_bounds__(NT) void session_expand_kernel(SessArgs a, const T* __restrict__ f, const T* __restrict__ w,
                                                            const float* __restrict__ bias, T* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) T As[Lds<T>::SIZE];
    __shared__ __attribute__((aligned(16))) T Bs[Lds<T>::SIZE];
    const int tid = threadIdx.x, b = blockIdx.z, t0 = blockIdx.y * TM, c0 = blockIdx.x * TN;
    const Sess s = sess_of(a, a.sid[b], 1, bias != nullptr);
    Acc<T> acc(tid);
    float cs = 0.f;
    const int64_t row0 = (int64_t)b * a.T + t0;
    if (c0 < s.n)            // a tile wholly in the padding multiplies nothing: its accumulators stay 0
        mma_range<T, true, true>(acc, As, Bs, f + row0 * a.ld_p, a.ld_p, a.T - t0, w + s.woff + (int64_t)c0 * a.P, a.P, s.n - c0, a.P, tid, nullptr, cs);
    const float* bs = (bias && s.n) ? bias + s.boff : nullptr;
    acc.each([&](int m, int nn, float v) {
        const int c = c0 + nn;
        if (t0 + m < a.T && c < a.N_max) io<T>::st(y + (row0 + m) * a.ld_pad + c, c < s.n ? (bs ? v + bs[c] : v) : 0.f);
    });
}

// run table (int32, DEVICE): [0] live chunks, [1] chunk size, [2] chunk capacity, [3] B, order[B], then {session, start, count, k} per
// chunk: k = 1 the session's only chunk (direct), k >= 2 the first of k chunks, k = 0 a later chunk of its session.
constexpr int RUN_HDR = 4, RUN_ENT = 4;

// dW_s[c, p] = sum over the samples b of session s, t: A[b, t, c] Q[b, t, p];  grid (ceil(P / 64), ceil(N_max / 64), chunk capacity)
template <typename T>
__global__ __launch_bounds__(NT) void session_dw_kernel(SessArgs a, const T* __restrict__ A, const T* __restrict__ Q,
                                                        const int32_t* __restrict__ runs, int nch_max, float* __restrict__ dw,
                                                        float* __restrict__ db, int bias_from_pad, float* __restrict__ slabs,
                                                        int64_t slab_stride) {
    __shared__ __attribute__((aligned(16))) T As[Lds<T>::SIZE];
    __shared__ __attribute__((aligned(16))) T Bs[Lds<T>::SIZE];
    const int tid = threadIdx.x, ch = blockIdx.z, c0 = blockIdx.y * TM, p0 = blockIdx.x * TN;
    if (runs[2] != nch_max || runs[3] != a.B || runs[0] > nch_max || ch >= runs[0]) return;      // beyond the live entries: before any load of data
    const int32_t* order = runs + RUN_HDR;
    const int32_t* e = runs + RUN_HDR + a.B + RUN_ENT * ch;
    const int start = e[1], cnt = e[2], k = e[3];
    if (start < 0 || cnt <= 0 || start + cnt > a.B) return;
    const Sess s = sess_of(a, e[0], bias_from_pad, db != nullptr);
    if (c0 >= s.n) return;                                                    // rows beyond n_s are not part of the session's span
    const bool cs_on = db != nullptr && (bias_from_pad ? p0 == 0 : c0 == 0);
    const T* cs_tile = cs_on ? (bias_from_pad ? As : Bs) : nullptr;
    Acc<T> acc(tid);
    float cs = 0.f;
    for (int i = 0; i < cnt; ++i) {
        const int b = order[start + i];
        if (b < 0 || b >= a.B) continue;
        const int64_t row0 = (int64_t)b * a.T;
        mma_range<T, false, false>(acc, As, Bs, A + row0 * a.ld_pad + c0, a.ld_pad, s.n - c0, Q + row0 * a.ld_p + p0, a.ld_p, a.P - p0, a.T, tid,
                                   cs_tile, cs);
    }
    float* dst = k == 1 ? dw + s.woff : slabs + (int64_t)ch * slab_stride;
    acc.each([&](int m, int nn, float v) {
        if (c0 + m < s.n && p0 + nn < a.P) dst[(int64_t)(c0 + m) * a.P + p0 + nn] = v;
    });
    if (cs_on && tid < TM) {
        float* dstb = k == 1 ? db + s.boff : slabs + (int64_t)ch * slab_stride + (int64_t)a.N_max * a.P;
        const int i = (bias_from_pad ? c0 : p0) + tid;
        if (i < (bias_from_pad ? s.n : a.P)) dstb[i] = cs;
    }
}

// the slabs of a session of k >= 2 chunks, summed in chunk order;  grid (ceil((N_max P + max(N_max, P)) / 256), chunk capacity)
__global__ __launch_bounds__(256) void session_dw_reduce_kernel(SessArgs a, const int32_t* __restrict__ runs, int nch_max, float* __restrict__ dw,
                                                               float* __restrict__ db, int bias_from_pad, const float* __restrict__ slabs,
                                                               int64_t slab_stride) {
    const int ch = blockIdx.y;
    if (runs[2] != nch_max || runs[3] != a.B || runs[0] > nch_max || ch >= runs[0]) return;
    const int32_t* e = runs + RUN_HDR + a.B + RUN_ENT * ch;
    const int k = e[3];
    if (k < 2 || ch + k > runs[0]) return;
    const Sess s = sess_of(a, e[0], bias_from_pad, db != nullptr);
    if (s.n == 0) return;
    const int64_t nw = (int64_t)s.n * a.P, nb = db ? (bias_from_pad ? s.n : a.P) : 0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw + nb) return;
    const int64_t src = i < nw ? i : (int64_t)a.N_max * a.P + (i - nw);
    float sum = slabs[(int64_t)ch * slab_stride + src];
    for (int j = 1; j < k; ++j) sum += slabs[(int64_t)(ch + j) * slab_stride + src];
    if (i < nw) dw[s.woff + i] = sum; else db[s.boff + (i - nw)] = sum;
}

int chunk_capacity(int B, int S, int chunk) {
    const int live = S < B ? S : B;
    const long cap = (long)cdiv(B, chunk) + (live < MAX_BATCH_SESSIONS ? live : MAX_BATCH_SESSIONS);
    return (int)(cap < B ? cap : B);
}
int64_t slab_elems(int P, int N_max) {
    const int64_t e = (int64_t)N_max * P + (N_max > P ? N_max : P);
    return (e + 3) / 4 * 4;
}

int check_desc(const mmfm_session_desc* d, const char* what, bool need_w) {
    MMFM_REQUIRE(d, "%s: NULL descriptor", what);
    MMFM_REQUIRE(d->dtype == MMFM_F32 || d->dtype == MMFM_BF16, "%s: unknown dtype %d", what, d->dtype);
    MMFM_REQUIRE(d->B >= 1 && d->T >= 1 && d->P >= 1 && d->N_max >= 1 && d->S >= 1, "%s: B %d, T %d, P %d, N_max %d, S %d must all be >= 1", what,
                 d->B, d->T, d->P, d->N_max, d->S);
    MMFM_REQUIRE(d->B <= 65535 && cdiv(d->T, TM) <= 65535, "%s: B %d or T %d beyond the grid limits", what, d->B, d->T);
    MMFM_REQUIRE(d->ld_pad >= d->N_max, "%s: ld_pad %d < N_max %d", what, d->ld_pad, d->N_max);
    MMFM_REQUIRE(d->ld_p >= d->P, "%s: ld_p %d < P %d", what, d->ld_p, d->P);
    MMFM_REQUIRE(d->sid && d->n && d->w_off, "%s: NULL session table (sid %p, n %p, w_off %p)", what, (const void*)d->sid, (const void*)d->n,
                 (const void*)d->w_off);
    MMFM_REQUIRE(d->w_elems >= 1, "%s: w_elems %lld", what, (long long)d->w_elems);
    if (need_w) {
        MMFM_REQUIRE(d->w, "%s: NULL weights", what);
        MMFM_REQUIRE(!d->bias || (d->b_off && d->b_elems >= 1), "%s: a bias needs b_off and b_elems", what);
    }
    return 0;
}
SessArgs args_of(const mmfm_session_desc* d) {
    return SessArgs{d->B, d->T, d->P, d->N_max, d->S, d->ld_pad, d->ld_p, d->sid, d->n, d->w_off, d->b_off, d->w_elems, d->b_elems};
}

}  // namespace

extern "C" int mmfm_session_reduce(const mmfm_session_desc* d, const void* x_pad, void* y, mmfm_stream stream) {
    if (int rc = check_desc(d, "mmfm_session_reduce", true)) return rc;
    MMFM_REQUIRE(x_pad && y, "mmfm_session_reduce: NULL operand (x_pad %p, y %p)", x_pad, y);
    const dim3 grid(cdiv(d->P, TN), cdiv(d->T, TM), d->B);
    hipStream_t st = (hipStream_t)stream;
    if (d->dtype == MMFM_BF16)
        session_reduce_kernel<uint16_t><<<grid, NT, 0, st>>>(args_of(d), (const uint16_t*)x_pad, (const uint16_t*)d->w, d->bias, (uint16_t*)y);
    else
        session_reduce_kernel<float><<<grid, NT, 0, st>>>(args_of(d), (const float*)x_pad, (const float*)d->w, d->bias, (float*)y);
    MMFM_LAUNCH_CHECK("mmfm_session_reduce");
    return 0;
}

extern "C" int mmfm_session_expand(const mmfm_session_desc* d, const void* f, void* y_pad, mmfm_stream stream) {
    if (int rc = check_desc(d, "mmfm_session_expand", true)) return rc;
    MMFM_REQUIRE(f && y_pad, "mmfm_session_expand: NULL operand (f %p, y_pad %p)", f, y_pad);
    const dim3 grid(cdiv(d->N_max, TN), cdiv(d->T, TM), d->B);
    hipStream_t st = (hipStream_t)stream;
    if (d->dtype == MMFM_BF16)
        session_expand_kernel<uint16_t><<<grid, NT, 0, st>>>(args_of(d), (const uint16_t*)f, (const uint16_t*)d->w, d->bias, (uint16_t*)y_pad);
    else
        session_expand_kernel<float><<<grid, NT, 0, st>>>(args_of(d), (const float*)f, (const float*)d->w, d->bias, (float*)y_pad);
    MMFM_LAUNCH_CHECK("mmfm_session_expand");
    return 0;
}

extern "C" int mmfm_session_dw_chunks(int B, int S, int chunk) {
    MMFM_REQUIRE(B >= 1 && S >= 1 && chunk >= 1, "mmfm_session_dw_chunks: B %d, S %d, chunk %d must all be >= 1", B, S, chunk);
    return chunk_capacity(B, S, chunk);
}

extern "C" int64_t mmfm_session_runs_ints(int B, int S, int chunk) {
    MMFM_REQUIRE(B >= 1 && S >= 1 && chunk >= 1, "mmfm_session_runs_ints: B %d, S %d, chunk %d must all be >= 1", B, S, chunk);
    return RUN_HDR + (int64_t)B + (int64_t)RUN_ENT * chunk_capacity(B, S, chunk);
}

extern "C" int64_t mmfm_session_dw_workspace(int B, int P, int N_max, int S, int chunk) {
    MMFM_REQUIRE(B >= 1 && P >= 1 && N_max >= 1 && S >= 1 && chunk >= 1, "mmfm_session_dw_workspace: B %d, P %d, N_max %d, S %d, chunk %d must all be >= 1",
                 B, P, N_max, S, chunk);
    return (int64_t)chunk_capacity(B, S, chunk) * slab_elems(P, N_max) * (int64_t)sizeof(float);
}

extern "C" int mmfm_session_dw(const mmfm_session_desc* d, const void* a_pad, const void* q, const int32_t* runs, int chunk, float* dw, float* db,
                               int bias_from_pad, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    if (int rc = check_desc(d, "mmfm_session_dw", false)) return rc;
    MMFM_REQUIRE(a_pad && q && runs && dw, "mmfm_session_dw: NULL operand (a_pad %p, q %p, runs %p, dw %p)", a_pad, q, (const void*)runs, (void*)dw);
    MMFM_REQUIRE(chunk >= 1, "mmfm_session_dw: chunk %d", chunk);
    MMFM_REQUIRE(bias_from_pad == 0 || bias_from_pad == 1, "mmfm_session_dw: bias_from_pad %d", bias_from_pad);
    MMFM_REQUIRE(!db || (d->b_off && d->b_elems >= 1), "mmfm_session_dw: a bias gradient needs b_off and b_elems");
    const int cap = chunk_capacity(d->B, d->S, chunk);
    MMFM_REQUIRE(cap <= 65535, "mmfm_session_dw: %d chunks beyond the grid limit", cap);
    const int64_t stride = slab_elems(d->P, d->N_max), need = (int64_t)cap * stride * (int64_t)sizeof(float);
    MMFM_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                 "mmfm_session_dw: workspace %p of %lld bytes, need %lld (16-byte aligned)", workspace, (long long)workspace_bytes, (long long)need);
    const int64_t red = (int64_t)d->N_max * d->P + (d->N_max > d->P ? d->N_max : d->P);
    MMFM_REQUIRE(cdiv(red, 256) <= 0x7fffffffL, "mmfm_session_dw: N_max %d x P %d too large", d->N_max, d->P);
    const dim3 grid(cdiv(d->P, TN), cdiv(d->N_max, TM), cap);
    hipStream_t st = (hipStream_t)stream;
    float* slabs = (float*)workspace;
    if (d->dtype == MMFM_BF16)
        session_dw_kernel<uint16_t><<<grid, NT, 0, st>>>(args_of(d), (const uint16_t*)a_pad, (const uint16_t*)q, runs, cap, dw, db, bias_from_pad, slabs, stride);
    else
        session_dw_kernel<float><<<grid, NT, 0, st>>>(args_of(d), (const float*)a_pad, (const float*)q, runs, cap, dw, db, bias_from_pad, slabs, stride);
    MMFM_LAUNCH_CHECK("mmfm_session_dw");
    session_dw_reduce_kernel<<<dim3(cdiv(red, 256), cap), 256, 0, st>>>(args_of(d), runs, cap, dw, db, bias_from_pad, slabs, stride);
    MMFM_LAUNCH_CHECK("mmfm_session_dw (slab reduction)");
    return 0;
}
