// Fused AdamW over a flat fp32 range (+ bf16 weight refresh), elementwise dropout, casts.
// HBM-bound: AdamW moves 28 B/param (read p,g,m,v; write p,m,v) + 2 B with the bf16 copy.
#include "common.h"
#include <algorithm>

namespace {

// hyper (device): [0] 1-lr*wd  [1] 1-beta1  [2] beta2  [3] 1-beta2  [4] lr/bias_corr1
//                 [5] sqrt(bias_corr2)  [6] eps  [7] grad_scale      (host computes them in double)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, uint16_t* __restrict__ pb, int64_t n,
                                                    const float* __restrict__ hyper) {
    const float decay = hyper[0], omb1 = hyper[1], b2 = hyper[2], omb2 = hyper[3], step = hyper[4], bc2s = hyper[5], eps = hyper[6],
                gs = hyper[7];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        float pi = p[i] * decay;
        const float mi = m[i] + omb1 * (gi - m[i]);           // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * b2 + omb2 * gi * gi;          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(vi) / bc2s + eps;
        pi -= step * (mi / denom);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (pb) pb[i] = f2bf(pi);
    }
}

template <typename T>
__global__ void dropout_apply_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t n, mmfm_dropout da) {
    const Drop dr = drop_init(da);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        io<T>::st(dst + i, dr.apply(io<T>::ld(src + i), (uint64_t)i));
}

// bf16, n % 8 == 0, 16-B aligned: 8 elements per thread (the scalar kernel above moves 2 B per lane: 3.3 TB/s)
__global__ __launch_bounds__(256) void dropout_apply8_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t n8, mmfm_dropout da) {
    const Drop dr = drop_init(da);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 g = *reinterpret_cast<const uint4*>(src + 8 * i);
        const uint32_t gw[4] = {g.x, g.y, g.z, g.w};
        uint32_t ow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v0 = dr.apply(__uint_as_float(gw[j] << 16), (uint64_t)(8 * i + 2 * j));
            const float v1 = dr.apply(__uint_as_float(gw[j] & 0xffff0000u), (uint64_t)(8 * i + 2 * j + 1));
            ow[j] = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
        }
        *reinterpret_cast<uint4*>(dst + 8 * i) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
}

__global__ void cast_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = f2bf(src[i]);
}

int ew_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

// ------------------------------------------------------------------ the range-table optimiser (include/mmfm.h, MMFM_OPTIM_RANGES)
// A workgroup of 256 lanes walks one chunk's CHUNK-aligned window in OPT_QUADS passes; lane t of pass q owns the four elements
// window + 4 * (256 q + t) .. + 3.  A quad that lies inside the chunk moves as 16 bytes (VEC: every buffer is 16-B aligned, the window
// is too); a quad the chunk's head or tail cuts, and every quad without VEC, goes element by element.  The assignment depends on the
// element's index only - never on the grid.
constexpr int OPT_CHUNK = MMFM_OPTIM_CHUNK;
constexpr int OPT_QUADS = OPT_CHUNK / (4 * 256);
static_assert(OPT_CHUNK % (4 * 256) == 0 && (OPT_CHUNK & (OPT_CHUNK - 1)) == 0, "a chunk is a power-of-two number of 256-lane float4 passes");
static_assert(sizeof(mmfm_optim_chunk) == 24 && sizeof(mmfm_optim_record) == 32 && sizeof(mmfm_optim_range) == 24, "range-table ABI");

struct AdamwHyper {
    float decay, omb1, b2, omb2, step, bc2s, eps, gs;
};

// adamw_kernel's update with every rounding written out.  hipcc contracts adamw_kernel's expressions into the fused multiply-adds below
// (read from its gfx950 code: v = fma(gi, omb2 gi, b2 v); m = fma(omb1, fma(gs, g, -m), m), the inner one on the UNROUNDED gs g;
// p = fma(decay, p, -(step q))); inlined into another loop the same expressions contract differently, so contraction is off here and
// the choice is explicit.  The GPU tests compare the two kernels bit for bit.  gx is the gradient before grad_scale.
__device__ __forceinline__ void adamw_update(const AdamwHyper& h, float gx, float& pi, float& mi, float& vi) {
#pragma clang fp contract(off)
    const float gi = gx * h.gs;
    vi = __builtin_fmaf(gi, h.omb2 * gi, vi * h.b2);
    mi = __builtin_fmaf(h.omb1, __builtin_fmaf(h.gs, gx, -mi), mi);
    const float denom = sqrtf(vi) / h.bc2s + h.eps;
    pi = __builtin_fmaf(h.decay, pi, -(h.step * (mi / denom)));
}

template <bool VEC>
__global__ __launch_bounds__(256) void adamw_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, uint16_t* __restrict__ pb, int64_t n,
                                                           const mmfm_optim_chunk* __restrict__ chunks, int64_t n_chunks,
                                                           const float* __restrict__ hyper, const mmfm_optim_record* __restrict__ rec,
                                                           int skip) {
    float clip = 1.0f;
    if (rec) {
        if (skip && rec->nonfinite) return;          // uniform over the grid: nobody stores anything
        clip = rec->clip_coef;
    }
    const bool clipped = rec != nullptr;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const mmfm_optim_chunk ch = chunks[c];
        const float* hr = hyper + 8 * (int64_t)ch.hyper_row;
        const AdamwHyper h = {hr[0], hr[1], hr[2], hr[3], hr[4], hr[5], hr[6], hr[7]};
        const int64_t lo = std::max<int64_t>(ch.start, 0), hi = std::min<int64_t>(ch.start + ch.len, n);   // a table never reaches past n
        const int64_t base = lo & ~(int64_t)(OPT_CHUNK - 1);
#pragma unroll
        for (int q = 0; q < OPT_QUADS; ++q) {
            const int64_t i0 = base + 4 * (q * 256 + (int)threadIdx.x);
            if (i0 + 4 <= lo || i0 >= hi) continue;
            if (VEC && i0 >= lo && i0 + 4 <= hi) {
                const float4 g4 = *reinterpret_cast<const float4*>(g + i0);
                float4 p4 = *reinterpret_cast<const float4*>(p + i0), m4 = *reinterpret_cast<const float4*>(m + i0),
                       v4 = *reinterpret_cast<const float4*>(v + i0);
                const float gr[4] = {g4.x, g4.y, g4.z, g4.w};
                float pr[4] = {p4.x, p4.y, p4.z, p4.w}, mr[4] = {m4.x, m4.y, m4.z, m4.w}, vr[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) adamw_update(h, clipped ? gr[j] * clip : gr[j], pr[j], mr[j], vr[j]);
                *reinterpret_cast<float4*>(p + i0) = make_float4(pr[0], pr[1], pr[2], pr[3]);
                *reinterpret_cast<float4*>(m + i0) = make_float4(mr[0], mr[1], mr[2], mr[3]);
                *reinterpret_cast<float4*>(v + i0) = make_float4(vr[0], vr[1], vr[2], vr[3]);
                if (pb)
                    *reinterpret_cast<uint2*>(pb + i0) = make_uint2((uint32_t)f2bf(pr[0]) | ((uint32_t)f2bf(pr[1]) << 16),
                                                                    (uint32_t)f2bf(pr[2]) | ((uint32_t)f2bf(pr[3]) << 16));
            } else {
                for (int j = 0; j < 4; ++j) {
                    const int64_t i = i0 + j;
                    if (i < lo || i >= hi) continue;
                    float pi = p[i], mi = m[i], vi = v[i];
                    adamw_update(h, clipped ? g[i] * clip : g[i], pi, mi, vi);
                    p[i] = pi; m[i] = mi; v[i] = vi;
                    if (pb) pb[i] = f2bf(pi);
                }
            }
        }
    }
}

// one fp64 partial per chunk: x = g * coef in fp32 (the value the update forms), x * x + acc in fp64 from the first addition
template <bool VEC>
__global__ __launch_bounds__(256) void sumsq_ranges_kernel(const float* __restrict__ g, int64_t n, const mmfm_optim_chunk* __restrict__ chunks,
                                                           int64_t n_chunks, float coef, double* __restrict__ partial) {
    __shared__ double red[4];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const mmfm_optim_chunk ch = chunks[c];
        const int64_t lo = std::max<int64_t>(ch.start, 0), hi = std::min<int64_t>(ch.start + ch.len, n);
        const int64_t base = lo & ~(int64_t)(OPT_CHUNK - 1);
        double acc = 0.0;
        if (VEC && hi - lo == OPT_CHUNK) {
            // a whole chunk (nearly all of them): workgroup-uniform, no bounds test, and all four 16-byte loads of the lane are requested
            // before the first is used.  Same lanes, same elements, same order of additions as the general path below.
            float4 gq[OPT_QUADS];
#pragma unroll
            for (int q = 0; q < OPT_QUADS; ++q) gq[q] = *reinterpret_cast<const float4*>(g + base + 4 * (q * 256 + (int)threadIdx.x));
#pragma unroll
            for (int q = 0; q < OPT_QUADS; ++q) {
                const double x0 = (double)(gq[q].x * coef), x1 = (double)(gq[q].y * coef), x2 = (double)(gq[q].z * coef), x3 = (double)(gq[q].w * coef);
                acc = fma(x0, x0, acc); acc = fma(x1, x1, acc); acc = fma(x2, x2, acc); acc = fma(x3, x3, acc);
            }
        } else {
#pragma unroll
            for (int q = 0; q < OPT_QUADS; ++q) {
                const int64_t i0 = base + 4 * (q * 256 + (int)threadIdx.x);
                if (i0 + 4 <= lo || i0 >= hi) continue;
                if (VEC && i0 >= lo && i0 + 4 <= hi) {
                    const float4 g4 = *reinterpret_cast<const float4*>(g + i0);
                    const double x0 = (double)(g4.x * coef), x1 = (double)(g4.y * coef), x2 = (double)(g4.z * coef), x3 = (double)(g4.w * coef);
                    acc = fma(x0, x0, acc); acc = fma(x1, x1, acc); acc = fma(x2, x2, acc); acc = fma(x3, x3, acc);
                } else {
                    for (int j = 0; j < 4; ++j) {
                        const int64_t i = i0 + j;
                        if (i < lo || i >= hi) continue;
                        const double x = (double)(g[i] * coef);
                        acc = fma(x, x, acc);
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);     // butterfly: the same tree in every lane
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partial[c] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();                                                            // red is reused by the next chunk
    }
}

// one workgroup: each range's partials in chunk order, the range sums in range order, then the record.  Lane t of a group of 256
// ranges owns range r0 + t; the group's partials are contiguous in the workspace (chunks lie in range order) and pass through LDS in
// tiles, so the loads are coalesced round trips of the whole workgroup and only the additions - one dependent chain per range, as the
// order demands - are serial.  Lane 0 adds the group's range sums, in range order, into the running total.
constexpr int FIN_TILE = 512;
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ first, int n_ranges,
                                                           float max_norm, int skip, mmfm_optim_record* __restrict__ rec,
                                                           double* __restrict__ range_sumsq) {
    __shared__ double tile[FIN_TILE];
    __shared__ double sums[256];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    double total = 0.0;                                  // lane 0's
    for (int r0 = 0; r0 < n_ranges; r0 += 256) {
        const int r = r0 + t, r_end = r0 + 256 < n_ranges ? r0 + 256 : n_ranges;
        const int32_t my_lo = r < n_ranges ? first[r] : 0, my_hi = r < n_ranges ? first[r + 1] : 0;
        const int32_t span_lo = first[r0], span_hi = first[r_end];
        double s = 0.0;
        for (int32_t tb = span_lo; tb < span_hi; tb += FIN_TILE) {
            const int32_t cnt = span_hi - tb < FIN_TILE ? span_hi - tb : FIN_TILE;
            __syncthreads();                             // the previous tile (and `sums`) has been read
            for (int32_t i = t; i < cnt; i += 256) tile[i] = partial[tb + i];
            __syncthreads();
            const int32_t lo = my_lo > tb ? my_lo : tb, hi = my_hi < tb + cnt ? my_hi : tb + cnt;
            // sixteen LDS reads in flight, then their additions in chunk order: the chain of additions is what the order costs, the
            // read latency is not
            int32_t c = lo;
            for (; c + 16 <= hi; c += 16) {
                double d[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) d[k] = tile[c - tb + k];
#pragma unroll
                for (int k = 0; k < 16; ++k) s += d[k];
            }
            for (; c < hi; ++c) s += tile[c - tb];
        }
        if (r < n_ranges) range_sumsq[r] = s;
        // the partials are sums of squares: none is negative, so an inf or NaN among them stays in s (inf + x = inf, NaN + x = NaN)
        if (!isfinite(s)) atomicOr(&bad, 1);             // an integer flag in LDS; no floating-point atomic anywhere
        __syncthreads();
        sums[t] = s;
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < r_end - r0; ++k) total += sums[k];
    }
    __syncthreads();
    if (t == 0) {
        const int nonfinite = (bad || !isfinite(total)) ? 1 : 0;
        float coef = 1.0f;
        if (max_norm > 0.0f && isfinite(max_norm)) {
            const double cc = (double)max_norm / (sqrt(total) + 1e-6);
            if (cc < 1.0) coef = (float)cc;          // a NaN total compares false: 1
        }
        rec->total = total;
        rec->clip_coef = coef;
        rec->nonfinite = nonfinite;
        if (nonfinite && skip) rec->skipped = rec->skipped + 1;
        rec->n_ranges = n_ranges;
        rec->reserved = 0;
    }
}

// the argument checks of every range entry point; the number of chunks, or -1 with the error set.  No HIP call.
int64_t optim_ranges_check(const char* who, const mmfm_optim_range* ranges, int n_ranges, int64_t n, int hyper_rows) {
    if (!ranges || n_ranges <= 0 || n <= 0 || hyper_rows <= 0)
        return mmfm_set_error(-1, "%s: bad arguments (ranges %p, n_ranges %d, n %lld, hyper_rows %d)", who, (const void*)ranges, n_ranges,
                              (long long)n, hyper_rows);
    int64_t chunks = 0, prev_end = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const mmfm_optim_range& x = ranges[r];
        if (x.start < 0 || x.end <= x.start)
            return mmfm_set_error(-1, "%s: range %d [%lld, %lld) is empty or negative", who, r, (long long)x.start, (long long)x.end);
        if (x.start < prev_end)
            return mmfm_set_error(-1, "%s: range %d [%lld, %lld) overlaps or precedes range %d (ranges are sorted and disjoint)", who, r,
                                  (long long)x.start, (long long)x.end, r - 1);
        if (x.end > n) return mmfm_set_error(-1, "%s: range %d [%lld, %lld) reaches past n = %lld", who, r, (long long)x.start, (long long)x.end, (long long)n);
        if (x.hyper_row < 0 || x.hyper_row >= hyper_rows)
            return mmfm_set_error(-1, "%s: range %d names hyper row %d of %d", who, r, x.hyper_row, hyper_rows);
        chunks += (x.end - 1) / OPT_CHUNK - x.start / OPT_CHUNK + 1;
        prev_end = x.end;
    }
    if (chunks > INT32_MAX) return mmfm_set_error(-1, "%s: %lld chunks do not fit the table's int32 index", who, (long long)chunks);
    return chunks;
}

int opt_blocks(int64_t n_chunks) { return (int)std::min<int64_t>(4096, n_chunks); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------ gradient accumulation (include/mmfm.h, MMFM_GRAD_ACCUM)
// Elements [lo, hi) of two flat fp32 buffers; ADD: g += stash, otherwise stash = g.  [a0, a1) is the interior whose quads are 16-byte
// aligned in BOTH buffers (empty where the two disagree modulo 16 bytes: everything is head then).  Quad q of the interior belongs to
// one lane of the grid-stride walk; the at most three elements of the head [lo, a0) and of the tail [a1, hi) belong to the first
// lanes of workgroup 0, and where there is no interior the "head" [lo, hi) is walked element by element.  One lane per element, one
// rounding per element: the grid changes nothing.
template <bool ADD>
__device__ __forceinline__ void accum_one(float* __restrict__ g, float* __restrict__ stash, int64_t i) {
    if (ADD) g[i] = g[i] + stash[i];
    else stash[i] = g[i];
}

template <bool ADD>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* __restrict__ g, float* __restrict__ stash, int64_t lo, int64_t a0,
                                                              int64_t a1, int64_t hi) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t nq = (a1 - a0) >> 2;
    for (int64_t q = tid; q < nq; q += step) {
        const int64_t i = a0 + 4 * q;
        if (ADD) {
            float4 x = *reinterpret_cast<const float4*>(g + i);
            const float4 s = *reinterpret_cast<const float4*>(stash + i);
            x.x = x.x + s.x; x.y = x.y + s.y; x.z = x.z + s.z; x.w = x.w + s.w;
            *reinterpret_cast<float4*>(g + i) = x;
        } else {
            *reinterpret_cast<float4*>(stash + i) = *reinterpret_cast<const float4*>(g + i);
        }
    }
    for (int64_t i = lo + tid; i < a0; i += step) accum_one<ADD>(g, stash, i);
    for (int64_t i = a1 + tid; i < hi; i += step) accum_one<ADD>(g, stash, i);
}

}  // namespace

extern "C" int64_t mmfm_optim_ranges_chunks(const mmfm_optim_range* ranges, int n_ranges, int64_t n, int hyper_rows) {
    return optim_ranges_check("mmfm_optim_ranges_chunks", ranges, n_ranges, n, hyper_rows);
}

extern "C" int64_t mmfm_optim_ranges_table_bytes(int64_t n_chunks, int n_ranges) {
    if (n_chunks <= 0 || n_ranges <= 0) return 0;
    return n_chunks * (int64_t)sizeof(mmfm_optim_chunk) + ((int64_t)n_ranges + 1) * (int64_t)sizeof(int32_t);
}

extern "C" int64_t mmfm_optim_ranges_workspace(int64_t n_chunks, int n_ranges) {
    if (n_chunks <= 0 || n_ranges <= 0) return 0;
    return (int64_t)sizeof(mmfm_optim_record) + ((int64_t)n_ranges + n_chunks) * (int64_t)sizeof(double);
}

extern "C" int mmfm_optim_ranges_table(const mmfm_optim_range* ranges, int n_ranges, int64_t n, int hyper_rows, void* table_host,
                                       int64_t table_bytes) {
    const int64_t n_chunks = optim_ranges_check("mmfm_optim_ranges_table", ranges, n_ranges, n, hyper_rows);
    if (n_chunks < 0) return -1;
    MMFM_REQUIRE(table_host && table_bytes >= mmfm_optim_ranges_table_bytes(n_chunks, n_ranges),
                 "mmfm_optim_ranges_table: table of %lld bytes, %lld needed", (long long)table_bytes,
                 (long long)mmfm_optim_ranges_table_bytes(n_chunks, n_ranges));
    mmfm_optim_chunk* ch = (mmfm_optim_chunk*)table_host;
    int32_t* first = (int32_t*)(ch + n_chunks);
    int64_t c = 0;
    for (int r = 0; r < n_ranges; ++r) {
        first[r] = (int32_t)c;
        for (int64_t k = ranges[r].start / OPT_CHUNK; k <= (ranges[r].end - 1) / OPT_CHUNK; ++k, ++c) {
            const int64_t lo = std::max<int64_t>(ranges[r].start, k * OPT_CHUNK), hi = std::min<int64_t>(ranges[r].end, (k + 1) * OPT_CHUNK);
            ch[c] = mmfm_optim_chunk{lo, (int32_t)(hi - lo), r, ranges[r].hyper_row, 0};
        }
    }
    first[n_ranges] = (int32_t)c;
    return 0;
}

extern "C" int mmfm_grad_sumsq_ranges(const float* g, int64_t n, const mmfm_optim_range* ranges, int n_ranges, const void* table,
                                      int64_t n_chunks, float coef_in, float max_norm, int skip_nonfinite, void* workspace,
                                      int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(g && table && workspace, "mmfm_grad_sumsq_ranges: NULL pointer (g %p, table %p, workspace %p)", (const void*)g, table, workspace);
    const int64_t want = optim_ranges_check("mmfm_grad_sumsq_ranges", ranges, n_ranges, n, 1 << 30);
    if (want < 0) return -1;
    MMFM_REQUIRE(n_chunks == want, "mmfm_grad_sumsq_ranges: the table has %lld chunks, these ranges cut into %lld", (long long)n_chunks, (long long)want);
    MMFM_REQUIRE(workspace_bytes >= mmfm_optim_ranges_workspace(n_chunks, n_ranges) && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)table & 7) == 0,
                 "mmfm_grad_sumsq_ranges: workspace of %lld bytes (%lld needed), workspace and table 8-byte aligned", (long long)workspace_bytes,
                 (long long)mmfm_optim_ranges_workspace(n_chunks, n_ranges));
    mmfm_optim_record* rec = (mmfm_optim_record*)workspace;
    double* range_sumsq = (double*)(rec + 1);
    double* partial = range_sumsq + n_ranges;
    const mmfm_optim_chunk* chunks = (const mmfm_optim_chunk*)table;
    const int32_t* first = (const int32_t*)(chunks + n_chunks);
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(g))
        hipLaunchKernelGGL(sumsq_ranges_kernel<true>, dim3(opt_blocks(n_chunks)), dim3(256), 0, st, g, n, chunks, n_chunks, coef_in, partial);
    else
        hipLaunchKernelGGL(sumsq_ranges_kernel<false>, dim3(opt_blocks(n_chunks)), dim3(256), 0, st, g, n, chunks, n_chunks, coef_in, partial);
    MMFM_LAUNCH_CHECK("mmfm_grad_sumsq_ranges");
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, first, n_ranges, max_norm, skip_nonfinite, rec,
                       range_sumsq);
    MMFM_LAUNCH_CHECK("mmfm_grad_sumsq_ranges (closing phase)");
    return 0;
}

extern "C" int mmfm_adamw_step_ranges(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const mmfm_optim_range* ranges,
                                      int n_ranges, const void* table, int64_t n_chunks, const float* hyper, int hyper_rows,
                                      const mmfm_optim_record* record, int skip_nonfinite, mmfm_stream stream) {
    MMFM_REQUIRE(p && g && m && v && table && hyper, "mmfm_adamw_step_ranges: NULL pointer (p %p, g %p, m %p, v %p, table %p, hyper %p)",
                 (void*)p, (const void*)g, (void*)m, (void*)v, table, (const void*)hyper);
    const int64_t want = optim_ranges_check("mmfm_adamw_step_ranges", ranges, n_ranges, n, hyper_rows);
    if (want < 0) return -1;
    MMFM_REQUIRE(n_chunks == want, "mmfm_adamw_step_ranges: the table has %lld chunks, these ranges cut into %lld", (long long)n_chunks, (long long)want);
    MMFM_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)record & 7) == 0, "mmfm_adamw_step_ranges: table and record are 8-byte aligned");
    const mmfm_optim_chunk* chunks = (const mmfm_optim_chunk*)table;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && ((uintptr_t)p_bf16 & 7) == 0;
    if (vec)
        hipLaunchKernelGGL(adamw_ranges_kernel<true>, dim3(opt_blocks(n_chunks)), dim3(256), 0, st, p, g, m, v, (uint16_t*)p_bf16, n, chunks, n_chunks,
                           hyper, record, skip_nonfinite);
    else
        hipLaunchKernelGGL(adamw_ranges_kernel<false>, dim3(opt_blocks(n_chunks)), dim3(256), 0, st, p, g, m, v, (uint16_t*)p_bf16, n, chunks, n_chunks,
                           hyper, record, skip_nonfinite);
    MMFM_LAUNCH_CHECK("mmfm_adamw_step_ranges");
    return 0;
}

extern "C" int mmfm_grad_accumulate(float* g, float* stash, int64_t n, int64_t start, int64_t end, int mode, mmfm_stream stream) {
    MMFM_REQUIRE(g && stash, "mmfm_grad_accumulate: NULL pointer (g %p, stash %p)", (void*)g, (void*)stash);
    MMFM_REQUIRE(start >= 0 && start <= end && end <= n, "mmfm_grad_accumulate: range [%lld, %lld) of n = %lld", (long long)start,
                 (long long)end, (long long)n);
    MMFM_REQUIRE(mode == MMFM_GRAD_STASH || mode == MMFM_GRAD_ADD, "mmfm_grad_accumulate: unknown mode %d", mode);
    if (start == end) return 0;
    int64_t a0 = end, a1 = end;                      // no 16-byte interior unless the two buffers agree modulo 16 bytes
    if ((((uintptr_t)g ^ (uintptr_t)stash) & 15) == 0 && ((uintptr_t)g & 3) == 0) {
        const int64_t mis = (int64_t)(((uintptr_t)(g + start) & 15) >> 2);
        a0 = std::min<int64_t>(end, start + ((4 - mis) & 3));
        a1 = a0 + ((end - a0) & ~(int64_t)3);
    }
    const int64_t work = std::max<int64_t>((a1 - a0) >> 2, std::max<int64_t>(a0 - start, end - a1));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (work + 255) / 256));
    if (mode == MMFM_GRAD_ADD)
        hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, stash, start, a0, a1, end);
    else
        hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, stash, start, a0, a1, end);
    MMFM_LAUNCH_CHECK("mmfm_grad_accumulate");
    return 0;
}

extern "C" int mmfm_adamw_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, const float* hyper, mmfm_stream stream) {
    MMFM_REQUIRE(p && g && m && v && hyper && n > 0, "mmfm_adamw_step: bad arguments");
    hipLaunchKernelGGL(adamw_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (uint16_t*)p_bf16, n, hyper);
    MMFM_LAUNCH_CHECK("mmfm_adamw_step");
    return 0;
}

extern "C" int mmfm_dropout_apply(int dtype, const void* src, void* dst, int64_t R, int N, mmfm_dropout drop, mmfm_stream stream) {
    MMFM_REQUIRE(src && dst && R > 0 && N > 0, "mmfm_dropout_apply: bad arguments");
    const int64_t n = R * N;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMFM_F32)
        hipLaunchKernelGGL(dropout_apply_kernel<float>, dim3(ew_blocks(n)), dim3(256), 0, st, (const float*)src, (float*)dst, n, drop);
    else if (dtype == MMFM_BF16 && n % 8 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0)
        hipLaunchKernelGGL(dropout_apply8_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, n / 8, drop);
    else if (dtype == MMFM_BF16)
        hipLaunchKernelGGL(dropout_apply_kernel<uint16_t>, dim3(ew_blocks(n)), dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, n, drop);
    else
        return mmfm_set_error(-1, "mmfm_dropout_apply: bad dtype %d", dtype);
    MMFM_LAUNCH_CHECK("mmfm_dropout_apply");
    return 0;
}

extern "C" int mmfm_cast_f32_to_bf16(const float* src, void* dst, int64_t n, mmfm_stream stream) {
    MMFM_REQUIRE(src && dst && n > 0, "mmfm_cast_f32_to_bf16: bad arguments");
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, src, (uint16_t*)dst, n);
    MMFM_LAUNCH_CHECK("mmfm_cast_f32_to_bf16");
    return 0;
}
