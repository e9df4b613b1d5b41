// Mask/index preparation and the per-modality "stitch" (tokens + modality/position embeddings
// scattered into the concatenated [B, M*T, H] sequence), forward and backward.
// mm.py:90-110,141-175,245-275; encoder_embeddings.py:56-61; decoder_embeddings.py:56-61.
// HBM-bound elementwise/gather work; index semantics are bit-exact (sample-0 quirk included).
#include "gemm_route.h"
#include <algorithm>

namespace {

constexpr int MAXM = 8;
// slot j of the stitched sequence: the tokens [off[j], off[j + 1]), its eval mask and its attention mask [B][off[j + 1] - off[j]]
// (mmfm_mask_prep: off[j] = j * T and one attention mask for every slot)
struct MaskSeg {
    const int64_t* p[MAXM];
    const int64_t* attn[MAXM];
    int64_t stride[MAXM];
    int64_t channels[MAXM];
    int off[MAXM + 1];
};

// ROWS (mmfm_mask_prep_rows): keep0 is [B][L], every sample's own row, and keep_any[l] (zeroed by zero_rows_kernel in front of this
// launch) is set where any sample keeps position l: every writer stores the same 1, so the outcome does not depend on their order
template <bool ROWS>
__global__ void mask_prep_kernel(MaskSeg src, int B, int L, int M, uint8_t* __restrict__ tokmask, uint8_t* __restrict__ keypad,
                                 uint8_t* __restrict__ keep0, uint8_t* __restrict__ keep_any, uint8_t* __restrict__ mod_id,
                                 unsigned long long* __restrict__ count) {
    unsigned long long local[MAXM];
#pragma unroll
    for (int m = 0; m < MAXM; ++m) local[m] = 0;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (int64_t)B * L; idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx / L), l = (int)(idx % L);
        int m = 0;
#pragma unroll
        for (int j = 1; j < MAXM; ++j)
            if (j < M && l >= src.off[j]) m = j;
        // (the slot's fields picked by compare-and-select: a struct in kernel arguments indexed by a run-time value goes to scratch)
        const int64_t* p = src.p[0];
        const int64_t* ap = src.attn[0];
        int64_t stride = src.stride[0];
        int o = 0, Tn = src.off[1];
#pragma unroll
        for (int j = 1; j < MAXM; ++j)
            if (j == m) { p = src.p[j]; ap = src.attn[j]; stride = src.stride[j]; o = src.off[j]; Tn = src.off[j + 1] - src.off[j]; }
        const int t = l - o;
        const int64_t a = ap[(size_t)b * Tn + t];
        const int64_t v = p[((size_t)b * Tn + t) * stride] & a;                     // mm.py:270
        tokmask[idx] = (uint8_t)(v != 0);
        keypad[idx] = (uint8_t)(a != 0);
        if (ROWS) {
            keep0[idx] = (uint8_t)(v != 1);                                          // the same comparison, per sample
            if (v != 1) keep_any[l] = 1;
            if (b == 0) mod_id[l] = (uint8_t)m;
        } else if (b == 0) {
            keep0[l] = (uint8_t)(v != 1);                                            // mm.py:145: argwhere(mask[0] == 1)
            mod_id[l] = (uint8_t)m;
        }
#pragma unroll
        for (int mm = 0; mm < MAXM; ++mm)
            if (mm == m) local[mm] += (unsigned long long)v * (unsigned long long)src.channels[mm];
    }
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
        if (m < M) {
            unsigned long long s = local[m];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&count[m], s);              // integer: order-independent, exact
        }
    }
}

// (a captured hipMemsetAsync node replayed with a stale fill pattern on this stack, so the counters are
// zeroed by a kernel of our own: plain stream order, identical eager and under hipGraph replay)
__global__ void zero_u64_kernel(unsigned long long* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0ull;
}
// the same for mmfm_mask_prep_rows: the counters and the L bytes of keep_any
__global__ void zero_rows_kernel(unsigned long long* p, int n, uint8_t* __restrict__ any, int L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0ull;
    if (i < L) any[i] = 0;
}

// The stitch kernels work on one slot: the Tn tokens from `off` of the stitched sequence of L.  The uniform and live-row entry points
// pass off = m * T, the segment ones (MMFM_MOD_SEGMENTS, include/mmfm.h) the slot's own offset, length and time stamps.
// The keep mask of (b, l) is keep0[b * kld + l]: kld = 0 is the one row shared by every sample (all entry points but the _rows ones,
// MMFM_TOKEN_MASK_ROWS), kld >= L every sample's own row.
template <typename T>
__global__ __launch_bounds__(256) void stitch_fwd_kernel(const T* __restrict__ tok, const float* __restrict__ mod_row,
                                                         const float* __restrict__ pos, const int64_t* __restrict__ ts,
                                                         const uint8_t* __restrict__ keep0, const int32_t* __restrict__ rec, T* __restrict__ x,
                                                         T* __restrict__ emb, int B, int Tn, int L, int off, int H, int max_F, int kld) {
    const int C4 = H / 4;
    const int64_t total = (int64_t)B * Tn * C4;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / C4;
        const int c = (int)(idx % C4) * 4;
        const int b = (int)(r / Tn), t = (int)(r % Tn);
        const int l = off + t;
        const float4 mr = *reinterpret_cast<const float4*>(mod_row + c);
        float4 e = mr;                                  // pos == NULL (embedder.pos: false): the modality row alone, ts is not read
        if (pos) {
            const int tsv = (int)min((int64_t)(max_F - 1), max((int64_t)0, ts[r]));     // memory-safe even for bad stamps
            const float4 pr = *reinterpret_cast<const float4*>(pos + (size_t)tsv * H + c);
            e = make_float4(mr.x + pr.x, mr.y + pr.y, mr.z + pr.z, mr.w + pr.w);
        }
        const size_t o = ((size_t)b * L + l) * H + c;
        if (emb) io<T>::st4(emb + o, e);
        if (keep0[(size_t)b * kld + l]) {
            // rec (mmfm_stitch_fwd_live): tok holds the live rows only, (b, t) at b * T_live + rank[t]
            const int64_t tr = rec ? (int64_t)b * rec[0] + rec[4 + Tn + t] : r;
            const float4 tv = io<T>::ld4(tok + (size_t)tr * H + c);
            e.x += tv.x; e.y += tv.y; e.z += tv.z; e.w += tv.w;
        }
        io<T>::st4(x + o, e);
    }
}

// block = CW threads (one column each); grid = (H/CW, nchunks); LDS table [max_F][CW].  POS = false (d_pos == NULL, embedder.pos: false):
// no table, no time stamps - a chunk's partial is its d_mod row alone (the caller passes max_F = 0)
template <typename T, bool POS>
__global__ void stitch_bwd_kernel(const T* __restrict__ dx, const T* __restrict__ dextra, const int64_t* __restrict__ ts,
                                  const uint8_t* __restrict__ keep0, const int32_t* __restrict__ rec, mmfm_dropout dropa,
                                  T* __restrict__ d_tok, float* __restrict__ part, int B, int Tn, int L, int off, int H, int max_F, int bper, int kld) {
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int CW = blockDim.x, j = threadIdx.x, col = blockIdx.x * CW + j;
    const Drop dr = drop_init(dropa);
    for (int f = 0; f < max_F; ++f) tab[f * CW + j] = 0.f;
    float macc = 0.f;
    const int b0 = blockIdx.y * bper, b1 = min(B, b0 + bper);
    for (int b = b0; b < b1; ++b) {
        for (int t = 0; t < Tn; ++t) {
            const int l = off + t;
            const size_t o = ((size_t)b * L + l) * H + col;
            const float g = io<T>::ld(dx + o);
            float e = g;
            if (dextra) e += io<T>::ld(dextra + o);
            const int64_t r = (int64_t)b * Tn + t;
            if (POS) {
                const int tsv = (int)min((int64_t)(max_F - 1), max((int64_t)0, ts[r]));
                tab[tsv * CW + j] += e;               // a thread owns its column: no race, fixed order
            }
            macc += e;
            const bool kp = keep0[(size_t)b * kld + l] != 0;
            if (d_tok && !rec) io<T>::st(d_tok + (size_t)r * H + col, kp ? dr.apply(g, (uint64_t)r * H + col) : 0.f);
            else if (d_tok && rec[4 + Tn + t] >= 0)        // live bins only, at their compact rows; the counter stays the original row's
                io<T>::st(d_tok + ((size_t)b * rec[0] + rec[4 + Tn + t]) * H + col, kp ? dr.apply(g, (uint64_t)r * H + col) : 0.f);
        }
    }
    float* out = part + (size_t)blockIdx.y * (max_F + 1) * H;
    for (int f = 0; f < max_F; ++f) out[(size_t)f * H + col] = tab[f * CW + j];
    out[(size_t)max_F * H + col] = macc;
}

// ---- bf16 throughput path of mmfm_stitch_bwd: the scatter d_pos[ts[b][t]] += e[b][t] and the sum d_mod += e ARE a matrix
// product with a one-hot matrix:  [d_pos; d_mod] = OH^T E,  OH[row][f] = (f == ts[row]), OH[row][max_F] = 1 for the rows of
// the slot (b, off + t) (zero rows elsewhere), E = dx viewed as [B*L][H].  It runs as a split-K dW-style launch of the bf16 MFMA GEMM
// (fp32 accumulation of exact 0/1 products = the plain fp32 sum, fixed order), 1 + 1 launches for dx and dextra; measured
// 429 us -> ~90 us per call at B = 1024 against the per-column LDS scatter kernel above (2-byte accesses, 4 waves/CU).
__global__ __launch_bounds__(256) void onehot_kernel(const int64_t* __restrict__ ts, uint16_t* __restrict__ oh, int B, int Tn, int L, int off,
                                                     int max_F, int ohc) {
    const int cpr = ohc / 8;
    const int64_t total = (int64_t)B * L * cpr;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cpr;
        const int c0 = (int)(idx % cpr) * 8;
        const int b = (int)(row / L), l = (int)(row % L), t = l - off;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (t >= 0 && t < Tn) {
            const int tsv = (int)min((int64_t)(max_F - 1), max((int64_t)0, ts[(int64_t)b * Tn + t]));
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + j == tsv || c0 + j == max_F) w[j >> 1] |= 0x3F80u << (16 * (j & 1));      // bf16 1.0
        }
        *reinterpret_cast<uint4*>(oh + row * ohc + c0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- bf16 path without a position table (d_pos == NULL): OH has the one column of ones, the product is the column sum of the modality's
// rows of E = dx + dextra.  grid (ceil(H / 256), S): slab s sums the rows (b, t) of samples [s * bper, (s + 1) * bper) - a thread owns 4
// columns, the block's 4 row lanes meet in LDS in a fixed order - and mmfm_reduce_slabs adds the S slabs: deterministic, no atomics.
__global__ __launch_bounds__(256) void stitch_modsum_kernel(const uint16_t* __restrict__ dx, const uint16_t* __restrict__ dextra,
                                                            float* __restrict__ part, int B, int Tn, int L, int off, int H, int bper) {
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + lane * 4;
    const int b0 = blockIdx.y * bper, b1 = min(B, b0 + bper);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < H) {
        for (int64_t r = (int64_t)b0 * Tn + rl; r < (int64_t)b1 * Tn; r += 4) {
            const size_t o = ((size_t)(r / Tn) * L + (size_t)off + (size_t)(r % Tn)) * H + c;
            float4 e = io<uint16_t>::ld4(dx + o);
            if (dextra) {
                const float4 x = io<uint16_t>::ld4(dextra + o);
                e.x += x.x; e.y += x.y; e.z += x.z; e.w += x.w;
            }
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
    }
    red[rl][lane] = acc;
    __syncthreads();
    if (rl == 0 && c < H) {
        float4 o;
        o.x = (red[0][lane].x + red[1][lane].x) + (red[2][lane].x + red[3][lane].x);
        o.y = (red[0][lane].y + red[1][lane].y) + (red[2][lane].y + red[3][lane].y);
        o.z = (red[0][lane].z + red[1][lane].z) + (red[2][lane].z + red[3][lane].z);
        o.w = (red[0][lane].w + red[1][lane].w) + (red[2][lane].w + red[3][lane].w);
        *reinterpret_cast<float4*>(part + (size_t)blockIdx.y * H + c) = o;
    }
}

// d_tok[b*T+t][:] = keep0[b*kld+off+t] ? dropout'(dx[b][off+t][:]) : 0      (bf16, 16-B accesses; H % 8 == 0)
__global__ __launch_bounds__(256) void stitch_dtok_kernel(const uint16_t* __restrict__ dx, const uint8_t* __restrict__ keep0,
                                                          const int32_t* __restrict__ rec, mmfm_dropout dropa,
                                                          uint16_t* __restrict__ d_tok, int B, int Tn, int L, int off, int H, int kld) {
    const Drop dr = drop_init(dropa);
    const int C8 = H / 8;
    const int64_t total = (int64_t)B * Tn * C8;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / C8;
        const int c = (int)(idx % C8) * 8;
        const int b = (int)(r / Tn), l = off + (int)(r % Tn);
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        // rec (mmfm_stitch_bwd_live): live bins only, at their compact rows; the dropout counter stays the original row's.  A bin is dead
        // where the mask the record was made from is 0: the shared row itself (kld = 0), or keep_any, the OR of the samples' rows - there
        // a live bin can be masked in this sample, and its compact row, which the weight-gradient product reads, gets zeros
        const int rank = rec ? rec[4 + Tn + (int)(r % Tn)] : 0;
        if (rank < 0) continue;
        const int64_t orow = rec ? (int64_t)b * rec[0] + rank : r;
        if (keep0[(size_t)b * kld + l]) {
            const uint4 g = *reinterpret_cast<const uint4*>(dx + ((size_t)b * L + l) * H + c);
            if (dr.on()) {
                const uint32_t gw[4] = {g.x, g.y, g.z, g.w};
                uint32_t ow[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v0 = dr.apply(__uint_as_float(gw[j] << 16), (uint64_t)r * H + c + 2 * j);
                    const float v1 = dr.apply(__uint_as_float(gw[j] & 0xffff0000u), (uint64_t)r * H + c + 2 * j + 1);
                    ow[j] = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
                }
                o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            } else {
                o = g;
            }
        }
        *reinterpret_cast<uint4*>(d_tok + (size_t)orow * H + c) = o;
    }
}

// Loader collate (loader/base.py:304-450, utils/dataset_utils.py:38-43): CSR (uint8 counts) ->
// dense [B][max_T][max_N] fp32, truncated / right-padded with pad_value, plus the two attention masks.
// One wavefront per (trial, time bin): the lanes fill the row (coalesced), then scatter the row's non-zeros with
// float atomic adds (duplicate (row, col) entries of a CSR add up, like scipy's toarray()).
struct CollateArgs {
    const uint8_t* data;
    const int32_t* indices;
    const int64_t* indptr;        // concatenated per-trial indptr arrays (T_b + 1 entries each)
    const int64_t* indptr_off;    // [B] offset of trial b's indptr
    const int64_t* nnz_off;       // [B] offset of trial b's data/indices
    const int32_t* T_b;
    const int32_t* N_b;
};
__global__ __launch_bounds__(256) void collate_csr_kernel(CollateArgs a, int B, int max_T, int max_N, float pad, float* __restrict__ out,
                                                          int64_t* __restrict__ tmask, int64_t* __restrict__ smask) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < (int64_t)B * max_T; row += (int64_t)gridDim.x * 4) {
        const int b = (int)(row / max_T), t = (int)(row % max_T);
        const int Tb = a.T_b[b], Nb = a.N_b[b];
        const bool live = t < Tb;                       // rows past the trial's length are padding
        const int nvalid = min(Nb, max_N);
        float* o = out + row * max_N;
        for (int n = lane; n < max_N; n += 64) o[n] = (live && n < nvalid) ? 0.f : pad;
        if (lane == 0) tmask[row] = live ? 1 : 0;
        if (t == 0)
            for (int n = lane; n < max_N; n += 64) smask[(size_t)b * max_N + n] = n < nvalid ? 1 : 0;
        if (!live) continue;
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
        const int64_t* ip = a.indptr + a.indptr_off[b];
        const int64_t z0 = ip[t], z1 = ip[t + 1], base = a.nnz_off[b];
        for (int64_t z = z0 + lane; z < z1; z += 64) {
            const int col = a.indices[base + z];
            if (col >= 0 && col < nvalid) atomicAdd(o + col, (float)a.data[base + z]);
        }
    }
}

int pick_cw(int H, int max_F) {
    for (int cw : {256, 128, 64, 32, 16, 8, 4})
        if (H % cw == 0 && (size_t)max_F * cw * 4 <= 60 * 1024) return cw;
    return 0;
}
int stitch_chunks(int B, int H, int cw) { return std::max(1, std::min(B, 512 / std::max(1, H / cw))); }
// one-hot GEMM path (bf16, H % 8 == 0): split-K geometry over K = B*L rows and the workspace carve-up
struct OhGeo { int ohc, S, kchunk; int64_t oh_bytes, slab; };
OhGeo oh_geo(int B, int L, int H, int max_F) {
    OhGeo g;
    g.ohc = (max_F + 1 + 7) & ~7;
    const int64_t K = (int64_t)B * L;
    const int tiles = ((max_F + 1 + 127) / 128) * ((H + 127) / 128);
    int S = (int)std::max<int64_t>(1, std::min<int64_t>(K / 512, (512 + tiles - 1) / tiles));
    g.kchunk = (int)(((K + S - 1) / S + 63) / 64 * 64);
    g.S = (int)((K + g.kchunk - 1) / g.kchunk);
    g.oh_bytes = ((int64_t)K * g.ohc * 2 + 255) / 256 * 256;
    g.slab = (int64_t)(max_F + 1) * H;
    return g;
}
bool oh_path(int dtype, int H) { return dtype == MMFM_BF16 && H % 8 == 0; }

}  // namespace

extern "C" int mmfm_reduce_slabs(float*, const float*, int64_t, int, int64_t, int, mmfm_stream);

// The mask-prep entry points: the slot table from the per-slot lengths and attention masks, then the counters zeroed and the kernel.
// keep_any: NULL - keep0 is the shared row [L]; set (mmfm_mask_prep_rows) - keep0 is [B][L] and keep_any [L] their OR over the samples.
static int mask_prep_impl(const char* what, int B, int M, const int32_t* seg_T, const int64_t* const* mask_src, const int64_t* mask_stride,
                          const int64_t* const* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad, uint8_t* keep0,
                          uint8_t* keep_any, uint8_t* mod_id, int64_t* count, mmfm_stream stream) {
    MaskSeg src;
    src.off[0] = 0;
    for (int m = 0; m < MAXM; ++m) {
        src.p[m] = m < M ? mask_src[m] : nullptr;
        src.attn[m] = m < M ? attn[m] : nullptr;
        src.stride[m] = m < M ? mask_stride[m] : 0;
        src.channels[m] = m < M ? channels[m] : 0;
        MMFM_REQUIRE(m >= M || (src.p[m] && src.attn[m] && src.stride[m] > 0 && seg_T[m] > 0 && seg_T[m] <= 65535),
                     "%s: slot %d has no mask source, no attention mask or no bins", what, m);
        src.off[m + 1] = src.off[m] + (m < M ? seg_T[m] : 0);
    }
    const int L = src.off[M];
    MMFM_REQUIRE(L <= 65535, "%s: sequence too long", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)B * L;
    const dim3 grid((int)std::min<int64_t>(256, (n + 255) / 256));
    if (keep_any) {
        hipLaunchKernelGGL(zero_rows_kernel, dim3(cdiv(std::max(L, M), 256)), dim3(256), 0, st, (unsigned long long*)count, M, keep_any, L);
        MMFM_LAUNCH_CHECK(what);
        hipLaunchKernelGGL(mask_prep_kernel<true>, grid, dim3(256), 0, st, src, B, L, M, tokmask, keypad, keep0, keep_any, mod_id,
                           (unsigned long long*)count);
        MMFM_LAUNCH_CHECK(what);
        return 0;
    }
    hipLaunchKernelGGL(zero_u64_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)count, M);
    MMFM_LAUNCH_CHECK(what);
    hipLaunchKernelGGL(mask_prep_kernel<false>, grid, dim3(256), 0, st, src, B, L, M, tokmask, keypad, keep0, (uint8_t*)nullptr, mod_id,
                       (unsigned long long*)count);
    MMFM_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int mmfm_mask_prep(int B, int T, int M, const int64_t* const* mask_src, const int64_t* mask_stride,
                              const int64_t* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad,
                              uint8_t* keep0, uint8_t* mod_id, int64_t* count, mmfm_stream stream) {
    MMFM_REQUIRE(B > 0 && T > 0 && M > 0 && M <= MAXM, "mmfm_mask_prep: bad shape B=%d T=%d M=%d (M <= %d)", B, T, M, MAXM);
    MMFM_REQUIRE(mask_src && mask_stride && attn && channels && tokmask && keypad && keep0 && mod_id && count, "mmfm_mask_prep: null pointer");
    int32_t seg_T[MAXM];
    const int64_t* attns[MAXM];
    for (int m = 0; m < MAXM; ++m) { seg_T[m] = T; attns[m] = attn; }       // slot j at j * T, one attention mask for all
    return mask_prep_impl("mmfm_mask_prep", B, M, seg_T, mask_src, mask_stride, attns, channels, tokmask, keypad, keep0, nullptr, mod_id, count, stream);
}

extern "C" int mmfm_mask_prep_seg(int B, int M, const int32_t* seg_T, const int64_t* const* mask_src, const int64_t* mask_stride,
                                  const int64_t* const* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad, uint8_t* keep0,
                                  uint8_t* mod_id, int64_t* count, mmfm_stream stream) {
    static_assert(MAXM == MMFM_MAX_SEGMENTS, "mmfm_mask_prep and the segment table hold the same number of slots");
    MMFM_REQUIRE(B > 0 && M > 0 && M <= MAXM, "mmfm_mask_prep_seg: bad shape B=%d M=%d (M <= %d)", B, M, MAXM);
    MMFM_REQUIRE(seg_T && mask_src && mask_stride && attn && channels && tokmask && keypad && keep0 && mod_id && count, "mmfm_mask_prep_seg: null pointer");
    return mask_prep_impl("mmfm_mask_prep_seg", B, M, seg_T, mask_src, mask_stride, attn, channels, tokmask, keypad, keep0, nullptr, mod_id, count, stream);
}

extern "C" int mmfm_mask_prep_rows(int B, int M, const int32_t* seg_T, const int64_t* const* mask_src, const int64_t* mask_stride,
                                   const int64_t* const* attn, const int64_t* channels, uint8_t* tokmask, uint8_t* keypad, uint8_t* keep,
                                   uint8_t* keep_any, uint8_t* mod_id, int64_t* count, mmfm_stream stream) {
    MMFM_REQUIRE(B > 0 && M > 0 && M <= MAXM, "mmfm_mask_prep_rows: bad shape B=%d M=%d (M <= %d)", B, M, MAXM);
    MMFM_REQUIRE(seg_T && mask_src && mask_stride && attn && channels && tokmask && keypad && keep && keep_any && mod_id && count,
                 "mmfm_mask_prep_rows: null pointer");
    return mask_prep_impl("mmfm_mask_prep_rows", B, M, seg_T, mask_src, mask_stride, attn, channels, tokmask, keypad, keep, keep_any, mod_id, count,
                          stream);
}

extern "C" int mmfm_collate_csr(int B, int max_T, int max_N, float pad_value, const uint8_t* data, const int32_t* indices,
                                const int64_t* indptr, const int64_t* indptr_off, const int64_t* nnz_off, const int32_t* T_b,
                                const int32_t* N_b, float* out, int64_t* time_mask, int64_t* space_mask, mmfm_stream stream) {
    MMFM_REQUIRE(B > 0 && max_T > 0 && max_N > 0, "mmfm_collate_csr: bad shape");
    MMFM_REQUIRE(indptr && indptr_off && nnz_off && T_b && N_b && out && time_mask && space_mask, "mmfm_collate_csr: null pointer");
    CollateArgs a{data, indices, indptr, indptr_off, nnz_off, T_b, N_b};
    const int64_t rows = (int64_t)B * max_T;
    hipLaunchKernelGGL(collate_csr_kernel, dim3((int)std::min<int64_t>(4096, (rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, B, max_T,
                       max_N, pad_value, out, time_mask, space_mask);
    MMFM_LAUNCH_CHECK("mmfm_collate_csr");
    return 0;
}

// The three stitch forwards.  what: the entry point's name, for its messages; off: the slot's first token (int64: m * T of the uniform
// forms is checked here before it is narrowed); rec: the live-bin record of mmfm_stitch_fwd_live, else NULL; keep_ld: 0, or the row
// stride of a per-sample keep mask (mmfm_stitch_fwd_rows).
static int stitch_fwd_impl(const char* what, int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb, const int64_t* ts,
                           const uint8_t* keep0, int keep_ld, const int32_t* rec, void* x, void* emb, int B, int T, int L, int64_t off, int H,
                           int max_F, mmfm_stream stream) {
    MMFM_REQUIRE(tok && mod_emb_row && (ts || !pos_emb) && keep0 && x, "%s: null pointer", what);       // pos_emb NULL: no position table
    MMFM_REQUIRE(B > 0 && T > 0 && H > 0 && H % 4 == 0 && off >= 0 && off + T <= L && max_F > 0, "%s: bad shape", what);
    const int64_t n = (int64_t)B * T * (H / 4);
    dim3 grid((int)std::min<int64_t>(4096, (n + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MMFM_F32)
        hipLaunchKernelGGL(stitch_fwd_kernel<float>, grid, block, 0, st, (const float*)tok, mod_emb_row, pos_emb, ts, keep0, rec, (float*)x, (float*)emb, B, T, L, (int)off, H, max_F, keep_ld);
    else if (dtype == MMFM_BF16)
        hipLaunchKernelGGL(stitch_fwd_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)tok, mod_emb_row, pos_emb, ts, keep0, rec, (uint16_t*)x, (uint16_t*)emb, B, T, L, (int)off, H, max_F, keep_ld);
    else
        return mmfm_set_error(-1, "%s: bad dtype %d", what, dtype);
    MMFM_LAUNCH_CHECK(what);
    return 0;
}
extern "C" int mmfm_stitch_fwd(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb, const int64_t* ts,
                               const uint8_t* keep0, void* x, void* emb, int B, int T, int L, int m, int H, int max_F, mmfm_stream stream) {
    return stitch_fwd_impl("mmfm_stitch_fwd", dtype, tok, mod_emb_row, pos_emb, ts, keep0, 0, nullptr, x, emb, B, T, L, (int64_t)m * T, H, max_F, stream);
}
extern "C" int mmfm_stitch_fwd_live(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb, const int64_t* ts,
                                    const uint8_t* keep0, const int32_t* rec, void* x, void* emb, int B, int T, int L, int m, int H, int max_F,
                                    mmfm_stream stream) {
    MMFM_REQUIRE(rec, "mmfm_stitch_fwd_live: null live-bin record");
    return stitch_fwd_impl("mmfm_stitch_fwd_live", dtype, tok, mod_emb_row, pos_emb, ts, keep0, 0, rec, x, emb, B, T, L, (int64_t)m * T, H, max_F, stream);
}
extern "C" int mmfm_stitch_fwd_seg(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb, const int64_t* ts,
                                   const uint8_t* keep0, void* x, void* emb, int B, int T, int L, int off, int H, int max_F, mmfm_stream stream) {
    return stitch_fwd_impl("mmfm_stitch_fwd_seg", dtype, tok, mod_emb_row, pos_emb, ts, keep0, 0, nullptr, x, emb, B, T, L, off, H, max_F, stream);
}
// The _rows pair (MMFM_TOKEN_MASK_ROWS): its own argument checks, then the same launches as every other entry point.
static int stitch_rows_args(const char* what, int dtype, const void* keep, int keep_ld, const int32_t* rec, int T, int L, int off) {
    MMFM_REQUIRE(keep, "%s: null pointer", what);
    MMFM_REQUIRE(keep_ld == 0 || keep_ld >= L, "%s: keep_ld = %d is neither 0 (one shared row) nor >= L = %d", what, keep_ld, L);
    MMFM_REQUIRE(T > 0 && off >= 0 && (int64_t)off + T <= L, "%s: the slot [%d, %d + %d) leaves the sequence of %d", what, off, off, T, L);
    MMFM_REQUIRE(!rec || dtype == MMFM_BF16, "%s: a live-bin record needs bf16", what);
    return 0;
}
extern "C" int mmfm_stitch_fwd_rows(int dtype, const void* tok, const float* mod_emb_row, const float* pos_emb, const int64_t* ts,
                                    const uint8_t* keep, int keep_ld, const int32_t* rec, void* x, void* emb, int B, int T, int L, int off, int H,
                                    int max_F, mmfm_stream stream) {
    if (int rc = stitch_rows_args("mmfm_stitch_fwd_rows", dtype, keep, keep_ld, rec, T, L, off)) return rc;
    return stitch_fwd_impl("mmfm_stitch_fwd_rows", dtype, tok, mod_emb_row, pos_emb, ts, keep, keep_ld, rec, x, emb, B, T, L, off, H, max_F, stream);
}

extern "C" int64_t mmfm_stitch_bwd_workspace(int dtype, int B, int T, int L, int H, int max_F) {
    (void)T;
    if (oh_path(dtype, H)) {
        const OhGeo g = oh_geo(B, L, H, max_F);
        return g.oh_bytes + 2 * (int64_t)g.S * g.slab * (int64_t)sizeof(float);
    }
    const int cw = pick_cw(H, max_F);
    if (!cw) return -1;
    return (int64_t)stitch_chunks(B, H, cw) * (max_F + 1) * H * sizeof(float);
}
// (the bound depends on the whole sequence, not on where the slot lies in it: the one-hot matrix covers all B * L rows)
extern "C" int64_t mmfm_stitch_bwd_seg_workspace(int dtype, int B, int T, int L, int off, int H, int max_F) {
    (void)off;
    return mmfm_stitch_bwd_workspace(dtype, B, T, L, H, max_F);
}

// The three stitch backwards: what, off and rec as in stitch_fwd_impl.  Every check comes before the first launch.
static int stitch_bwd_impl(const char* what, int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0, int keep_ld,
                           const int32_t* rec, mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos, int B,
                           int T, int L, int64_t off64, int H, int max_F, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(dx && (ts || !d_pos) && keep0 && d_mod_row, "%s: null pointer", what);                        // d_pos NULL: no position table
    MMFM_REQUIRE(B > 0 && T > 0 && H > 0 && max_F > 0 && off64 >= 0 && off64 + T <= L, "%s: bad shape", what);
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "%s: bad dtype %d", what, dtype);
    const int64_t need = mmfm_stitch_bwd_workspace(dtype, B, T, L, H, max_F);
    MMFM_REQUIRE(need >= 0, "%s: no column slab fits LDS for H=%d max_F=%d", what, H, max_F);
    MMFM_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small", what);
    const int off = (int)off64;
    hipStream_t st = (hipStream_t)stream;
    if (oh_path(dtype, H)) {
        const OhGeo g = oh_geo(B, L, H, max_F);
        MMFM_REQUIRE((uintptr_t)dx % 16 == 0 && (!dextra || (uintptr_t)dextra % 16 == 0) && (!d_tok || (uintptr_t)d_tok % 16 == 0) &&
                     (uintptr_t)workspace % 16 == 0, "%s: bf16 tensors must be 16-byte aligned", what);
        if (d_tok) {
            const int64_t n = (int64_t)B * T * (H / 8);
            hipLaunchKernelGGL(stitch_dtok_kernel, dim3((int)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0, st, (const uint16_t*)dx, keep0,
                               rec, drop, (uint16_t*)d_tok, B, T, L, off, H, keep_ld);
        }
        if (!d_pos) {
            // the column sum: as many slabs of H floats as samples, at most 256, and no more than the workspace bound of the one-hot
            // product holds (mmfm_stitch_bwd_workspace does not know which form it sizes; it holds at least 2 (max_F + 1) such slabs)
            const int64_t room = need / ((int64_t)H * (int64_t)sizeof(float));
            const int S = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(B, 256), room));
            const int bper = (B + S - 1) / S, nsl = (B + bper - 1) / bper;
            hipLaunchKernelGGL(stitch_modsum_kernel, dim3(cdiv(H, 256), nsl), dim3(256), 0, st, (const uint16_t*)dx, (const uint16_t*)dextra,
                               (float*)workspace, B, T, L, off, H, bper);
            MMFM_LAUNCH_CHECK(what);
            return mmfm_reduce_slabs(d_mod_row, (const float*)workspace, H, nsl, H, acc_mod, stream);
        }
        uint16_t* oh = reinterpret_cast<uint16_t*>(workspace);
        float* slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + g.oh_bytes);
        const int64_t nch = (int64_t)B * L * (g.ohc / 8);
        hipLaunchKernelGGL(onehot_kernel, dim3((int)std::min<int64_t>(4096, (nch + 255) / 256)), dim3(256), 0, st, ts, oh, B, T, L, off, max_F, g.ohc);
        MMFM_LAUNCH_CHECK(what);
        mmfm_gemm_desc gd = {};
        gd.dtype = MMFM_BF16; gd.c_f32 = 1;
        gd.A = oh; gd.lda = g.ohc; gd.a_kcontig = 0;
        gd.ldb = H; gd.b_kcontig = 0;
        gd.M = max_F + 1; gd.N = H; gd.K = B * L; gd.ldc = H;
        gd.splits = g.S; gd.kchunk = g.kchunk; gd.slab_stride = g.slab;
        gd.act_scale = 1.f;
        int nsl = 0;
        for (const void* src : {dx, dextra}) {
            if (!src) continue;
            gd.B = src;
            gd.C = slabs + (int64_t)nsl * g.slab;
            if (int rc = mmfm_gemm_routed(gd, st)) return rc;
            nsl += g.S;
        }
        if (int rc = mmfm_reduce_slabs(d_pos, slabs, (int64_t)max_F * H, nsl, g.slab, acc_pos, stream)) return rc;
        return mmfm_reduce_slabs(d_mod_row, slabs + (int64_t)max_F * H, H, nsl, g.slab, acc_mod, stream);
    }
    const int cw = pick_cw(H, max_F);
    const int nch = stitch_chunks(B, H, cw);
    const int bper = (B + nch - 1) / nch;
    dim3 grid(H / cw, nch), block(cw);
    const int F = d_pos ? max_F : 0;                  // no position table: no LDS table, a chunk's partial is one row of H floats
    const size_t lds = (size_t)F * cw * sizeof(float);
#define STITCH_BWD(TT, POS) hipLaunchKernelGGL((stitch_bwd_kernel<TT, POS>), grid, block, lds, st, (const TT*)dx, (const TT*)dextra, ts, keep0, rec, drop, (TT*)d_tok, (float*)workspace, B, T, L, off, H, F, bper, keep_ld)
    if (dtype == MMFM_F32) { if (d_pos) STITCH_BWD(float, true); else STITCH_BWD(float, false); }
    else { if (d_pos) STITCH_BWD(uint16_t, true); else STITCH_BWD(uint16_t, false); }
#undef STITCH_BWD
    MMFM_LAUNCH_CHECK(what);
    const int64_t stride = (int64_t)(F + 1) * H;
    if (d_pos)
        if (int rc = mmfm_reduce_slabs(d_pos, (const float*)workspace, (int64_t)max_F * H, nch, stride, acc_pos, stream)) return rc;
    return mmfm_reduce_slabs(d_mod_row, (const float*)workspace + (size_t)F * H, H, nch, stride, acc_mod, stream);
}

extern "C" int mmfm_stitch_bwd(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0,
                               mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos, int B, int T,
                               int L, int m, int H, int max_F, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    return stitch_bwd_impl("mmfm_stitch_bwd", dtype, dx, dextra, ts, keep0, 0, nullptr, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, L,
                           (int64_t)m * T, H, max_F, workspace, workspace_bytes, stream);
}
extern "C" int mmfm_stitch_bwd_live(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0, const int32_t* rec,
                                    mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos, int B, int T,
                                    int L, int m, int H, int max_F, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    MMFM_REQUIRE(rec, "mmfm_stitch_bwd_live: null live-bin record");
    return stitch_bwd_impl("mmfm_stitch_bwd_live", dtype, dx, dextra, ts, keep0, 0, rec, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, L,
                           (int64_t)m * T, H, max_F, workspace, workspace_bytes, stream);
}
extern "C" int mmfm_stitch_bwd_seg(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep0, mmfm_dropout drop,
                                   void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos, int B, int T, int L, int off, int H,
                                   int max_F, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    return stitch_bwd_impl("mmfm_stitch_bwd_seg", dtype, dx, dextra, ts, keep0, 0, nullptr, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, L,
                           off, H, max_F, workspace, workspace_bytes, stream);
}
extern "C" int mmfm_stitch_bwd_rows(int dtype, const void* dx, const void* dextra, const int64_t* ts, const uint8_t* keep, int keep_ld,
                                    const int32_t* rec, mmfm_dropout drop, void* d_tok, float* d_mod_row, float* d_pos, int acc_mod, int acc_pos,
                                    int B, int T, int L, int off, int H, int max_F, void* workspace, int64_t workspace_bytes, mmfm_stream stream) {
    if (int rc = stitch_rows_args("mmfm_stitch_bwd_rows", dtype, keep, keep_ld, rec, T, L, off)) return rc;
    return stitch_bwd_impl("mmfm_stitch_bwd_rows", dtype, dx, dextra, ts, keep, keep_ld, rec, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, L,
                           off, H, max_F, workspace, workspace_bytes, stream);
}

// ---- live-bin records and the gather of live input rows (include/mmfm.h, "live rows")
namespace {
// one wave per modality slot: ballot + popcount prefix over 64 bins at a time
__global__ __launch_bounds__(64) void live_bins_kernel(const uint8_t* __restrict__ keep0, int T, int32_t* __restrict__ rec_all) {
    const uint8_t* k = keep0 + (size_t)blockIdx.x * T;
    int32_t* rec = rec_all + (size_t)blockIdx.x * MMFM_LIVE_REC_INTS(T);
    const int lane = threadIdx.x;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool live = t < T && k[t] != 0;
        const unsigned long long mask = __ballot(live);
        const int r = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (t < T) rec[4 + T + t] = live ? r : -1;
        if (live) rec[4 + r] = t;
        base += __popcll(mask);
    }
    if (lane < 4) rec[lane] = lane == 0 ? base : 0;
}

// V = uint4 / uint32_t pieces, cpr of them per row; the grid is sized for all B * T rows, the loop ends at the live ones
template <typename V>
__global__ __launch_bounds__(256) void gather_live_kernel(const V* __restrict__ src, V* __restrict__ dst, int B, int T, int cpr,
                                                          const int32_t* __restrict__ rec) {
    const int tl = rec[0];
    const int64_t total = (int64_t)B * tl * cpr;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cpr;
        const int c = (int)(idx - row * cpr), b = (int)(row / tl), j = (int)(row - (int64_t)b * tl);
        dst[idx] = src[((int64_t)b * T + rec[4 + j]) * cpr + c];
    }
}
}  // namespace

extern "C" int mmfm_live_bins(const uint8_t* keep0, int T, int M, int32_t* rec, mmfm_stream stream) {
    MMFM_REQUIRE(keep0 && rec && T > 0 && M > 0, "mmfm_live_bins: bad arguments");
    hipLaunchKernelGGL(live_bins_kernel, dim3(M), dim3(64), 0, (hipStream_t)stream, keep0, T, rec);
    MMFM_LAUNCH_CHECK("mmfm_live_bins");
    return 0;
}

extern "C" int mmfm_gather_live_rows(const void* src, void* dst, int B, int T, int64_t row_bytes, const int32_t* rec, mmfm_stream stream) {
    MMFM_REQUIRE(src && dst && rec && B > 0 && T > 0 && row_bytes > 0 && row_bytes % 4 == 0 && row_bytes < ((int64_t)1 << 30),
                 "mmfm_gather_live_rows: bad arguments (rows of a multiple of 4 bytes)");
    const bool v16 = row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const int cpr = (int)(row_bytes / (v16 ? 16 : 4));
    const int64_t n = (int64_t)B * T * cpr;
    dim3 grid((int)std::min<int64_t>(4096, (n + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (v16) hipLaunchKernelGGL(gather_live_kernel<uint4>, grid, block, 0, st, (const uint4*)src, (uint4*)dst, B, T, cpr, rec);
    else hipLaunchKernelGGL(gather_live_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)src, (uint32_t*)dst, B, T, cpr, rec);
    MMFM_LAUNCH_CHECK("mmfm_gather_live_rows");
    return 0;
}

// ---------------------------------------------------------------------------------- attention window: time stamps -> pos (MMFM_ATTN_WINDOW)
// pos[b][off_j + t] = clamp(ts_j[b][t]) for the slots of a stitched sequence; the slot table travels as a launch argument.
namespace {
struct PosSeg {
    const int64_t* ts[MAXM];
    int T[MAXM], off[MAXM];
    int M, L;
};
__global__ __launch_bounds__(256) void attn_pos_prep_kernel(const PosSeg s, int B, int32_t* __restrict__ pos) {
    constexpr int64_t LIM = (int64_t)1 << 29;
    const int64_t total = (int64_t)B * s.L;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx / s.L), i = (int)(idx - (int64_t)b * s.L);
        int j = 0;
#pragma unroll
        for (int m = 1; m < MAXM; ++m)
            if (m < s.M && i >= s.off[m]) j = m;
        const int64_t v = s.ts[j][(int64_t)b * s.T[j] + (i - s.off[j])];
        pos[idx] = (int32_t)(v < -LIM ? -LIM : v > LIM ? LIM : v);
    }
}
}  // namespace

extern "C" int mmfm_attn_pos_prep(int B, int M, const int32_t* seg_T, const int64_t* const* ts, int32_t* pos, mmfm_stream stream) {
    MMFM_REQUIRE(B > 0 && M > 0 && M <= MAXM, "mmfm_attn_pos_prep: bad shape B=%d M=%d (M <= %d)", B, M, MAXM);
    MMFM_REQUIRE(seg_T && ts && pos, "mmfm_attn_pos_prep: null pointer");
    PosSeg s{};
    int64_t L = 0;
    for (int j = 0; j < M; ++j) {
        MMFM_REQUIRE(seg_T[j] > 0 && ts[j], "mmfm_attn_pos_prep: slot %d: T=%d, ts %s", j, seg_T[j], ts[j] ? "set" : "null");
        s.ts[j] = ts[j]; s.T[j] = seg_T[j]; s.off[j] = (int)L;
        L += seg_T[j];
        MMFM_REQUIRE(L < ((int64_t)1 << 30), "mmfm_attn_pos_prep: sequence too long");
    }
    s.M = M; s.L = (int)L;
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(attn_pos_prep_kernel, dim3((int)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s, B, pos);
    MMFM_LAUNCH_CHECK("mmfm_attn_pos_prep");
    return 0;
}
