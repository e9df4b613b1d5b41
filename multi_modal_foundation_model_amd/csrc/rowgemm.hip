// mmfm_rowgemm / mmfm_prep_weights: row-owner GEMMs for the width-256 block linears (bf16 throughput mode).
//   y[R][N] = epi( pro(x)[R][K] . W[N][K]^T ),  K = 256, 512 or 768, token rows owned by wavefronts (rowchain.h).
// prologue : LayerNorm statistics + normalisation of the row in registers (K = 256; the affine part is folded into the
//            prepared weights), with x_hat / rstd side outputs for the backward
//            -> replaces nn.LayerNorm + the nn.Linear it feeds: ln1+qkv, query_norm+query, context_norm+key/value,
//               encoder_norm+decoder_proj_context (encoder_embeddings.py:110-112, decoder_embeddings.py:139-143, mm.py:290-292)
// epilogue : + bias, + residual, bf16 store  (attention out_proj + residual add, mm_utils.py:114 / encoder_embeddings.py:112)
//        or  LayerNorm BACKWARD on the full output row (N = 256) + residual gradient: the dX product of a linear that
//            was fed by a LayerNorm never writes d(x_hat) to memory (autograd of the sites above).
// activation rows are read once by these kernels: non-temporal line loads keep them from displacing the weights in L2
// (measured on the B = 1024 step: 7.83 -> 7.72 ms over the 72 launches; the MLP kernels re-read their rows and lose with it)
#define MMFM_ACT_LOAD_AUX 2
#include "rowchain.h"
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

using namespace rowchain;

namespace {

constexpr int NT = 256, NW = 4;

// ------------------------------------------------------------------------------------------------ forward-type kernel
constexpr int BIAS_MAX = 1024;                      // floats of bias kept in LDS behind the ring and the staging areas

// NWV waves per workgroup (8 = two per SIMD wherever the registers allow: the barrier / LDS-write overhead of a chunk is
// paid once per 256 rows instead of 128 and a SIMD's MFMA pipe is fed by two waves), 32 rows each
template <int KP, int LN, bool NTS, int NWV>
__global__ __launch_bounds__(NWV * 64, (KP == 1 ? 2 : 1)) void rowgemm_kernel(const mmfm_rowgemm_desc d) {
    constexpr int NT = NWV * 64, NW = NWV;
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES + NW * STG_BYTES + BIAS_MAX * 4];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    const int npair = d.N >> 6, cpp = 2 * npair * KP;                   // N % 64 == 0
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const uint16_t* W = reinterpret_cast<const uint16_t*>(d.w);
    const int ldw = d.ldw;
    // every workgroup walks the same weight tiles; each starts at a different tile pair
    const int rot = d.rotate ? (int)(blockIdx.x % npair) : 0;
    auto src = [=](int g) {
        const int idx = g % cpp, ti = idx / KP, p = idx - ti * KP;
        int pr = (ti >> 1) + rot; pr = pr >= npair ? pr - npair : pr;
        WChunk c;
        c.base = W + (size_t)(32 * (2 * pr + (ti & 1))) * ldw + 256 * p;
        c.ld = ldw; c.kind = 0;
        return c;
    };
    char* stg = smem + LDS_BYTES + wave * STG_BYTES;
    float* lbias = reinterpret_cast<float*>(smem + LDS_BYTES + NW * STG_BYTES);
    stage_vec(lbias, d.bias, d.N, t, NT);           // visible after the first chunk's barrier
    const GBuf X = gbuf(d.x, d.R * d.ldx * 2), Y = gbuf(d.y, d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.xhat, d.R * 512), RS = gbuf(d.rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    RING_DECL(NT);
    RING_START(smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32);
        const bool live = wrow0 < (uint32_t)d.R;          // wave-uniform: a wave without rows only keeps the ring's barriers
        opnd x[16 * KP];
        if (live) load_rows_lines<4 * KP>(stg, x, X, wrow0, ldxb, lane, m, h);
        if constexpr (LN != 0) if (live) {
            const float rs = norm_rows<LN>(x, d.eps);
            store_rows_lines<4, true>(stg, XH, wrow0, 512u, lane, m, h, x);
            st4f(RS, h == 0 ? (wrow0 + m) * 4u : 0xfffffff0u, rs);
        }
        for (int tp = 0; tp < npair; ++tp) {
            int pr = tp + rot; pr = pr >= npair ? pr - npair : pr;
            f32x16 acc[2];
            Lines res;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[j] = zero16();
#pragma unroll
                for (int p = 0; p < KP; ++p) {
                    RING_SYNC_WRITE(src);
                    if (j == 0 && p == 0) res = fetch_lines(RES, wrow0, ldrb, 128u * pr, lane);   // older than the chunk fetch
                    const char* slot;
                    RING_FETCH(src, slot);
                    if (live) acc[j] = mma16(slot, x + 16 * p, acc[j], m, h);
                }
                add_vec(acc[j], lbias, 2 * pr + j, h);
            }
            if (!live) continue;
            stage_lines(stg, res, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[j][i] += r[i];
            }
            stage_tile(stg, 0, m, h, acc[0]);
            stage_tile(stg, 1, m, h, acc[1]);
            flush_lines<NTS>(stg, Y, wrow0, ldyb, 128u * pr, lane);
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward-type kernel, asynchronous ring
// K = 256 (every forward-type launch of the step).  Same row ownership and epilogue as rowgemm_kernel; the weights come through the
// three-slot LDS-DMA ring of rowchain.h (chunk cc+2 requested - one request behind each MFMA group - while chunk cc is multiplied; no
// staging registers, no ds_write pass; the move that took the MLP forward from 251 to 213 us).  A vector-memory LOAD inside the ring
// loop would be waited for with a compiler-counted vmcnt that does not know the DMA requests, i.e. it would drain the prefetch: the
// residual lines of the whole pass are therefore requested in front of the loop (RES4: N = 256, the only residual site), and the only
// other traffic of the loop, the four line stores behind each tile pair, is accounted for in the ring's wait (EXTRA, below).
// NPV = N / 64 when known at compile time (4: unrolled, residual allowed), 0 = runtime.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int LN, bool NTS, int NPV>
__global__ __launch_bounds__(256, 2) void rowgemm_a_kernel(const mmfm_rowgemm_desc d) {
    constexpr int NT = 256, NW = 4, RING_B = RINGA_SLOTS * CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // RING_B + NW * STG_BYTES + BIAS_MAX * 4
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    // Column blocks (gridDim.y > 1: launches with fewer row passes than CUs - the reference's batch of 16 is 25 passes - where one workgroup
    // walking all of N is a chain of 2 N / 64 dependent ring steps; split, every workgroup re-reads its 128 rows and takes `npair` tile pairs
    // starting at `pbase`).  The LayerNorm side outputs are written by column block 0 only.
    const int np_all = d.N >> 6;                                                    // N % 64 == 0
    const int npb = NPV ? NPV : (np_all + (int)gridDim.y - 1) / (int)gridDim.y, pbase = (int)blockIdx.y * npb;
    const int npair = NPV ? NPV : min(npb, np_all - pbase), cpp = 2 * npair;
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0 || npair <= 0) return;
    const __amdgpu_buffer_rsrc_t rs_w = wbuf(d.w);
    const uint32_t ldwb = (uint32_t)d.ldw * 2u;
    const int rot = d.rotate ? (int)(blockIdx.x % npair) : 0;
    auto src = [=](int g) {
        const int ti = g % cpp;
        int pr = (ti >> 1) + rot; pr = pbase + (pr >= npair ? pr - npair : pr);
        AChunk c;
        c.rs = rs_w; c.off = (uint32_t)(32 * (2 * pr + (ti & 1))) * ldwb; c.ldb = ldwb; c.kind = 0;
        return c;
    };
    char* stg = smem + RING_B + wave * STG_BYTES;
    float* lbias = reinterpret_cast<float*>(smem + RING_B + NW * STG_BYTES);
    stage_vec(lbias, d.bias, d.N, t, NT);           // visible after the first chunk's barrier
    const GBuf X = gbuf(d.x, d.R * d.ldx * 2), Y = gbuf(d.y, d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(blockIdx.y == 0 ? d.xhat : nullptr, d.R * 512), RS = gbuf(blockIdx.y == 0 ? d.rstd : nullptr, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    const bool has_res = NPV != 0 && d.residual != nullptr;
    const ALane<NT> ring_al = alane_init<NT>(t, ldwb, 0u);
    const AFrag fr = afrag_init(m, h);
    RINGA_DECL(NT);
    RINGA_START((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32);
        const bool live = wrow0 < (uint32_t)d.R;          // wave-uniform: a wave without rows only keeps the ring turning
        opnd x[16];
        Lines res[NPV ? NPV : 1];
        if (live) {
            load_rows_lines<4>(stg, x, X, wrow0, ldxb, lane, m, h);
            if constexpr (LN != 0) {
                const float rs = norm_rows<LN>(x, d.eps);
                store_rows_lines<4, true>(stg, XH, wrow0, 512u, lane, m, h, x);
                st4f(RS, h == 0 ? (wrow0 + m) * 4u : 0xfffffff0u, rs);
            }
            if constexpr (NPV != 0) if (has_res) {          // behind the LayerNorm: its fp32 row and these 64 registers do not fit together
#pragma unroll
                for (int tp = 0; tp < NPV; ++tp) {
                    int pr = tp + rot; pr = pbase + (pr >= npair ? pr - npair : pr);
                    res[tp] = fetch_lines(RES, wrow0, ldrb, 128u * pr, lane);
                }
            }
        }
        // One tile pair = two ring steps + four line stores.  The stores of pair tp-1 were issued behind the requests of chunks 2tp and
        // 2tp+1, so both steps of pair tp may leave them in flight (EXTRA = 4; a wave without rows has issued none: 0); the first pair
        // of a pass waits conservatively (its predecessors are the prologue's loads / stores, of which there may be none).
        auto pair = [&](int tp, auto first) {
            constexpr int EX = decltype(first)::value ? 0 : 4;
            int pr = tp + rot; pr = pbase + (pr >= npair ? pr - npair : pr);
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint32_t slot;
                if (live) vm_wait_n<1024 / NT + EX>(); else vm_wait_n<1024 / NT>();
                RINGA_SYNC_NOWAIT(src, slot);
                if (live) {
                    acc[j] = mma16a<4>(slot, fr, x, zero16(), [&](int g_) { RINGA_PIECE(g_); });
                    add_vec(acc[j], lbias, 2 * pr + j, h);
                } else {
#pragma unroll
                    for (int q = 0; q < 1024 / NT; ++q) RINGA_PIECE(q);
                }
            }
            if (!live) return;
            if constexpr (NPV != 0) if (has_res) {
                stage_lines(stg, res[NPV ? tp : 0], lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[j][i] += r[i];
                }
            }
            stage_tile(stg, 0, m, h, acc[0]);
            stage_tile(stg, 1, m, h, acc[1]);
            flush_lines<NTS>(stg, Y, wrow0, ldyb, 128u * pr, lane);
        };
        pair(0, std::true_type());
        if constexpr (NPV != 0) {
#pragma unroll
            for (int tp = 1; tp < NPV; ++tp) pair(tp, std::false_type());
        } else {
            for (int tp = 1; tp < npair; ++tp) pair(tp, std::false_type());
        }
    }
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------------ dX + LayerNorm backward
// v = x . W^T (N = 256: the gradient wrt x_hat of the LayerNorm that fed the forward linear; W = prepared W'^T);
// y = dres + rstd * (v - mean(v) - x_hat * mean(v * x_hat))
template <int KP, int NORM>
__global__ __launch_bounds__(NT) void rowgemm_lnbwd_kernel(const mmfm_rowgemm_desc d) {
    // + a 16 KB per-wave stash of the pass's x_hat rows (as in the MLP backward): the statistics loop fetches them once, the output
    // loop reads them from LDS instead of putting a second dependent round trip per line pair into every pass
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES + NW * STG_BYTES + NW * 4 * STG_BYTES];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    constexpr int cpp = 8 * KP;
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const uint16_t* W = reinterpret_cast<const uint16_t*>(d.w);
    const int ldw = d.ldw;
    auto src = [=](int g) {
        const int idx = g % cpp, tt = idx / KP, p = idx - tt * KP;
        WChunk c;
        c.base = W + (size_t)(32 * tt) * ldw + 256 * p;
        c.ld = ldw; c.kind = 0;
        return c;
    };
    char* stg = smem + LDS_BYTES + wave * STG_BYTES;
    char* xstash = smem + LDS_BYTES + NW * STG_BYTES + wave * 4 * STG_BYTES;
    const GBuf X = gbuf(d.x, d.R * d.ldx * 2), Y = gbuf(d.y, d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.bwd_xhat, d.R * 512), RS = gbuf(d.bwd_rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    RING_DECL(NT);
    RING_START(smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32);
        opnd x[16 * KP];
        load_rows_lines<4 * KP>(stg, x, X, wrow0, ldxb, lane, m, h);
        float rs = ld4f(RS, (wrow0 + m) * 4u);
        f32x16 acc[8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            Lines xl;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[2 * tp + j] = zero16();
#pragma unroll
                for (int p = 0; p < KP; ++p) {
                    RING_SYNC_WRITE(src);
                    if (j == 0 && p == 0) xl = fetch_lines(XH, wrow0, 512u, 128u * tp, lane);
                    const char* slot;
                    RING_FETCH(src, slot);
                    acc[2 * tp + j] = mma16(slot, x + 16 * p, acc[2 * tp + j], m, h);
                }
            }
            stage_lines(xstash + tp * STG_BYTES, xl, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += acc[2 * tp + j][i]; s2 = fmaf(acc[2 * tp + j][i], xt[i], s2); }
            }
        }
        s1 = xhalf(s1);
        s2 = xhalf(s2);
        norm_bwd_stats<NORM>(s1, s2, rs);
        Lines rl4[4];                                   // the residual-gradient lines, requested together (the operand registers are dead here)
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) rl4[tp] = fetch_lines(RES, wrow0, ldrb, 128u * tp, lane);
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            const Lines& rl = rl4[tp];
            f32x16 o[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] = rs * (acc[2 * tp + j][i] - s1 - xt[i] * s2);
            }
            stage_lines(stg, rl, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] += r[i];
            }
            stage_tile(stg, 0, m, h, o[0]);
            stage_tile(stg, 1, m, h, o[1]);
            flush_lines<false>(stg, Y, wrow0, ldyb, 128u * tp, lane);
        }
    }
}

// ------------------------------------------------------------------------------------------------ dX + LayerNorm backward, asynchronous ring
// The one-wave-per-tile kernel above with the weights on the three-slot LDS-DMA ring.  The x_hat lines of the pass are fetched and
// stashed in front of the ring loop (a load inside it would be waited for with a vmcnt that does not know the DMA requests and drain
// the prefetch), so the loop issues nothing but ring requests and MFMAs.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int KP, int NORM>
__global__ __launch_bounds__(NT) void rowgemm_lnbwd_a_kernel(const mmfm_rowgemm_desc d) {
    constexpr int RING_B = RINGA_SLOTS * CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // RING_B + NW * STG_BYTES + NW * 4 * STG_BYTES
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    constexpr int cpp = 8 * KP;
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const __amdgpu_buffer_rsrc_t rs_w = wbuf(d.w);
    const uint32_t ldwb = (uint32_t)d.ldw * 2u;
    auto src = [=](int g) {
        const int idx = g % cpp, tt = idx / KP, p = idx - tt * KP;
        AChunk c;
        c.rs = rs_w; c.off = (uint32_t)(32 * tt) * ldwb + 512u * (uint32_t)p; c.ldb = ldwb; c.kind = 0;
        return c;
    };
    char* stg = smem + RING_B + wave * STG_BYTES;
    char* xstash = smem + RING_B + NW * STG_BYTES + wave * 4 * STG_BYTES;
    const GBuf X = gbuf(d.x, d.R * d.ldx * 2), Y = gbuf(d.y, d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.bwd_xhat, d.R * 512), RS = gbuf(d.bwd_rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    const ALane<NT> ring_al = alane_init<NT>(t, ldwb, 0u);
    const AFrag fr = afrag_init(m, h);
    RINGA_DECL(NT);
    RINGA_START((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32);
        opnd x[16 * KP];
        {
            Lines xl[4];
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) xl[tp] = fetch_lines(XH, wrow0, 512u, 128u * tp, lane);
            load_rows_lines<4 * KP>(stg, x, X, wrow0, ldxb, lane, m, h);
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) stage_lines(xstash + tp * STG_BYTES, xl[tp], lane);
        }
        float rs = ld4f(RS, (wrow0 + m) * 4u);
        f32x16 acc[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            acc[tt] = zero16();
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                uint32_t slot;
                RINGA_SYNC(src, slot, 0);
                acc[tt] = mma16a<4>(slot, fr, x + 16 * p, acc[tt], [&](int g_) { RINGA_PIECE(g_); });
            }
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += acc[2 * tp + j][i]; s2 = fmaf(acc[2 * tp + j][i], xt[i], s2); }
            }
        }
        s1 = xhalf(s1);
        s2 = xhalf(s2);
        norm_bwd_stats<NORM>(s1, s2, rs);
        Lines rl4[4];                                   // the residual-gradient lines, requested together (the operand registers are dead here)
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) rl4[tp] = fetch_lines(RES, wrow0, ldrb, 128u * tp, lane);
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            const Lines& rl = rl4[tp];
            f32x16 o[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] = rs * (acc[2 * tp + j][i] - s1 - xt[i] * s2);
            }
            stage_lines(stg, rl, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] += r[i];
            }
            stage_tile(stg, 0, m, h, o[0]);
            stage_tile(stg, 1, m, h, o[1]);
            flush_lines<false>(stg, Y, wrow0, ldyb, 128u * tp, lane);
        }
    }
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------------ dX + LayerNorm backward, wave pairs
// Eight waves; waves w and w+4 own the SAME 32 rows and split the 256 output columns (tiles 0-3 / 4-7): 64 accumulator
// registers each instead of 128, the K = 256*KP input streamed one 256-wide piece at a time (64 registers + the next piece in
// flight) -> two waves per SIMD fit where the one-wave version needed 512 registers and spent its time copying operands out
// of the accumulator file.  A 32 KB chunk = the two groups' weight tiles of one (piece, tile) step; the row statistics of the
// LayerNorm backward are summed across the pair through LDS behind one extra barrier per pass.
template <int KP, int NORM>
__global__ __launch_bounds__(512) void rowgemm_lnbwd8_kernel(const mmfm_rowgemm_desc d) {
    constexpr int NT = 512, NW = 8, NPAIR = 4;
    __shared__ __attribute__((aligned(16))) char smem[2 * CHUNK2 + NW * STG_BYTES + NW * 32 * 8];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    const int half = wave >> 2, pw = wave & 3;
    constexpr int cpp = 4 * KP;
    const int64_t npass = (d.R + 32 * NPAIR - 1) / (32 * NPAIR);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const uint16_t* W = reinterpret_cast<const uint16_t*>(d.w);
    const int ldw = d.ldw;
    auto src = [=](int g) {
        const int idx = g % cpp, p = idx >> 2, j = idx & 3;
        WChunk2 c;
        c.s[0].base = W + (size_t)(32 * j) * ldw + 256 * p; c.s[0].ld = ldw; c.s[0].kind = 0;
        c.s[1].base = W + (size_t)(32 * (4 + j)) * ldw + 256 * p; c.s[1].ld = ldw; c.s[1].kind = 0;
        return c;
    };
    char* stg = smem + 2 * CHUNK2 + wave * STG_BYTES;
    float2* exch = reinterpret_cast<float2*>(smem + 2 * CHUNK2 + NW * STG_BYTES);      // [wave][32 rows]
    const GBuf X = gbuf(d.x, d.R * d.ldx * 2), Y = gbuf(d.y, d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.bwd_xhat, d.R * 512), RS = gbuf(d.bwd_rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    RING2_DECL(NT);
    RING2_START(smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NPAIR + pw) * 32);
        const bool live = wrow0 < (uint32_t)d.R;
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = zero16();
        Lines L[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) L[q] = fetch_lines(X, wrow0, ldxb, 128u * q, lane);
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            opnd x[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                stage_lines(stg, L[q], lane);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) x[4 * q + s4] = unstage_opnd(stg, s4, m, h);
                if (p + 1 < KP) L[q] = fetch_lines(X, wrow0, ldxb, 512u * (p + 1) + 128u * q, lane);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const char* slot;
                RING2_STEP(src, slot);
                if (live) acc[j] = mma16<4>(slot + half * CHUNK, x, acc[j], m, h);
            }
        }
        // this wave's columns: tiles 4*half .. 4*half+3 = line pairs 2*half, 2*half+1
        f32x16 xt[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const Lines xl = fetch_lines(XH, wrow0, 512u, 128u * (2 * half + q), lane);
            stage_lines(stg, xl, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                xt[2 * q + j] = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += acc[2 * q + j][i]; s2 = fmaf(acc[2 * q + j][i], xt[2 * q + j][i], s2); }
            }
        }
        s1 = xhalf(s1); s2 = xhalf(s2);
        if (h == 0) exch[wave * 32 + m] = make_float2(s1, s2);
        __syncthreads();
        const float2 o2 = exch[(wave ^ 4) * 32 + m];
        s1 = s1 + o2.x;
        s2 = s2 + o2.y;
        float rs = ld4f(RS, (wrow0 + m) * 4u);
        norm_bwd_stats<NORM>(s1, s2, rs);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const Lines rl = fetch_lines(RES, wrow0, ldrb, 128u * (2 * half + q), lane);
            stage_lines(stg, rl, lane);
            f32x16 o[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] = r[i] + rs * (acc[2 * q + j][i] - s1 - xt[2 * q + j][i] * s2);
            }
            stage_tile(stg, 0, m, h, o[0]);
            stage_tile(stg, 1, m, h, o[1]);
            flush_lines<false>(stg, Y, wrow0, ldyb, 128u * (2 * half + q), lane);
        }
    }
}

// ------------------------------------------------------------------------------------------------ grouped launches (mmfm_rowgemm_groups)
// Up to 8 weight sets against the same rows.  The weights of all groups go through ONE buffer resource (`wbase` + a 32-bit byte offset
// per group, host-checked); outputs / operands get one bounds-checked resource per group.  The per-group values are picked out of the
// kernel arguments by a chain of scalar selects.
constexpr int GROUPS_MAX = MMFM_ROWGEMM_MAX_GROUPS;
constexpr int GBIAS_MAX = 2560;                     // floats: the biases of all groups stay in LDS (74 KB per workgroup, two per CU)
struct GroupOff { uint32_t w[GROUPS_MAX]; };
template <typename T>
__device__ __forceinline__ T pick8(const T (&a)[GROUPS_MAX], int g) {
    T r = a[0];
#pragma unroll
    for (int i = 1; i < GROUPS_MAX; ++i) r = g == i ? a[i] : r;
    return r;
}

// Grouped forward: rowgemm_a_kernel<LN, NTS, 0> whose tile-pair loop walks the groups * N / 64 pairs of all groups (virtual pair vp:
// group vp >> nps, pair vp & (N / 64 - 1)); the norm prologue and its side outputs run once per row pass.  Every output element sees
// the statistics and the K = 256 product of the per-group launch, in the same order.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int LN, bool NTS>
__global__ __launch_bounds__(256, 2) void rowgemm_groups_a_kernel(const mmfm_rowgemm_groups_desc d, const void* wbase, const GroupOff wo, int nps) {
    constexpr int NT = 256, NW = 4, RING_B = RINGA_SLOTS * CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // RING_B + NW * STG_BYTES + GBIAS_MAX * 4
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    // column blocks over the virtual pairs, as in rowgemm_a_kernel; the norm's side outputs are written by column block 0 only
    const int np_g = d.N >> 6, np_all = np_g * d.groups;
    const int npb = (np_all + (int)gridDim.y - 1) / (int)gridDim.y, pbase = (int)blockIdx.y * npb;
    const int npair = min(npb, np_all - pbase), cpp = 2 * npair;
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0 || npair <= 0) return;
    const __amdgpu_buffer_rsrc_t rs_w = wbuf(wbase);
    const uint32_t ldwb = (uint32_t)d.ldw * 2u;
    const int rot = d.rotate ? (int)(blockIdx.x % npair) : 0;
    auto src = [&](int g) {
        const int ti = g % cpp;
        int vp = (ti >> 1) + rot; vp = pbase + (vp >= npair ? vp - npair : vp);
        const int pr = vp & (np_g - 1);
        AChunk c;
        c.rs = rs_w; c.off = __builtin_amdgcn_readfirstlane(pick8(wo.w, vp >> nps) + (uint32_t)(32 * (2 * pr + (ti & 1))) * ldwb); c.ldb = ldwb; c.kind = 0;
        return c;
    };
    char* stg = smem + RING_B + wave * STG_BYTES;
    float* lbias = reinterpret_cast<float*>(smem + RING_B + NW * STG_BYTES);
    for (int g = 0; g < d.groups; ++g) stage_vec(lbias + g * d.N, pick8(d.bias, g), d.N, t, NT);      // visible after the first chunk's barrier
    const GBuf X = gbuf(d.x[0], d.R * d.ldx * 2);
    const GBuf XH = gbuf(blockIdx.y == 0 ? d.xhat : nullptr, d.R * 512), RS = gbuf(blockIdx.y == 0 ? d.rstd : nullptr, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2;
    const ALane<NT> ring_al = alane_init<NT>(t, ldwb, 0u);
    const AFrag fr = afrag_init(m, h);
    RINGA_DECL(NT);
    RINGA_START((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem, my_passes * cpp, src);
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32);
        const bool live = wrow0 < (uint32_t)d.R;          // wave-uniform: a wave without rows only keeps the ring turning
        opnd x[16];
        if (live) {
            load_rows_lines<4>(stg, x, X, wrow0, ldxb, lane, m, h);
            const float rs = norm_rows<LN>(x, d.eps);
            store_rows_lines<4, true>(stg, XH, wrow0, 512u, lane, m, h, x);
            st4f(RS, h == 0 ? (wrow0 + m) * 4u : 0xfffffff0u, rs);
        }
        // one tile pair = two ring steps + four line stores: the accounting of rowgemm_a_kernel (EXTRA = 4 behind the pass's first pair)
        auto pair = [&](int tp, auto first) {
            constexpr int EX = decltype(first)::value ? 0 : 4;
            int vp = tp + rot; vp = pbase + (vp >= npair ? vp - npair : vp);
            const int grp = vp >> nps, pr = vp & (np_g - 1);
            const GBuf Y = gbuf(pick8(d.y, grp), d.R * d.ldy * 2);
            const float* gb = lbias + grp * d.N;
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint32_t slot;
                if (live) vm_wait_n<1024 / NT + EX>(); else vm_wait_n<1024 / NT>();
                RINGA_SYNC_NOWAIT(src, slot);
                if (live) {
                    acc[j] = mma16a<4>(slot, fr, x, zero16(), [&](int g_) { RINGA_PIECE(g_); });
                    add_vec(acc[j], gb, 2 * pr + j, h);
                } else {
#pragma unroll
                    for (int q = 0; q < 1024 / NT; ++q) RINGA_PIECE(q);
                }
            }
            if (!live) return;
            stage_tile(stg, 0, m, h, acc[0]);
            stage_tile(stg, 1, m, h, acc[1]);
            flush_lines<NTS>(stg, Y, wrow0, ldyb, 128u * pr, lane);
        };
        pair(0, std::true_type());
        for (int tp = 1; tp < npair; ++tp) pair(tp, std::false_type());
    }
}

// Grouped dX + norm backward: acc[32 rows x 256] = sum over the groups * KP pieces (256 of K each) of x_piece . WpT_piece, then the
// epilogue of rowgemm_lnbwd_a_kernel.  The operand is STREAMED: one piece (16 operands, 64 registers) is multiplied against the eight
// persistent accumulator tiles (eight ring steps) while the lines of the next piece - the next pass's first piece behind a pass's last,
// so every piece issues the same 16 loads - are in flight.  Vector-memory operations retire in order, hence the waits of a piece's steps:
//   the lines are requested in front of step 0, behind the requests of chunks c and c+1: steps 0 and 1 may leave them in flight (EXTRA = 16);
//   step 2 waits for chunk c+2, requested behind the lines: they have landed, and are moved into operand layout in front of that step,
//   where the compiler's own (conservative) wait for them costs nothing the ring's wait would not.
// (Requesting a whole K = 512 group's lines at once - one exposed round trip per 16 steps instead of 8 - measured the same 406 us at
// R = 204,800 with five groups and needs 512 registers + 44 bytes of scratch: not kept.)
// The weight ring's source is a counter pair (piece, tile) advanced once per request: no division by the runtime piece count.
template <int KP, int NORM>
__global__ __launch_bounds__(NT) void rowgemm_groups_lnbwd_kernel(const mmfm_rowgemm_groups_desc d, const void* wbase, const GroupOff wo) {
    constexpr int RING_B = RINGA_SLOTS * CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // RING_B + NW * STG_BYTES + NW * 4 * STG_BYTES
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    const int npiece = d.groups * KP;
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const __amdgpu_buffer_rsrc_t rs_w = wbuf(wbase);
    const uint32_t ldwb = (uint32_t)d.ldw * 2u;
    int src_q = 0, src_t = 0;                           // the next chunk to request: piece, tile
    auto src = [&](int) {
        const int g = KP == 1 ? src_q : src_q >> 1, p = KP == 1 ? 0 : src_q & 1;
        AChunk c;
        c.rs = rs_w; c.off = __builtin_amdgcn_readfirstlane(pick8(wo.w, g) + (uint32_t)(32 * src_t) * ldwb + 512u * (uint32_t)p); c.ldb = ldwb; c.kind = 0;
        if (++src_t == 8) { src_t = 0; if (++src_q == npiece) src_q = 0; }
        return c;
    };
    char* stg = smem + RING_B + wave * STG_BYTES;
    char* xstash = smem + RING_B + NW * STG_BYTES + wave * 4 * STG_BYTES;
    const GBuf Y = gbuf(d.y[0], d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.bwd_xhat, d.R * 512), RS = gbuf(d.bwd_rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    const int64_t xbytes = d.R * d.ldx * 2;
    const ALane<NT> ring_al = alane_init<NT>(t, ldwb, 0u);
    const AFrag fr = afrag_init(m, h);
    RINGA_DECL(NT);
    RINGA_START((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem, my_passes * 8 * npiece, src);
    auto row_of = [&](int pi) { return (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32); };
    opnd x[16];
    load_rows_lines<4>(stg, x, gbuf(d.x[0], xbytes), row_of(0), ldxb, lane, m, h);      // piece 0 of the first pass
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = row_of(pi);
        // rows the next pass's first piece comes from; behind the last pass: beyond the tensor (the bounds check returns zeros)
        const uint32_t nrow0 = pi + 1 < my_passes ? row_of(pi + 1) : (uint32_t)(npass * 32 * NW);
        {
            Lines xl[4];
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) xl[tp] = fetch_lines(XH, wrow0, 512u, 128u * tp, lane);
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) stage_lines(xstash + tp * STG_BYTES, xl[tp], lane);
        }
        float rs = ld4f(RS, (wrow0 + m) * 4u);
        f32x16 acc[8];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) acc[tt] = zero16();
        for (int q = 0; q < npiece; ++q) {
            const int nq = q + 1 < npiece ? q + 1 : 0;
            const uint32_t nrow = q + 1 < npiece ? wrow0 : nrow0;
            const GBuf XN = gbuf(pick8(d.x, KP == 1 ? nq : nq >> 1), xbytes);
            const uint32_t ncol = KP == 1 ? 0u : 512u * (uint32_t)(nq & 1);
            Lines L[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) L[s] = fetch_lines(XN, nrow, ldxb, ncol + 128u * s, lane);
            opnd xn[16];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) {
                if (tt == 2) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        stage_lines(stg, L[s], lane);
#pragma unroll
                        for (int s4 = 0; s4 < 4; ++s4) xn[4 * s + s4] = unstage_opnd(stg, s4, m, h);
                    }
                }
                uint32_t slot;
                if (tt < 2) { RINGA_SYNC(src, slot, 16); acc[tt] = mma16a<4>(slot, fr, x, acc[tt], [&](int g_) { RINGA_PIECE(g_); }); }
                else { RINGA_SYNC(src, slot, 0); acc[tt] = mma16a<4>(slot, fr, x, acc[tt], [&](int g_) { RINGA_PIECE(g_); }); }
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) x[s] = xn[s];
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += acc[2 * tp + j][i]; s2 = fmaf(acc[2 * tp + j][i], xt[i], s2); }
            }
        }
        s1 = xhalf(s1);
        s2 = xhalf(s2);
        norm_bwd_stats<NORM>(s1, s2, rs);
        Lines rl4[4];                                   // the residual-gradient lines, requested together
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) rl4[tp] = fetch_lines(RES, wrow0, ldrb, 128u * tp, lane);
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            const Lines& rl = rl4[tp];
            f32x16 o[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(xstash + tp * STG_BYTES, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] = rs * (acc[2 * tp + j][i] - s1 - xt[i] * s2);
            }
            stage_lines(stg, rl, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 r = unstage_tile(stg, j, m, h);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] += r[i];
            }
            stage_tile(stg, 0, m, h, o[0]);
            stage_tile(stg, 1, m, h, o[1]);
            flush_lines<false>(stg, Y, wrow0, ldyb, 128u * tp, lane);
        }
    }
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------------ dX + norm backward, two workgroups per CU
// The product and epilogue of rowgemm_lnbwd_a_kernel / rowgemm_groups_lnbwd_kernel (K = 512 / 768, one or several groups) in a form of which
// two workgroups fit one CU: 256 registers per wave, 64 KB of LDS per workgroup.  What had to shrink, and how:
//   operand registers   the K-deep operand rows (128 / 192 registers, or 64 + the next piece's 64 in the grouped kernel) are never held.  The
//                       weights come as kind-2 chunks, [256 outputs][32 k]: one ring step multiplies ONE 32-deep k slice against all eight
//                       accumulator tiles, so a step needs two operands (8 registers) and the rows stream past in 64-wide blocks (one block =
//                       one `Lines` = 16 registers = two ring steps), one block in flight (a second one would not be waited for any later:
//                       vector-memory operations retire in order, and the ring's wait for the chunk requested behind a block covers the
//                       block).  Per accumulator element the MFMA sequence is k-step 0, 1, 2, ... of group 0, then group 1, ...: the order
//                       of the kernels above, so the results are bit-identical.
//   LDS                 no x_hat stash (64 KB per workgroup: with it not even a two-slot ring fits beside a second workgroup).  The x_hat lines
//                       are requested BEHIND the ring loop, once for the statistics and once more (out of L2) for the output; holding them
//                       as 64 registers of raw tiles beside the 128 accumulator registers spilled.  The round trips this exposes once per
//                       pass are what the other workgroup covers.
// The ring loop issues no compiler-visible vector-memory operation: the operand blocks are requested by inline asm like the ring's DMA and
// waited for by count.  Steady state, block b (ring steps 2b, 2b+1):
//   issue order     ... L(b) C(2b) C(2b+1) | L(b+1) C(2b+2) C(2b+3) | ...      L = 4 loads, C = 4 DMA requests per lane
//   front of b      L(b) must have landed: the 8 younger requests may stay in flight; the block is staged, then L(b+1) is requested
//   steps 2b, 2b+1  chunk C(s) must have landed: C(s+1) and L(b+1) may stay in flight (EXTRA = 4)
// A pass's last block requests nothing (EXTRA = 0); the next pass's first block is requested in the epilogue, behind the second of the four
// line-pair stores, where half the accumulators are dead: eight loads and eight stores follow it, so the same wait holds.  Anything else
// issued in between is younger than what a wait is for and only makes it conservative.  Behind the last pass the block comes from rows
// beyond the tensor, which the bounds check answers with zeros without touching memory.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void fetch_lines_async(Lines& L, const GBuf& b, uint32_t wrow0, uint32_t ldb, uint32_t colb, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t off = (wrow0 + 8 * i + (lane >> 3)) * ldb + colb + 16 * (lane & 7);
        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "=v"(L.v[i]) : "v"(off), "s"(b.rs) : "memory");
    }
}
// The wait for such a block is a separate statement (vm_wait_n): it pins the ORDER of request, wait and use, not the register allocation.
// hipcc sees the load's result as ready at once, so a register copy of the block between request and wait would copy what has not landed
// (naming the destinations as in-out operands of the wait does not compile: hipcc rejects tied 128-bit operands of this type).  There is
// no such copy in this build: no v_mov / scratch access of the destinations on any path of either instantiation in the --save-temps
// assembly.  Repeat that reading whenever hipcc or this kernel changes; the bit-identity test against the one-workgroup kernels
// (tests/test_rowgemm_lnbwd_two_wg_gpu.py) fails on a block used before it landed.
template <int NORM>
__global__ __launch_bounds__(256, 2) void rowgemm_lnbwd2_kernel(const mmfm_rowgemm_groups_desc d, const void* wbase, const GroupOff wo) {
    constexpr int NT = 256, NW = 4, RING_B = RINGA_SLOTS * CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];       // RING_B + NW * STG_BYTES
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), m = lane & 31, h = lane >> 5;
    const int kb = d.K >> 6, kc = 2 * kb, nblk = d.groups * kb;       // 64-wide operand blocks / 32-deep chunks per group; blocks per pass
    const int64_t npass = (d.R + 32 * NW - 1) / (32 * NW);
    const int my_passes = blockIdx.x < npass ? (int)((npass - 1 - blockIdx.x) / gridDim.x) + 1 : 0;
    if (my_passes == 0) return;
    const __amdgpu_buffer_rsrc_t rs_w = wbuf(wbase);
    const uint32_t ldwb = (uint32_t)d.ldw * 2u;
    int src_g = 0, src_c = 0;                           // the next chunk to request: group, k slice
    auto src = [&](int) {
        AChunk c;
        c.rs = rs_w; c.off = __builtin_amdgcn_readfirstlane(pick8(wo.w, src_g) + 64u * (uint32_t)src_c); c.ldb = ldwb; c.kind = 2;
        if (++src_c == kc) { src_c = 0; if (++src_g == d.groups) src_g = 0; }
        return c;
    };
    char* stg = smem + RING_B + wave * STG_BYTES;
    const GBuf Y = gbuf(d.y[0], d.R * d.ldy * 2), RES = gbuf(d.residual, d.R * d.ldr * 2);
    const GBuf XH = gbuf(d.bwd_xhat, d.R * 512), RS = gbuf(d.bwd_rstd, d.R * 4);
    const uint32_t ldxb = d.ldx * 2, ldyb = d.ldy * 2, ldrb = d.ldr * 2;
    const int64_t xbytes = d.R * d.ldx * 2;
    auto row_of = [&](int pi) { return (uint32_t)(((int64_t)(blockIdx.x + (int64_t)pi * gridDim.x) * NW + wave) * 32); };
    int xs_g = 0, xs_c = 0, xs_pi = 0;                  // the next operand block to request: group, block in group, pass
    auto xfetch = [&](Lines& L) {
        const uint32_t row0 = xs_pi < my_passes ? row_of(xs_pi) : (uint32_t)(npass * 32 * NW);
        fetch_lines_async(L, gbuf(pick8(d.x, xs_g), xbytes), row0, ldxb, 128u * (uint32_t)xs_c, lane);
        if (++xs_c == kb) { xs_c = 0; if (++xs_g == d.groups) { xs_g = 0; ++xs_pi; } }
    };
    const ALane<NT> ring_al = alane_init<NT>(t, 0u, ldwb);
    const AFrag fr = afrag_init(m, h);
    RINGA_DECL(NT);
    Lines L0;
    xfetch(L0);
    RINGA_START((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem, my_passes * nblk * 2, src);
    f32x16 acc[8];
    // one ring step: the 32-deep slice against the eight tiles, weight operands in two sets of four (tile pair x 2 k-steps), ping-pong,
    // counted waits, one ring request behind each MFMA group (mlp_fused.hip's d(x_hat) product)
#define L2_READS(SET, Q) do { ALDS_READ_B(wv[SET][0], slot, fr, 2 * (Q), 0); ALDS_READ_B(wv[SET][1], slot, fr, 2 * (Q), 1);          \
                              ALDS_READ_B(wv[SET][2], slot, fr, 2 * (Q) + 1, 0); ALDS_READ_B(wv[SET][3], slot, fr, 2 * (Q) + 1, 1); } while (0)
#define L2_MMAS(SET, Q, X0, X1) do { acc[2 * (Q)] = mfma_u4(wv[SET][0], X0, acc[2 * (Q)]); acc[2 * (Q) + 1] = mfma_u4(wv[SET][2], X0, acc[2 * (Q) + 1]); \
                                     acc[2 * (Q)] = mfma_u4(wv[SET][1], X1, acc[2 * (Q)]); acc[2 * (Q) + 1] = mfma_u4(wv[SET][3], X1, acc[2 * (Q) + 1]); \
                                     __builtin_amdgcn_sched_barrier(0); } while (0)
#define L2_STEP(X0, X1, EXTRA)                                                                           \
        {                                                                                                \
            uint32_t slot;                                                                               \
            RINGA_SYNC(src, slot, EXTRA);                                                                \
            uint4 wv[2][4];                                                                              \
            L2_READS(0, 0); L2_READS(1, 1);                                                              \
            ALDS_WAITN(4); L2_MMAS(0, 0, X0, X1); RINGA_PIECE(0); L2_READS(0, 2);                        \
            ALDS_WAITN(4); L2_MMAS(1, 1, X0, X1); RINGA_PIECE(1); L2_READS(1, 3);                        \
            ALDS_WAITN(4); L2_MMAS(0, 2, X0, X1); RINGA_PIECE(2);                                        \
            ALDS_WAITN(0); L2_MMAS(1, 3, X0, X1); RINGA_PIECE(3);                                        \
        }
#define L2_BLOCK(L, FETCH)                                                                               \
        {                                                                                                \
            vm_wait_n<8>();                                                                              \
            stage_lines(stg, L, lane);                                                                   \
            opnd xa[2];                              /* two operands at a time: the staged block stays until the next one */ \
            xa[0] = unstage_opnd(stg, 0, m, h); xa[1] = unstage_opnd(stg, 1, m, h);                      \
            if (FETCH) xfetch(L);                                                                        \
            L2_STEP(xa[0], xa[1], (FETCH) ? 4 : 0)                                                       \
            xa[0] = unstage_opnd(stg, 2, m, h); xa[1] = unstage_opnd(stg, 3, m, h);                      \
            L2_STEP(xa[0], xa[1], (FETCH) ? 4 : 0)                                                       \
        }
    for (int pi = 0; pi < my_passes; ++pi) {
        const uint32_t wrow0 = row_of(pi);
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) acc[tt] = zero16();
        for (int b = 1; b < nblk; ++b) L2_BLOCK(L0, 1)
        L2_BLOCK(L0, 0)
        // Epilogue.  The x_hat lines pass through two line blocks (32 registers) twice - once for the row statistics, once for the output,
        // the second time out of L2 - and the residual-gradient lines follow through the same two: every request is issued as soon as
        // the block it overwrites has been staged, one block ahead of its use.
        // (its per-lane addresses are derived from a laundered lane index: held through the ring loop they cost the registers the loop lacks)
        int le = lane;
        asm volatile("" : "+v"(le));
        const int me = le & 31, he = le >> 5;
        Lines la = fetch_lines(XH, wrow0, 512u, 0u, le), lb = fetch_lines(XH, wrow0, 512u, 128u, le);
        float rs = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            Lines& lx = (tp & 1) ? lb : la;
            stage_lines(stg, lx, le);
            if (tp < 2) lx = fetch_lines(XH, wrow0, 512u, 128u * (tp + 2), le);
            else if (tp == 2) lx = fetch_lines(XH, wrow0, 512u, 0u, le);
            else { lx = fetch_lines(RES, wrow0, ldrb, 0u, le); rs = ld4f(RS, (wrow0 + me) * 4u); }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(stg, j, me, he);
#pragma unroll
                for (int i = 0; i < 16; ++i) { s1 += acc[2 * tp + j][i]; s2 = fmaf(acc[2 * tp + j][i], xt[i], s2); }
            }
        }
        s1 = xhalf(s1);
        s2 = xhalf(s2);
        norm_bwd_stats<NORM>(s1, s2, rs);
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            f32x16 o[2];
            stage_lines(stg, la, le);                   // x_hat
            if (tp + 1 < 4) la = fetch_lines(XH, wrow0, 512u, 128u * (tp + 1), le);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x16 xt = unstage_tile(stg, j, me, he);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] = rs * (acc[2 * tp + j][i] - s1 - xt[i] * s2);
            }
            stage_lines(stg, lb, le);                   // residual gradient
            if (tp + 1 < 4) lb = fetch_lines(RES, wrow0, ldrb, 128u * (tp + 1), le);
#pragma unroll
            for (int j = 0; j < 2; ++j) {               // tile by tile, the output over the residual tile it has just read: 16 registers less
                const f32x16 r = unstage_tile(stg, j, me, he);
#pragma unroll
                for (int i = 0; i < 16; ++i) o[j][i] += r[i];
                stage_tile(stg, j, me, he, o[j]);
            }
            flush_lines<false>(stg, Y, wrow0, ldyb, 128u * tp, le);
            if (tp == 1) xfetch(L0);                    // the next pass's first block; behind it: eight more loads and eight line stores
        }
    }
#undef L2_BLOCK
#undef L2_STEP
#undef L2_MMAS
#undef L2_READS
}
#pragma clang diagnostic pop

// ------------------------------------------------------------------------------------------------ weight preparation
// One block per (entry, 32-row tile of W): Wp = bf16(W * gamma[k]) [N][K], WpT = its transpose [K][N] (WpP / WpTP: the same, unit-permuted),
// bp[n] = bias[n] + sum_k W[n][k] * beta[k]  (the LayerNorm affine folded into the linear it feeds).  scalar_gain: gamma is ONE float g
// (a ScaleNorm's gain) applied to every k, no beta: Wp = bf16(g * W), bp = bias.
__global__ __launch_bounds__(256) void prep_weights_kernel(const mmfm_prep_entry* __restrict__ E, int ne) {
    __shared__ float tile[32][33];
    int e = 0;
    while (e + 1 < ne && (int)blockIdx.x >= E[e + 1].tile0) ++e;
    const mmfm_prep_entry en = E[e];
    const int n0 = ((int)blockIdx.x - en.tile0) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    uint16_t* Wp = reinterpret_cast<uint16_t*>(en.Wp);
    uint16_t* WpT = reinterpret_cast<uint16_t*>(en.WpT);
    uint16_t* WpP = reinterpret_cast<uint16_t*>(en.WpP);
    uint16_t* WpTP = reinterpret_cast<uint16_t*>(en.WpTP);
    // unit-permuted position of element i of a row: 4-element (8-byte) units 1 and 2 of every 16 swap places
    auto perm = [](int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); };
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    const float gs = en.scalar_gain ? en.gamma[0] : 1.f;
    for (int k0 = 0; k0 < en.K; k0 += 32) {
        const int k = k0 + tx;
        const float g = en.scalar_gain ? gs : (en.gamma && k < en.K) ? en.gamma[k] : 1.f;
        const float bt = (en.beta && k < en.K && !en.scalar_gain) ? en.beta[k] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + ty + 8 * j;
            const float v = (n < en.N && k < en.K) ? en.W[(size_t)n * en.K + k] : 0.f;
            const float w = v * g;
            dot[j] = fmaf(v, bt, dot[j]);
            if (Wp && n < en.N && k < en.K) Wp[(size_t)n * en.K + k] = f2bf(w);
            if (WpP && n < en.N && k < en.K && perm(k) < en.K) WpP[(size_t)n * en.K + perm(k)] = f2bf(w);    // K % 16 == 0 (mmfm.h)
            tile[ty + 8 * j][tx] = w;
        }
        __syncthreads();
        if (WpT || WpTP) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k0 + ty + 8 * j, n = n0 + tx;
                if (kk < en.K && n < en.N) {
                    if (WpT) WpT[(size_t)kk * en.N + n] = f2bf(tile[tx][ty + 8 * j]);
                    if (WpTP && perm(n) < en.N) WpTP[(size_t)kk * en.N + perm(n)] = f2bf(tile[tx][ty + 8 * j]);   // N % 16 == 0 (mmfm.h)
                }
            }
        }
        __syncthreads();
    }
    if (en.bp) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = dot[j];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) r += __shfl_xor(r, o);
            const int n = n0 + ty + 8 * j;
            if (tx == 0 && n < en.N) en.bp[n] = (en.bias ? en.bias[n] : 0.f) + r;
        }
    }
}

int grid_for(int64_t R, int per_cu, int nw = NW) {
    const int64_t npass = (R + 32 * nw - 1) / (32 * nw);
    return (int)std::max<int64_t>(1, std::min<int64_t>(npass, 256 * per_cu));
}

// Which form a dX + norm-backward launch at K >= 512 takes: 2 = rowgemm_lnbwd2_kernel, two workgroups per CU; 1 = the one-workgroup kernels.
// MMFM_ROWGEMM_LNBWD_WG = 1 or 2 forces one of them at every R.  It is a switch of its own - MMFM_ROWGEMM_WG_PER_CU keeps scaling the grids
// of every other row-owner kernel (and of the one-workgroup kernels here), read once - and it is read at every launch, so that one process
// can run both forms: A/B runs and the bit-identity test need one library and one process.  Default: two workgroups once there are more row
// passes than CUs (with fewer, no CU would hold a second workgroup; B = 16, 64 and 256 measured); MMFM_ROWGEMM_RING
// with bit 1 clear asks for the register-staged ring, which only the one-workgroup kernels have.
int lnbwd_wg_per_cu(int64_t R) {
    static const int ring_env = [] { const char* e = getenv("MMFM_ROWGEMM_RING"); return (e ? atoi(e) : 3) & 2; }();
    const char* e = getenv("MMFM_ROWGEMM_LNBWD_WG");
    const int v = e ? atoi(e) : 0;
    if (v == 1 || v == 2) return v;
    if (!ring_env) return 1;
    return (R + 32 * NW - 1) / (32 * NW) > 256 ? 2 : 1;
}
constexpr int LDS_L2 = RINGA_SLOTS * CHUNK + NW * STG_BYTES;          // 64 KB: two workgroups per CU
int launch_lnbwd2(const mmfm_rowgemm_groups_desc& g, int norm, const void* wbase, const GroupOff& wo, hipStream_t st, const char* who) {
    dim3 grid(grid_for(g.R, 2)), block(NT);
    if (norm == 2) {
        if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_lnbwd2_kernel<2>), LDS_L2, who)) return rc;
        hipLaunchKernelGGL((rowgemm_lnbwd2_kernel<2>), grid, block, LDS_L2, st, g, wbase, wo);
    } else {
        if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_lnbwd2_kernel<1>), LDS_L2, who)) return rc;
        hipLaunchKernelGGL((rowgemm_lnbwd2_kernel<1>), grid, block, LDS_L2, st, g, wbase, wo);
    }
    return 0;
}

}  // namespace

extern "C" int mmfm_rowgemm(const mmfm_rowgemm_desc* dp, mmfm_stream stream) {
    const mmfm_rowgemm_desc d = *dp;
    MMFM_REQUIRE(d.x && d.w && d.y && d.R > 0, "mmfm_rowgemm: null operand / empty problem");
    MMFM_REQUIRE(d.K == 256 || d.K == 512 || d.K == 768, "mmfm_rowgemm: K = %d (256, 512 or 768 only)", d.K);
    MMFM_REQUIRE(d.N > 0 && d.N % 64 == 0, "mmfm_rowgemm: N = %d must be a positive multiple of 64", d.N);
    MMFM_REQUIRE(d.ldx % 8 == 0 && d.ldw % 8 == 0 && d.ldy % 8 == 0 && d.ldx >= d.K && d.ldw >= d.K && d.ldy >= d.N,
                 "mmfm_rowgemm: leading dimensions (%d, %d, %d) must be multiples of 8 and cover the rows", d.ldx, d.ldw, d.ldy);
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    MMFM_REQUIRE(al16(d.x) && al16(d.w) && al16(d.y) && al16(d.residual) && al16(d.xhat) && al16(d.bwd_xhat) && al16(d.bias),
                 "mmfm_rowgemm: operands must be 16-byte aligned");
    MMFM_REQUIRE(!d.residual || (d.ldr % 8 == 0 && d.ldr >= d.N), "mmfm_rowgemm: ldr %d", d.ldr);
    MMFM_REQUIRE(d.ln >= 0 && d.ln <= 2 && d.ln_bwd >= 0 && d.ln_bwd <= 2, "mmfm_rowgemm: ln = %d, ln_bwd = %d (0, 1 = LayerNorm, 2 = ScaleNorm)", d.ln, d.ln_bwd);
    MMFM_REQUIRE(!d.ln || d.K == 256, "mmfm_rowgemm: the norm prologue needs K = 256");
    const int64_t maxld = std::max<int64_t>(std::max(d.ldx, d.ldy), std::max(d.ldr, 256));
    MMFM_REQUIRE((d.R + 128) * maxld * 2 < (int64_t)1 << 31, "mmfm_rowgemm: tensors beyond 2 GiB are not addressable by the 32-bit buffer offsets");
    MMFM_REQUIRE(d.N <= BIAS_MAX, "mmfm_rowgemm: N = %d > %d", d.N, BIAS_MAX);
    // Launch shapes (measured on MI355X at R = 204,800 inside the bench step, profiles/r04_step_launches_B1024.txt; rejected variants - 8 skewed
    // waves, a dedicated weight-stager wave, one 8-wave workgroup per CU, wave pairs at K >= 512 - are described in DESIGN.md sections 3b / 3e):
    //   forward-type, K = 256 : 4 waves, 2 workgroups per CU, LDS-DMA ring (LN+qkv 119 us, LN+kv 94 us, LN+q 62 us, out_proj + residual 69 us,
    //                           plain 56 us); LayerNorm + residual in one launch, and K = 512 / 768: the register-staged ring
    //   LN-backward epilogue  : K = 256 -> wave pairs (8 waves, 101 us); K = 512 / 768 -> beyond 256 row passes rowgemm_lnbwd2_kernel, 4 waves,
    //                           2 workgroups per CU, operand rows streamed (114 / 146 us against 141 / 178 us of the one-workgroup kernels on the
    //                           same box, profiles/rowgemm_lnbwd_two_wg_launches_B1024.txt; DESIGN.md section 3ac, with its rejected variants);
    //                           up to 256 passes, MMFM_ROWGEMM_LNBWD_WG=1 or MMFM_ROWGEMM_RING bit 1 clear: one wave per row tile, one workgroup
    static const int per_cu_env = [] { const char* e = getenv("MMFM_ROWGEMM_WG_PER_CU"); return e ? atoi(e) : 0; }();
    hipStream_t st = (hipStream_t)stream;
    if (d.ln_bwd) {
        MMFM_REQUIRE(d.N == 256 && d.bwd_xhat && d.bwd_rstd && !d.ln && !d.bias, "mmfm_rowgemm: ln_bwd needs N = 256, x_hat, rstd, no bias/ln");
        const bool sn = d.ln_bwd == 2;
        if (d.K == 256) {
            dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 1, 4)), block(512);      // 4 row tiles (wave pairs) per pass
            if (sn) hipLaunchKernelGGL((rowgemm_lnbwd8_kernel<1, 2>), grid, block, 0, st, d);
            else hipLaunchKernelGGL((rowgemm_lnbwd8_kernel<1, 1>), grid, block, 0, st, d);
        } else if (lnbwd_wg_per_cu(d.R) == 2) {                                           // the grouped descriptor's kernel with one group
            mmfm_rowgemm_groups_desc g = {};
            g.R = d.R; g.K = d.K; g.N = d.N; g.groups = 1;
            g.x[0] = d.x; g.ldx = d.ldx; g.w[0] = d.w; g.ldw = d.ldw; g.y[0] = d.y; g.ldy = d.ldy;
            g.residual = d.residual; g.ldr = d.ldr; g.ln_bwd = d.ln_bwd; g.bwd_xhat = d.bwd_xhat; g.bwd_rstd = d.bwd_rstd;
            if (int rc = launch_lnbwd2(g, d.ln_bwd, d.w, GroupOff{}, st, "mmfm_rowgemm")) return rc;
        } else {
            dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 1)), block(NT);
            static const int ring_env = [] { const char* e = getenv("MMFM_ROWGEMM_RING"); return (e ? atoi(e) : 3) & 2; }();   // bit 1 clear: register-staged ring
            constexpr int LDS_L = RINGA_SLOTS * CHUNK + NW * STG_BYTES + NW * 4 * STG_BYTES;
#define LNB_A(KP, NORM)                                                                                                     \
            {                                                                                                               \
                if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_lnbwd_a_kernel<KP, NORM>), LDS_L, "mmfm_rowgemm")) return rc; \
                hipLaunchKernelGGL((rowgemm_lnbwd_a_kernel<KP, NORM>), grid, block, LDS_L, st, d);                           \
            }
            if (ring_env && d.K == 512) { if (sn) LNB_A(2, 2) else LNB_A(2, 1) }
            else if (ring_env) { if (sn) LNB_A(3, 2) else LNB_A(3, 1) }
            else if (d.K == 512) { if (sn) hipLaunchKernelGGL((rowgemm_lnbwd_kernel<2, 2>), grid, block, 0, st, d); else hipLaunchKernelGGL((rowgemm_lnbwd_kernel<2, 1>), grid, block, 0, st, d); }
            else { if (sn) hipLaunchKernelGGL((rowgemm_lnbwd_kernel<3, 2>), grid, block, 0, st, d); else hipLaunchKernelGGL((rowgemm_lnbwd_kernel<3, 1>), grid, block, 0, st, d); }
#undef LNB_A
        }
    } else {
#define RG_LAUNCH(KP, LN)                                                                                   \
    if (d.stream_out) hipLaunchKernelGGL((rowgemm_kernel<KP, LN, true, 4>), grid, block, 0, st, d);         \
    else hipLaunchKernelGGL((rowgemm_kernel<KP, LN, false, 4>), grid, block, 0, st, d);
        if (d.K != 256) {
            dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 1, 4)), block(256);
            if (d.K == 512) { RG_LAUNCH(2, 0) } else { RG_LAUNCH(3, 0) }
        } else {
            dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 2, 4)), block(256);
            static const int ring_env = [] { const char* e = getenv("MMFM_ROWGEMM_RING"); return (e ? atoi(e) : 3) & 1; }();   // bit 0 clear: register-staged ring
            if (ring_env && (!d.residual || (d.N == 256 && !d.ln))) {     // LayerNorm + residual (one launch per step) stays on the staged ring: 171 spills
                constexpr int LDS_A = RINGA_SLOTS * CHUNK + 4 * STG_BYTES + BIAS_MAX * 4;
#define RGA_LAUNCH(LN, NTS, NPV)                                                                                            \
                {                                                                                                          \
                    if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_a_kernel<LN, NTS, NPV>), LDS_A, "mmfm_rowgemm")) return rc; \
                    hipLaunchKernelGGL((rowgemm_a_kernel<LN, NTS, NPV>), grid, block, LDS_A, st, d);                        \
                }
#define RGA_LAUNCH2(LN, NPV) if (d.stream_out) RGA_LAUNCH(LN, true, NPV) else RGA_LAUNCH(LN, false, NPV)
                // fewer row passes than a quarter of the resident slots (2 workgroups per CU): split N into column blocks too (kernel comment)
                const int64_t npass = (d.R + 127) / 128;
                const int np_all = d.N >> 6;
                static const int nsplit_env = [] { const char* e = getenv("MMFM_ROWGEMM_NSPLIT"); return e ? atoi(e) : 1; }();
                const int ny = (nsplit_env && npass < 128) ? (int)std::max<int64_t>(1, std::min<int64_t>(np_all, 512 / npass)) : 1;
                if (d.residual) {                                  // N = 256: four pairs in one block, or one pair in each of four
                    if (ny >= 4) { grid.y = 4; RGA_LAUNCH2(0, 1) } else { RGA_LAUNCH2(0, 4) }
                } else {
                    grid.y = (unsigned)((np_all + (np_all + ny - 1) / ny - 1) / ((np_all + ny - 1) / ny));      // blocks of ceil(np_all / ny) pairs
                    if (d.ln == 2) RGA_LAUNCH2(2, 0)
                    else if (d.ln) RGA_LAUNCH2(1, 0)
                    else RGA_LAUNCH2(0, 0)
                }
#undef RGA_LAUNCH2
#undef RGA_LAUNCH
            } else if (d.ln == 2) { RG_LAUNCH(1, 2) } else if (d.ln) { RG_LAUNCH(1, 1) } else { RG_LAUNCH(1, 0) }
        }
#undef RG_LAUNCH
    }
    MMFM_LAUNCH_CHECK("mmfm_rowgemm");
    return 0;
}

extern "C" int mmfm_rowgemm_lnbwd_form(int64_t R, int K) { return K == 512 || K == 768 ? lnbwd_wg_per_cu(R) : 1; }

extern "C" int mmfm_rowgemm_groups(const mmfm_rowgemm_groups_desc* dp, mmfm_stream stream) {
    const mmfm_rowgemm_groups_desc d = *dp;
    MMFM_REQUIRE(d.groups >= 1 && d.groups <= GROUPS_MAX && d.R > 0, "mmfm_rowgemm_groups: groups = %d (1 .. %d), R = %lld", d.groups, GROUPS_MAX, (long long)d.R);
    MMFM_REQUIRE(d.ln >= 0 && d.ln <= 2 && d.ln_bwd >= 0 && d.ln_bwd <= 2 && (d.ln != 0) != (d.ln_bwd != 0),
                 "mmfm_rowgemm_groups: ln = %d, ln_bwd = %d: exactly one of them must be 1 (LayerNorm) or 2 (ScaleNorm)", d.ln, d.ln_bwd);
    MMFM_REQUIRE(d.ldx % 8 == 0 && d.ldw % 8 == 0 && d.ldy % 8 == 0 && d.ldx >= d.K && d.ldw >= d.K && d.ldy >= d.N,
                 "mmfm_rowgemm_groups: leading dimensions (%d, %d, %d) must be multiples of 8 and cover the rows", d.ldx, d.ldw, d.ldy);
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const int nx = d.ln_bwd ? d.groups : 1, ny = d.ln_bwd ? 1 : d.groups;
    uintptr_t wmin = (uintptr_t)d.w[0];
    for (int g = 0; g < d.groups; ++g) {
        MMFM_REQUIRE(d.w[g] && al16(d.w[g]) && al16(d.bias[g]), "mmfm_rowgemm_groups: group %d: weights NULL or operands not 16-byte aligned", g);
        MMFM_REQUIRE(g >= nx || (d.x[g] && al16(d.x[g])), "mmfm_rowgemm_groups: group %d: x NULL or not 16-byte aligned", g);
        MMFM_REQUIRE(g >= ny || (d.y[g] && al16(d.y[g])), "mmfm_rowgemm_groups: group %d: y NULL or not 16-byte aligned", g);
        wmin = std::min(wmin, (uintptr_t)d.w[g]);
    }
    MMFM_REQUIRE(al16(d.residual) && al16(d.xhat) && al16(d.bwd_xhat), "mmfm_rowgemm_groups: operands must be 16-byte aligned");
    GroupOff wo = {};
    const int64_t wbytes = (int64_t)(d.ln_bwd ? 256 : d.N) * d.ldw * 2;
    for (int g = 0; g < d.groups; ++g) {
        const int64_t off = (int64_t)((uintptr_t)d.w[g] - wmin);
        MMFM_REQUIRE(off + wbytes < (int64_t)1 << 31, "mmfm_rowgemm_groups: group %d: weights more than 2 GiB from the first group's", g);
        wo.w[g] = (uint32_t)off;
    }
    const int64_t maxld = std::max<int64_t>(std::max(d.ldx, d.ldy), std::max(d.ldr, 256));
    MMFM_REQUIRE((d.R + 256) * maxld * 2 < (int64_t)1 << 31, "mmfm_rowgemm_groups: tensors beyond 2 GiB are not addressable by the 32-bit buffer offsets");
    static const int per_cu_env = [] { const char* e = getenv("MMFM_ROWGEMM_WG_PER_CU"); return e ? atoi(e) : 0; }();
    hipStream_t st = (hipStream_t)stream;
    const void* wbase = (const void*)wmin;
    if (d.ln_bwd) {
        MMFM_REQUIRE(d.N == 256 && (d.K == 256 || d.K == 512) && d.bwd_xhat && d.bwd_rstd,
                     "mmfm_rowgemm_groups: ln_bwd needs N = 256, K = 256 or 512 (got %d, %d), x_hat and rstd", d.N, d.K);
        MMFM_REQUIRE(!d.residual || (d.ldr % 8 == 0 && d.ldr >= d.N), "mmfm_rowgemm_groups: ldr %d", d.ldr);
        if (d.K == 512 && lnbwd_wg_per_cu(d.R) == 2) {
            if (int rc = launch_lnbwd2(d, d.ln_bwd, wbase, wo, st, "mmfm_rowgemm_groups")) return rc;
            MMFM_LAUNCH_CHECK("mmfm_rowgemm_groups");
            return 0;
        }
        dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 1)), block(NT);
        constexpr int LDS_L = RINGA_SLOTS * CHUNK + NW * STG_BYTES + NW * 4 * STG_BYTES;
#define GLNB(KP, NORM)                                                                                                      \
        {                                                                                                                   \
            if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_groups_lnbwd_kernel<KP, NORM>), LDS_L, "mmfm_rowgemm_groups")) return rc; \
            hipLaunchKernelGGL((rowgemm_groups_lnbwd_kernel<KP, NORM>), grid, block, LDS_L, st, d, wbase, wo);              \
        }
        if (d.K == 256) { if (d.ln_bwd == 2) GLNB(1, 2) else GLNB(1, 1) }
        else { if (d.ln_bwd == 2) GLNB(2, 2) else GLNB(2, 1) }
#undef GLNB
    } else {
        MMFM_REQUIRE(d.K == 256, "mmfm_rowgemm_groups: the norm prologue needs K = 256 (got %d)", d.K);
        MMFM_REQUIRE(d.N >= 64 && d.N <= 1024 && (d.N & (d.N - 1)) == 0, "mmfm_rowgemm_groups: N = %d must be 64, 128, 256, 512 or 1024", d.N);
        MMFM_REQUIRE(d.groups * d.N <= GBIAS_MAX, "mmfm_rowgemm_groups: groups * N = %d > %d", d.groups * d.N, GBIAS_MAX);
        MMFM_REQUIRE(!d.residual, "mmfm_rowgemm_groups: the grouped forward takes no residual");
        int nps = 0;
        while ((64 << nps) < d.N) ++nps;
        dim3 grid(grid_for(d.R, per_cu_env > 0 ? per_cu_env : 2, 4)), block(256);
        constexpr int LDS_A = RINGA_SLOTS * CHUNK + 4 * STG_BYTES + GBIAS_MAX * 4;
        // fewer row passes than a quarter of the resident slots: column blocks over the pairs of all groups (as mmfm_rowgemm)
        const int64_t npass = (d.R + 127) / 128;
        const int np_all = (d.N >> 6) * d.groups;
        static const int nsplit_env = [] { const char* e = getenv("MMFM_ROWGEMM_NSPLIT"); return e ? atoi(e) : 1; }();
        const int nyb = (nsplit_env && npass < 128) ? (int)std::max<int64_t>(1, std::min<int64_t>(np_all, 512 / npass)) : 1;
        grid.y = (unsigned)((np_all + (np_all + nyb - 1) / nyb - 1) / ((np_all + nyb - 1) / nyb));
#define GFWD(LN, NTS)                                                                                                       \
        {                                                                                                                   \
            if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(rowgemm_groups_a_kernel<LN, NTS>), LDS_A, "mmfm_rowgemm_groups")) return rc; \
            hipLaunchKernelGGL((rowgemm_groups_a_kernel<LN, NTS>), grid, block, LDS_A, st, d, wbase, wo, nps);              \
        }
        if (d.ln == 2) { if (d.stream_out) GFWD(2, true) else GFWD(2, false) }
        else { if (d.stream_out) GFWD(1, true) else GFWD(1, false) }
#undef GFWD
    }
    MMFM_LAUNCH_CHECK("mmfm_rowgemm_groups");
    return 0;
}

extern "C" int mmfm_prep_weights(const mmfm_prep_entry* entries_dev, int n_entries, int total_tiles, mmfm_stream stream) {
    MMFM_REQUIRE(entries_dev && n_entries > 0 && total_tiles > 0, "mmfm_prep_weights: empty table");
    hipLaunchKernelGGL(prep_weights_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, entries_dev, n_entries);
    MMFM_LAUNCH_CHECK("mmfm_prep_weights");
    return 0;
}
