// bf16 attention, dh = 64 or 128, any sequence length (BASELINE configs[4]: d_model 512, 8 heads, L = 600): the keep-bit kernels for heads
// whose K / V images do not fit the LDS.  Same contract as attention_bf16.hip (masks: the whole rule of include/mmfm.h - key padding,
// DIAG, CAUSAL, SEP; dense / DIAG launches run the instantiations they always ran, CAUSAL / SEP launches the MASKED ones, see "mask
// tiles" below), reference: mm_utils.py:97-152, mm.py:178-194.  They replace the round-1 tiled pair (attention_bf16.hip: 0.99 ms forward, 2.64 ms
// two-phase backward per launch at B = 256, L = 600 - 54 of the 98 ms config-5 step) whenever the caller provides the keep-bit
// workspace (mmfm_attn_desc.keepbits):
//   * dropout decisions are the generator kernel's bit tiles (attention_fast.hip): scalar lane masks where the lane is the query
//     (forward, dQ phase), the lane's own word where it is the key (dK / dV phase) - no hash in any of the three kernels;
//   * the forward keeps the first key tile's row maximum as the reference exponent (no running maximum, no rescaling; rows whose sum
//     overflows send the workgroup through an exact pass);
//   * eight waves per workgroup where the registers allow it (forward, dQ phase: 8 query tiles share every streamed K / V chunk), and
//     the next chunk's global loads are in flight while the current one is multiplied (one LDS buffer, register staging);
//   * the backward's per-query constants (delta, the output-dropout'd d_o) are computed ONCE by a small kernel instead of once per
//     workgroup and phase: d_o' lands in the dq buffer (each dQ workgroup reads its own rows before it overwrites them), delta in the
//     tail of the keep-bit workspace.
// The two-phase backward stays (a single pass needs every key tile of a head in one workgroup's registers: 19 tiles x 64 accumulator
// registers), so S and P are evaluated twice; what changed is what an evaluation costs.
#include "attn_common.h"
#include "attn_route.h"
#include <algorithm>
#include <stdlib.h>

using namespace attn;

namespace {

// What follows from the head dim DH (64 or 128), a template parameter of every kernel: KS = DH / 16 k-steps of a 32x32x16 MFMA over the
// head dim, DT = DH / 32 accumulator tiles of an O / dQ / dK / dV tile, C8 = DH / 8 16-byte pieces per row, and
// RS = 2 DH + 16 bytes per LDS image row: 144 B at dh 64, 272 B at dh 128.  Both are 16 B past a multiple of 128 B, so the 16-byte
// fragments of eight consecutive rows cover all 32 banks once: conflict-free row fragments.
constexpr int row_stride(int dh) { return dh * 2 + 16; }
constexpr int CH = 128;                  // streamed rows per chunk (four 32-row tiles)
// waves per SIMD the register allocation must allow (__launch_bounds__): at dh 128 an O / dQ tile is 64 accumulator registers and the
// dK^T + dV^T pair 128, beside twice the operand fragments - half the waves of the dh-64 instantiations, which keep their bounds
constexpr int occ_q(int dh) { return dh > 64 ? 2 : 4; }       // forward, dQ phase (eight waves per workgroup)
constexpr int occ_k(int dh) { return dh > 64 ? 1 : 2; }       // dK / dV phase (four waves per workgroup)
constexpr float OVERFLOW_SUM = 1.2676506e30f;      // 2^100

// ---- chunk streaming: rows [c0, c0 + CH) of two [L][ld] bf16 tensors -> registers -> two LDS images (RS-byte rows); NPT pieces per thread
template <int NT, int DH>
struct Stager {
    static constexpr int C8 = DH / 8, RS = row_stride(DH), NPT = CH * C8 / NT;
    uint4 x[NPT], y[NPT];
    __device__ __forceinline__ void load(const uint16_t* xg, int ldx, const uint16_t* yg, int ldy, int c0, int L, int t) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int idx = t + NT * j, row = c0 + idx / C8, col = idx % C8;
            x[j] = make_uint4(0u, 0u, 0u, 0u); y[j] = x[j];
            if (row < L) {
                x[j] = *reinterpret_cast<const uint4*>(xg + (size_t)row * ldx + 8 * col);
                y[j] = *reinterpret_cast<const uint4*>(yg + (size_t)row * ldy + 8 * col);
            }
        }
    }
    __device__ __forceinline__ void store(char* Xs, char* Ys, int t) const {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int idx = t + NT * j, row = idx / C8, col = idx % C8;
            *reinterpret_cast<uint4*>(Xs + row * RS + col * 16) = x[j];
            *reinterpret_cast<uint4*>(Ys + row * RS + col * 16) = y[j];
        }
    }
};

__device__ __forceinline__ float tile_max16(const f32x16& st) {
    float mx = fmaxf(fmaxf(st[0], st[1]), st[2]);
#pragma unroll
    for (int r = 3; r < 16; ++r) mx = fmaxf(mx, st[r]);
    return xhalf_max(mx);
}

// key bias of a head (0 / -inf per key, -inf beyond Lk) into LDS + "some key of the head is padded" (wave-uniform)
template <int NW>
__device__ __forceinline__ int stage_kbias(float* kbias, int* wflag, const uint8_t* keypad, int b, int Lk, int LkP, int t, int wave, int lane,
                                           bool causal = false) {
    int pad = 0;
    for (int i = t; i < LkP; i += NW * 64) {
        // CAUSAL replaces the key padding: every existing key has bias 0
        const bool ok = i < Lk && (causal || keypad == nullptr || keypad[(size_t)b * Lk + i] != 0);
        kbias[i] = ok ? 0.f : -INFINITY;
        pad |= (i < Lk && !ok) ? 1 : 0;
    }
    const int wv = __any(pad) ? 1 : 0;
    if (lane == 0) wflag[wave] = wv;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) any |= wflag[w];
    return __builtin_amdgcn_readfirstlane(any);
}

// ---------------------------------------------------------------------------------------------- mask tiles (CAUSAL / SEP)
// The MASKED instantiations of the three kernels implement the whole rule of include/mmfm.h with the four tile classes of
// attention_fast.hip (attn_common.h: tile_class, mixed_start).  Heads have any length here, so what the dh = 32 kernels keep in eight
// words lives in LDS arrays sized by the padded length LP (Lq == Lk: launcher), behind the key bias:
//   tmod[LP / 32]  the vote of every 32-position tile: its modality if all 32 mod_id bytes agree (positions beyond L repeat the last
//                  byte), TMOD_MIXED otherwise;
//   cneed[nch]     1 when some wave of the workgroup has a tile of streamed chunk c that is not T_SKIP: a chunk nobody needs is neither
//                  loaded nor staged (a workgroup-uniform walk, so the chunk barriers stay matched);
//   modb[LP]       the mod_id bytes, for the per-element rule of T_MIXED tiles;
// and (forward, dQ phase) kzero[LP], the second bias row of T_ZERO tiles: 0 for every existing key, -inf beyond Lk.
struct MaskLds {
    int* tmod;
    int* cneed;
    uint8_t* modb;
};
__device__ __forceinline__ MaskLds carve_mask(void* p, int LP) {
    MaskLds m;
    m.tmod = reinterpret_cast<int*>(p);
    m.cneed = m.tmod + (LP >> 5);
    m.modb = reinterpret_cast<uint8_t*>(m.cneed + (LP + CH - 1) / CH);
    return m;
}
size_t mask_lds(int LP) { return (size_t)(LP >> 5) * 4 + (size_t)((LP + CH - 1) / CH) * 4 + (size_t)LP + 16; }

// mod_id bytes and tile votes of the head, cneed cleared.  The caller's next workgroup barrier publishes them.
template <int NT>
__device__ __forceinline__ void stage_mask(const MaskLds& m, const uint8_t* mod_id, bool sep, int L, int LP, int nch, int t) {
    const int lane = t & 63;
    for (int i0 = 0; i0 < LP; i0 += NT) {          // workgroup-uniform trip count: every lane of a wave takes part in the ballot
        const int i = i0 + t;
        uint32_t mv = 0u;
        if (sep && i < LP) mv = mod_id[min(i, L - 1)];
        const uint32_t first = (uint32_t)__shfl((int)mv, lane & 32);
        const uint64_t eq = __ballot(mv == first);
        const uint32_t half = (lane & 32) ? (uint32_t)(eq >> 32) : (uint32_t)eq;
        if (i < LP) {                               // LP % 32 == 0: a wave half lies wholly inside or wholly outside
            m.modb[i] = (uint8_t)mv;
            if ((lane & 31) == 0) m.tmod[i >> 5] = half == 0xffffffffu ? (int)mv : TMOD_MIXED;
        }
    }
    for (int i = t; i < nch; i += NT) m.cneed[i] = 0;
}
// every active wave marks the streamed chunks in which its own tile (a query tile when OWN_Q, else a key tile) meets a tile that is
// not T_SKIP; ends with the barrier that publishes cneed
template <bool OWN_Q>
__device__ __forceinline__ void vote_chunks(const MaskLds& m, bool causal, bool sep, bool active, int own, int ntiles, int nch, int lane) {
    if (active) {
        const int town = sep ? m.tmod[own] : 0;
        for (int c = lane; c < nch; c += 64) {
            bool need = false;
            for (int j = 0; j < CH / 32; ++j) {
                const int o = c * (CH / 32) + j;
                if (o < ntiles) {
                    const int toth = sep ? m.tmod[o] : 0;
                    need |= (OWN_Q ? tile_class(causal, sep, town, toth, own, o) : tile_class(causal, sep, toth, town, o, own)) != T_SKIP;
                }
            }
            if (need) m.cneed[c] = 1;
        }
    }
    __syncthreads();
}
// the first needed chunk after c (nch: none); workgroup-uniform
__device__ __forceinline__ int next_needed(const int* cneed, int c, int nch) {
    int n = c + 1;
    while (n < nch && __builtin_amdgcn_readfirstlane(cneed[n]) == 0) ++n;
    return n;
}

// S^T tile of key tile (rows kl*32.. of the K image) against the wave's Q fragments, starting from the key bias.  MASKED and `mixed`
// (a T_MIXED tile): every accumulator start is set from the whole rule, for query q and keys key0 + .., on a branch like dfix
template <int DH, bool MASKED = false>
__device__ __forceinline__ f32x16 score_tile(const char* Ks, const float* kb, int kl, const bf16x8v (&qf)[DH / 16], bool dfix, int kh, int l31,
                                             bool mixed = false, int flags = 0, int q = 0, int key0 = 0, int Lk = 0,
                                             const uint8_t* modb = nullptr) {
    constexpr int KS = DH / 16, RS = row_stride(DH);
    f32x16 a;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 kb4 = *reinterpret_cast<const float4*>(kb + 8 * g + 4 * kh);
        a[4 * g + 0] = kb4.x; a[4 * g + 1] = kb4.y; a[4 * g + 2] = kb4.z; a[4 * g + 3] = kb4.w;
    }
    if (dfix) {              // rare: padded keys and `eye |`: the diagonal keeps S[q][q] finite
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = (mrow(r, kh) == l31) ? 0.f : a[r];
    }
    if constexpr (MASKED) {
        if (mixed) {
            asm volatile("" ::: "memory");
            const bool sep = flags & MMFM_ATTN_SEP;
            const uint32_t mq = sep ? modb[q] : 0u;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t mw = sep ? *reinterpret_cast<const uint32_t*>(modb + key0 + 8 * g + 4 * kh) : 0u;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[4 * g + i] = mixed_start(flags, q, key0 + 8 * g + 4 * kh + i, Lk, a[4 * g + i], mq, (mw >> (8 * i)) & 0xffu);
            }
        }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag(Ks, (kl * 32 + l31) * RS + ks * 32 + kh * 16), qf[ks], a, 0, 0, 0);
    return a;
}

// ---------------------------------------------------------------------------------------------- forward
constexpr int F_NW = 8;
// MASKED = the launch carries CAUSAL and / or SEP (see "mask tiles" above); false compiles to the dense / DIAG kernel as it was.
template <int DH, bool DROP, bool MASKED>
__global__ __launch_bounds__(F_NW * 64, occ_q(DH)) void attn_fwd_long_kernel(const mmfm_attn_desc d, const float keep_scale) {
    constexpr int NW = F_NW, NT = NW * 64, KS = DH / 16, DT = DH / 32, C8 = DH / 8, RS = row_stride(DH);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, kh = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bh_ = attn_xcd_remap((int)blockIdx.x, (int)gridDim.x, d.flags);
    const int b = bh_ / d.heads, h = bh_ % d.heads;
    const int Lq = d.Lq, Lk = d.Lk, LkP = (Lk + 31) & ~31;
    const int nqt = (Lq + 31) >> 5, nkt = LkP >> 5, nch = (LkP + CH - 1) / CH;
    char* Ks = smem;                                   // [CH][RS]
    char* Vs = Ks + CH * RS;                           // [CH][RS]
    char* ost = Vs + CH * RS;                          // [NW][32][RS] output transpose tiles
    float* kbias = reinterpret_cast<float*>(ost + NW * 32 * RS);
    int* wflag = reinterpret_cast<int*>(kbias + LkP);
    float* kzero = reinterpret_cast<float*>(wflag + 16);           // MASKED: the bias row of T_ZERO tiles
    const MaskLds ml = carve_mask(kzero + LkP, LkP);               // MASKED: tile votes, chunk votes, mod_id bytes
    const bool causal = MASKED && (d.flags & MMFM_ATTN_CAUSAL), sep = MASKED && (d.flags & MMFM_ATTN_SEP);
    const uint16_t* qg = reinterpret_cast<const uint16_t*>(d.q) + (size_t)b * Lq * d.ldq + h * DH;
    const uint16_t* kg = reinterpret_cast<const uint16_t*>(d.k) + (size_t)b * Lk * d.ldk + h * DH;
    const uint16_t* vg = reinterpret_cast<const uint16_t*>(d.v) + (size_t)b * Lk * d.ldv + h * DH;

    const int qt = blockIdx.y * NW + wave;
    const bool active = qt < nqt;                      // inactive waves still stage chunks and take part in the barriers
    const int q0 = qt * 32, q = q0 + l31;
    Stager<NT, DH> stg;
    stg.load(kg, d.ldk, vg, d.ldv, 0, Lk, t);          // chunk 0 in flight under the prologue
    bf16x8v qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (active && q < Lq) v = *reinterpret_cast<const uint4*>(qg + (size_t)q * d.ldq + ks * 16 + 8 * kh);
        qf[ks] = __builtin_bit_cast(bf16x8v, v);
    }
    if constexpr (MASKED) {
        for (int i = t; i < LkP; i += NT) kzero[i] = i < Lk ? 0.f : -INFINITY;
        stage_mask<NT>(ml, d.mod_id, sep, Lk, LkP, nch, t);
    }
    const int anypad = stage_kbias<NW>(kbias, wflag, d.keypad, b, Lk, LkP, t, wave, lane, causal);
    int tq = 0;                                        // MASKED: the vote of this wave's query tile
    if constexpr (MASKED) {
        vote_chunks<true>(ml, causal, sep, active, qt, nkt, nch, lane);
        if (sep && active) tq = __builtin_amdgcn_readfirstlane(ml.tmod[qt]);
    }
    const bool fixdiag = anypad && (d.flags & MMFM_ATTN_DIAG);
    const float c2 = d.scale * LOG2E;
    const masks_ptr mkp = reinterpret_cast<masks_ptr>(reinterpret_cast<uintptr_t>(d.keepbits)) + ((size_t)bh_ * nqt + (active ? qt : 0)) * nkt;

    float m_ref = 0.f, l_run = 0.f;
    f32x16 acc[DT];
    // one pass over the head's keys.  EXACT = false: reference exponent = first key tile's row maximum; true: running maximum
    auto pass = [&](auto exact_tag) {
        constexpr bool EXACT = decltype(exact_tag)::value;
        float m_run = -1e30f;
        l_run = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        // MASKED: the walk visits the chunks some wave needs (chunk 0 always is: tile 0 is never T_SKIP, k = 0 <= q)
        for (int c = 0, cn; c < nch; c = cn) {
            cn = c + 1;
            if constexpr (MASKED) cn = next_needed(ml.cneed, c, nch);
            __syncthreads();                           // readers of the previous chunk are done
            stg.store(Ks, Vs, t);
            // the next chunk's loads fly while this one is multiplied (after the last chunk: chunk 0 again, for a possible second pass)
            stg.load(kg, d.ldk, vg, d.ldv, (cn < nch ? cn : 0) * CH, Lk, t);
            __syncthreads();
            if (!active) continue;
            const int ntl = min(CH / 32, nkt - c * (CH / 32));
            for (int kl = 0; kl < ntl; ++kl) {
                const int kt = c * (CH / 32) + kl;
                const float* kb = kbias;
                bool mixed = false;
                if constexpr (MASKED) {
                    const int cls = __builtin_amdgcn_readfirstlane(tile_class(causal, sep, tq, sep ? ml.tmod[kt] : 0, qt, kt));
                    if (cls == T_SKIP) continue;       // contributes exactly nothing; its keep bits are never read
                    if (cls == T_ZERO) kb = kzero;
                    mixed = cls == T_MIXED;
                }
                const f32x16 st = score_tile<DH, MASKED>(Ks, kb + kt * 32, kl, qf, fixdiag && kt == qt, kh, l31, mixed, d.flags, q, kt * 32, Lk, ml.modb);
                Masks16 mk;
                if (DROP) mk = ld_masks(mkp + kt);
                if (EXACT) {
                    const float m_new = v_max(m_run, tile_max16(st) * c2);
                    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
                    for (int i = 0; i < DT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][r] *= alpha;
                    l_run *= alpha;
                    m_run = m_new;
                    m_ref = m_run;
                } else if (kt == 0) {
                    m_ref = v_max(tile_max16(st), -1e30f / c2) * c2;
                }
                uint32_t pk[8];
                float ps0 = 0.f, ps1 = 0.f;
                const float nm = -m_ref;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], c2, nm));
                    float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r + 1], c2, nm));
                    ps0 = v_add(ps0, p0);
                    ps1 = v_add(ps1, p1);
                    if (DROP) {
                        p0 = v_keep(p0, mk.m[r]);
                        p1 = v_keep(p1, mk.m[r + 1]);
                    }
                    asm volatile("" : "+v"(p0), "+v"(p1), "+v"(ps0), "+v"(ps1));     // see attention_fast.hip fwd_tile
                    pk[r >> 1] = pack2(p0, p1);
                }
                l_run = v_add(l_run, v_add(ps0, ps1));
                const bf16x8v lo = __builtin_bit_cast(bf16x8v, make_uint4(pk[0], pk[1], pk[2], pk[3]));
                const bf16x8v hi = __builtin_bit_cast(bf16x8v, make_uint4(pk[4], pk[5], pk[6], pk[7]));
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag(Vs, RS, kl * 32, i * 32, lane), lo, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag(Vs, RS, kl * 32 + 16, i * 32, lane), hi, acc[i], 0, 0, 0);
                }
            }
        }
    };
    pass(std::false_type{});
    float l_tot = xhalf_sum(l_run);
    // exact pass if ANY row of the workgroup overflowed its first-tile reference (the chunk barriers need every wave)
    const int bad = (active && __any(!(l_tot < OVERFLOW_SUM))) ? 1 : 0;
    __syncthreads();
    if (lane == 0) wflag[wave] = bad;
    __syncthreads();
    int redo = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) redo |= wflag[w];
    if (__builtin_amdgcn_readfirstlane(redo)) {
        pass(std::true_type{});
        l_tot = xhalf_sum(l_run);
    }
    if (!active) return;
    const Drop dout = drop_init(d.drop_o);
    const float inv = keep_scale / l_tot;
    if (kh == 0 && q < Lq) d.lse[(size_t)bh_ * Lq + q] = m_ref * LN2 + __logf(l_tot);
    // O^T (rows = d in registers, lane = query) -> bf16 rows [query][d] through the wave's staging tile, output dropout on the way
    char* tl = ost + wave * 32 * RS;
    uint16_t* og = reinterpret_cast<uint16_t*>(d.o) + (size_t)b * Lq * d.ldo + h * DH;
    const uint64_t base = ((uint64_t)b * Lq + (uint64_t)q) * (uint64_t)(d.heads * DH) + (uint64_t)(h * DH);
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = i * 32 + 8 * g + 4 * kh;
            float v0 = acc[i][4 * g + 0] * inv, v1 = acc[i][4 * g + 1] * inv, v2 = acc[i][4 * g + 2] * inv, v3 = acc[i][4 * g + 3] * inv;
            if (dout.on()) {
                dout.apply2(v0, v1, base + d0);
                dout.apply2(v2, v3, base + d0 + 2);
            }
            *reinterpret_cast<uint2*>(tl + l31 * RS + d0 * 2) = make_uint2(pack2(v0, v1), pack2(v2, v3));
        }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < 32 * C8 / 64; ++i) {
        const int idx = lane + 64 * i, row = idx / C8, c = idx % C8;
        if (q0 + row < Lq)
            *reinterpret_cast<uint4*>(og + (size_t)(q0 + row) * d.ldo + 8 * c) = *reinterpret_cast<const uint4*>(tl + row * RS + c * 16);
    }
}
size_t fwd_long_lds(int dh, int Lk, bool masked) {
    const int LkP = (Lk + 31) & ~31, RS = row_stride(dh);
    return (size_t)2 * CH * RS + (size_t)F_NW * 32 * RS + (size_t)LkP * 4 + 64 + (masked ? (size_t)LkP * 4 + mask_lds(LkP) : 0);
}

// ---------------------------------------------------------------------------------------------- backward: per-query constants
// d_o' = dropout'(d_o) as bf16 -> the dq buffer (scratch until the dQ phase overwrites it with dq);  delta / dropout scale -> dl[bh][q]
template <int DH>
__global__ __launch_bounds__(256) void attn_bwd_long_prep_kernel(const mmfm_attn_desc d, float* dl, const float inv_keep) {
    constexpr int C8 = DH / 8;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one 16-byte piece per thread: (token row, head, piece)
    const int64_t total = (int64_t)d.B * d.Lq * d.heads * C8;
    const bool ok = idx < total;
    const int c = (int)(idx % C8), h = (int)((idx / C8) % d.heads);
    const int64_t row = ok ? idx / (C8 * d.heads) : 0;                     // b * Lq + q
    const Drop dout = drop_init(d.drop_o);
    uint4 g = make_uint4(0u, 0u, 0u, 0u), o = g;
    if (ok) {
        g = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(d.d_o) + row * d.lddo + h * DH + 8 * c);
        o = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(d.o) + row * d.ldo + h * DH + 8 * c);
    }
    const uint32_t gw[4] = {g.x, g.y, g.z, g.w}, ow[4] = {o.x, o.y, o.z, o.w};
    const uint64_t base = (uint64_t)row * (uint64_t)(d.heads * DH) + (uint64_t)(h * DH + 8 * c);
    float part = 0.f, gd[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float g0 = __uint_as_float(gw[j] << 16), g1 = __uint_as_float(gw[j] & 0xffff0000u);
        const float o0 = __uint_as_float(ow[j] << 16), o1 = __uint_as_float(ow[j] & 0xffff0000u);
        part += g0 * o0 + g1 * o1;
        if (dout.on()) dout.apply2(g0, g1, base + 2 * j);
        gd[2 * j] = g0;
        gd[2 * j + 1] = g1;
    }
#pragma unroll
    for (int off = 1; off < C8; off <<= 1) part += __shfl_xor(part, off);       // the C8 pieces of a (row, head) sit in neighbouring lanes
    if (ok) {
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(d.dq) + row * d.lddq + h * DH + 8 * c) = __builtin_bit_cast(uint4, pack8(gd));
        if (c == 0) {
            const int64_t bq = row / d.Lq, qq = row % d.Lq;
            dl[(bq * d.heads + h) * d.Lq + qq] = part * inv_keep;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward, dQ phase
// A workgroup owns eight query tiles (one per wave: Q, d_o', lse, delta in registers, the query on the lane) and streams K / V.
constexpr int Q_NW = 8;
template <int DH, bool DROP, bool MASKED>
__global__ __launch_bounds__(Q_NW * 64, occ_q(DH)) void attn_bwd_long_dq_kernel(const mmfm_attn_desc d, const float* dl, const float keep_scale) {
    constexpr int NW = Q_NW, NT = NW * 64, KS = DH / 16, DT = DH / 32, RS = row_stride(DH);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, kh = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bh_ = attn_xcd_remap((int)blockIdx.x, (int)gridDim.x, d.flags);
    const int b = bh_ / d.heads, h = bh_ % d.heads;
    const int Lq = d.Lq, Lk = d.Lk, LkP = (Lk + 31) & ~31;
    const int nqt = (Lq + 31) >> 5, nkt = LkP >> 5, nch = (LkP + CH - 1) / CH;
    char* Ks = smem;
    char* Vs = Ks + CH * RS;
    char* sct = Vs + CH * RS;                          // [NW][32][RS] dQ transpose tiles
    float* kbias = reinterpret_cast<float*>(sct + NW * 32 * RS);
    int* wflag = reinterpret_cast<int*>(kbias + LkP);
    float* kzero = reinterpret_cast<float*>(wflag + 16);           // MASKED: as in the forward
    const MaskLds ml = carve_mask(kzero + LkP, LkP);
    const bool causal = MASKED && (d.flags & MMFM_ATTN_CAUSAL), sep = MASKED && (d.flags & MMFM_ATTN_SEP);
    const uint16_t* qg = reinterpret_cast<const uint16_t*>(d.q) + (size_t)b * Lq * d.ldq + h * DH;
    const uint16_t* kg = reinterpret_cast<const uint16_t*>(d.k) + (size_t)b * Lk * d.ldk + h * DH;
    const uint16_t* vg = reinterpret_cast<const uint16_t*>(d.v) + (size_t)b * Lk * d.ldv + h * DH;
    const uint16_t* dog = reinterpret_cast<const uint16_t*>(d.dq) + (size_t)b * Lq * d.lddq + h * DH;      // d_o' (prep kernel)

    const int qt = blockIdx.y * NW + wave;
    const bool active = qt < nqt;
    const int q = qt * 32 + l31;
    Stager<NT, DH> stg;
    stg.load(kg, d.ldk, vg, d.ldv, 0, Lk, t);
    // Q fragments stay in registers; the d_o' fragments of the wave's rows live in its (until the end unused) transpose tile and are
    // re-read per key tile: at dh 64 (128 registers) the kernel spills 33 with both resident next to two dQ tiles, S and dP; the
    // dh-128 form keeps the arrangement and has 232-238 of its 256 registers in use without a spill
    char* dot = sct + wave * 32 * RS;
    bf16x8v qfr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        uint4 qv = make_uint4(0u, 0u, 0u, 0u), gv = qv;
        if (active && q < Lq) {
            qv = *reinterpret_cast<const uint4*>(qg + (size_t)q * d.ldq + ks * 16 + 8 * kh);
            gv = *reinterpret_cast<const uint4*>(dog + (size_t)q * d.lddq + ks * 16 + 8 * kh);
        }
        qfr[ks] = __builtin_bit_cast(bf16x8v, qv);
        *reinterpret_cast<uint4*>(dot + l31 * RS + ks * 32 + kh * 16) = gv;
    }
    float lq = 0.f, dq_ = 0.f;
    if (active && q < Lq) {
        lq = d.lse[(size_t)bh_ * Lq + q] * LOG2E;
        dq_ = dl[(size_t)bh_ * Lq + q];
    }
    if constexpr (MASKED) {
        for (int i = t; i < LkP; i += NT) kzero[i] = i < Lk ? 0.f : -INFINITY;
        stage_mask<NT>(ml, d.mod_id, sep, Lk, LkP, nch, t);
    }
    const int anypad = stage_kbias<NW>(kbias, wflag, d.keypad, b, Lk, LkP, t, wave, lane, causal);
    int tq = 0;
    if constexpr (MASKED) {
        vote_chunks<true>(ml, causal, sep, active, qt, nkt, nch, lane);
        if (sep && active) tq = __builtin_amdgcn_readfirstlane(ml.tmod[qt]);
    }
    const bool fixdiag = anypad && (d.flags & MMFM_ATTN_DIAG);
    const float c2 = d.scale * LOG2E, osc = d.scale * keep_scale;
    const masks_ptr mkp = reinterpret_cast<masks_ptr>(reinterpret_cast<uintptr_t>(d.keepbits)) + ((size_t)bh_ * nqt + (active ? qt : 0)) * nkt;
    f32x16 dQt[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQt[i][r] = 0.f;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int c = 0, cn; c < nch; c = cn) {             // MASKED: the chunks some wave needs, as in the forward
        cn = c + 1;
        if constexpr (MASKED) cn = next_needed(ml.cneed, c, nch);
        // (no register prefetch of the next chunk here: at dh 64 the 16 staging registers spill beside Q, d_o' and two dQ tiles; at
        // dh 128 they are 32, beside four dQ tiles, and do not fit either)
        if (c > 0) stg.load(kg, d.ldk, vg, d.ldv, c * CH, Lk, t);
        __syncthreads();
        stg.store(Ks, Vs, t);
        __syncthreads();
        if (!active) continue;
        const int ntl = min(CH / 32, nkt - c * (CH / 32));
        for (int kl = 0; kl < ntl; ++kl) {
            const int kt = c * (CH / 32) + kl;
            const float* kb = kbias;
            bool mixed = false;
            if constexpr (MASKED) {
                const int cls = __builtin_amdgcn_readfirstlane(tile_class(causal, sep, tq, sep ? ml.tmod[kt] : 0, qt, kt));
                if (cls == T_SKIP) continue;
                if (cls == T_ZERO) kb = kzero;
                mixed = cls == T_MIXED;
            }
            // S^T[key][q] + key bias
            const f32x16 s = score_tile<DH, MASKED>(Ks, kb + kt * 32, kl, qfr, fixdiag && kt == qt, kh, l31, mixed, d.flags, q, kt * 32, Lk, ml.modb);
            f32x16 dpv = zero;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)                                                                    // dP^T[key][q]
                dpv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag(Vs, (kl * 32 + l31) * RS + ks * 32 + kh * 16),
                                                              rowfrag(dot, l31 * RS + ks * 32 + kh * 16), dpv, 0, 0, 0);
            Masks16 mk;
            if (DROP) mk = ld_masks(mkp + kt);
            uint32_t sk[8];
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                float e[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r + j], c2, -lq));       // padded keys: exp2(-inf) = 0
                    const float pm = DROP ? v_keep(p, mk.m[r + j]) : p;
                    e[j] = __builtin_fmaf(pm, dpv[r + j], -v_mul(p, dq_));                             // dS / dropout scale
                }
                asm volatile("" : "+v"(e[0]), "+v"(e[1]));
                sk[r >> 1] = pack2(e[0], e[1]);
            }
            const bf16x8v sf[2] = {__builtin_bit_cast(bf16x8v, make_uint4(sk[0], sk[1], sk[2], sk[3])),
                                   __builtin_bit_cast(bf16x8v, make_uint4(sk[4], sk[5], sk[6], sk[7]))};
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    dQt[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag(Ks, RS, kl * 32 + 16 * s2, i * 32, lane), sf[s2], dQt[i], 0, 0, 0);
        }
    }
    if (!active) return;
    store_tile_T<DH, DT>(sct + wave * 32 * RS, RS, dQt, reinterpret_cast<uint16_t*>(d.dq) + (size_t)b * Lq * d.lddq + h * DH, d.lddq, qt * 32, Lq,
                         lane, osc);
}
size_t dq_long_lds(int dh, int Lk, bool masked) {
    const int LkP = (Lk + 31) & ~31, RS = row_stride(dh);
    return (size_t)2 * CH * RS + (size_t)Q_NW * 32 * RS + (size_t)LkP * 4 + 64 + (masked ? (size_t)LkP * 4 + mask_lds(LkP) : 0);
}

// ---------------------------------------------------------------------------------------------- backward, dK / dV phase
// A workgroup owns four key tiles (one per wave: K, V operands and the 2 x 2 accumulator tiles in registers, the key on the lane) and
// streams Q / d_o' with their per-query constants.  dh 64: 128 accumulator + operand registers per wave, two waves per SIMD; dh 128:
// the dK^T + dV^T tiles alone are 128 accumulator registers (152-160 AGPRs in all) beside 64 of K / V fragments, one wave per SIMD.
constexpr int K_NW = 4;
// MASKED: a wave (one key tile) classifies the query tiles it meets; the walk visits the query chunks some wave needs - under CAUSAL
// those from the workgroup's first diagonal tile on, unless SEP allows something before it.
template <int DH, bool DROP, bool MASKED>
__global__ __launch_bounds__(K_NW * 64, occ_k(DH)) void attn_bwd_long_dkv_kernel(const mmfm_attn_desc d, const float* dl, const float keep_scale) {
    constexpr int NW = K_NW, NT = NW * 64, KS = DH / 16, DT = DH / 32, RS = row_stride(DH);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, kh = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bh_ = attn_xcd_remap((int)blockIdx.x, (int)gridDim.x, d.flags);
    const int b = bh_ / d.heads, h = bh_ % d.heads;
    const int Lq = d.Lq, Lk = d.Lk, LqP = (Lq + 31) & ~31, LkP = (Lk + 31) & ~31;
    const int nqt = LqP >> 5, nkt = LkP >> 5, nch = (LqP + CH - 1) / CH;
    char* As = smem;                                   // Q chunk
    char* Bs = As + CH * RS;                           // d_o' chunk
    float* lse2 = reinterpret_cast<float*>(Bs + CH * RS);          // [CH] lse * log2 e of the chunk's queries
    float* dlc = lse2 + CH;                                         // [CH] delta / dropout scale
    char* sct = reinterpret_cast<char*>(dlc + CH);                  // [NW][32][RS] output transpose tiles
    int* wflag = reinterpret_cast<int*>(sct + NW * 32 * RS);
    const MaskLds ml = carve_mask(wflag + 16, LqP);                 // MASKED: tile votes, chunk votes, mod_id bytes
    const bool causal = MASKED && (d.flags & MMFM_ATTN_CAUSAL), sep = MASKED && (d.flags & MMFM_ATTN_SEP);
    const uint16_t* qg = reinterpret_cast<const uint16_t*>(d.q) + (size_t)b * Lq * d.ldq + h * DH;
    const uint16_t* kg = reinterpret_cast<const uint16_t*>(d.k) + (size_t)b * Lk * d.ldk + h * DH;
    const uint16_t* vg = reinterpret_cast<const uint16_t*>(d.v) + (size_t)b * Lk * d.ldv + h * DH;
    const uint16_t* dog = reinterpret_cast<const uint16_t*>(d.dq) + (size_t)b * Lq * d.lddq + h * DH;      // d_o' (prep kernel)

    const int kt = blockIdx.y * NW + wave;
    const bool active = kt < nkt;
    const int key = kt * 32 + l31;
    Stager<NT, DH> stg;
    if constexpr (!MASKED) stg.load(qg, d.ldq, dog, d.lddq, 0, Lq, t);         // MASKED: the first chunk is known after the votes
    float lse_n = 0.f, dl_n = 0.f;                     // the next chunk's per-query constants (threads 0 .. CH-1)
    auto load_consts = [&](int c0) {
        lse_n = 0.f; dl_n = 0.f;
        if (t < CH && c0 + t < Lq) { lse_n = d.lse[(size_t)bh_ * Lq + c0 + t] * LOG2E; dl_n = dl[(size_t)bh_ * Lq + c0 + t]; }
    };
    if constexpr (!MASKED) load_consts(0);
    bf16x8v kfr[KS], vfr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        uint4 kv = make_uint4(0u, 0u, 0u, 0u), vv = kv;
        if (active && key < Lk) {
            kv = *reinterpret_cast<const uint4*>(kg + (size_t)key * d.ldk + ks * 16 + 8 * kh);
            vv = *reinterpret_cast<const uint4*>(vg + (size_t)key * d.ldv + ks * 16 + 8 * kh);
        }
        kfr[ks] = __builtin_bit_cast(bf16x8v, kv);
        vfr[ks] = __builtin_bit_cast(bf16x8v, vv);
    }
    // key bias of this lane's key; "a key of the head is padded" decides between the literal-zero and the bias-initialised S product
    int pad = 0;
    for (int i = t; i < Lk; i += NT) pad |= (!causal && d.keypad != nullptr && d.keypad[(size_t)b * Lk + i] == 0) ? 1 : 0;   // CAUSAL replaces the padding
    const int wv = __any(pad) ? 1 : 0;
    if (lane == 0) wflag[wave] = wv;
    const bool kok = key < Lk && (causal || d.keypad == nullptr || d.keypad[(size_t)b * Lk + (key < Lk ? key : 0)] != 0);
    const float kbv = kok ? 0.f : -INFINITY;
    // keep words of (query tile i, this wave's key tile): key l31 = mrow(r, kh') sits in word 2 r + kh' of its tile
    const uint32_t* kbp = reinterpret_cast<const uint32_t*>(d.keepbits) + ((size_t)bh_ * nqt * nkt + min(kt, nkt - 1)) * 32 +
                          2 * ((l31 & 3) + 4 * (l31 >> 3)) + ((l31 >> 2) & 1);
    const int kw_stride = nkt * 32;
    uint32_t kw_next = 0u;
    if (DROP && !MASKED) kw_next = kbp[0];
    if constexpr (MASKED) stage_mask<NT>(ml, d.mod_id, sep, Lq, LqP, nch, t);
    __syncthreads();
    int anypad = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) anypad |= wflag[w];
    int c0 = 0, tk = 0;                                // MASKED: the first chunk of the walk, the vote of this wave's key tile
    if constexpr (MASKED) {
        vote_chunks<false>(ml, causal, sep, active, kt, nqt, nch, lane);
        if (sep && active) tk = __builtin_amdgcn_readfirstlane(ml.tmod[kt]);
        c0 = next_needed(ml.cneed, -1, nch);
        if (c0 < nch) { stg.load(qg, d.ldq, dog, d.lddq, c0 * CH, Lq, t); load_consts(c0 * CH); }
    }
    // (keys beyond Lk need no bias here: their K / V rows are zero, their accumulator lanes are never stored and nothing is exchanged)
    anypad = __builtin_amdgcn_readfirstlane(anypad);
    const float c2 = d.scale * LOG2E;
    f32x16 dKt[DT], dVt[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dKt[i][r] = 0.f; dVt[i][r] = 0.f; }
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    for (int c = c0, cn; c < nch; c = cn) {
        cn = c + 1;
        if constexpr (MASKED) cn = next_needed(ml.cneed, c, nch);
        __syncthreads();
        stg.store(As, Bs, t);
        if (t < CH) { lse2[t] = lse_n; dlc[t] = dl_n; }
        if (cn < nch) { stg.load(qg, d.ldq, dog, d.lddq, cn * CH, Lq, t); load_consts(cn * CH); }
        __syncthreads();
        if (!active) continue;
        const int ntl = min(CH / 32, nqt - c * (CH / 32));
        for (int ql = 0; ql < ntl; ++ql) {
            const int qt = c * (CH / 32) + ql;
            bool zstart = !anypad, mixed = false;
            uint32_t kwv = 0u;
            if constexpr (MASKED) {
                const int cls = __builtin_amdgcn_readfirstlane(tile_class(causal, sep, sep ? ml.tmod[qt] : 0, tk, qt, kt));
                if (cls == T_SKIP) continue;           // contributes exactly nothing; its keep bits are never read
                zstart = zstart || cls == T_ZERO;
                mixed = cls == T_MIXED;
                if (DROP) kwv = kbp[(size_t)qt * kw_stride];          // no prefetch chain across skipped tiles: requested ahead of the MFMAs
            }
            f32x16 s, dpv = zero;
            if (MASKED && mixed) {
                // T_MIXED: the whole rule per element (lane = key, register = query)
                const uint32_t mk = sep ? ml.modb[min(key, LkP - 1)] : 0u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint32_t mw = sep ? *reinterpret_cast<const uint32_t*>(ml.modb + qt * 32 + 8 * g + 4 * kh) : 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        s[4 * g + i] = mixed_start(d.flags, qt * 32 + 8 * g + 4 * kh + i, key, Lk, kbv, (mw >> (8 * i)) & 0xffu, mk);
                }
            } else if (zstart) {
                s = zero;
            } else {
                const bool dfix = (d.flags & MMFM_ATTN_DIAG) && qt == kt;
                int lv = l31;
                asm volatile("" : "+v"(lv));
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = (dfix && mrow(r, kh) == lv) ? 0.f : kbv;
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int off = (ql * 32 + l31) * RS + ks * 32 + kh * 16;
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag(As, off), kfr[ks], s, 0, 0, 0);        // S[q][key]
                dpv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rowfrag(Bs, off), vfr[ks], dpv, 0, 0, 0);    // dP[q][key]
            }
            uint32_t wq = 0u;
            if (DROP) {
                if constexpr (MASKED) {
                    wq = kwv >> (4 * kh);
                } else {
                    wq = kw_next >> (4 * kh);          // bit (r & 3) + 8 (r >> 2) is now register r's query
                    kw_next = kbp[(size_t)min(qt + 1, nqt - 1) * kw_stride];
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint32_t pkp[4], pks[4];
                const int qb = ql * 32 + 16 * s2 + 4 * kh;             // chunk-local queries qb + 0..3 and qb + 8 + 0..3
#pragma unroll
                for (int e4 = 0; e4 < 2; ++e4) {
                    const float4 l4 = *reinterpret_cast<const float4*>(lse2 + qb + 8 * e4), d4 = *reinterpret_cast<const float4*>(dlc + qb + 8 * e4);
                    const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
                    float pm[4], ds[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 8 * s2 + 4 * e4 + i;
                        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -lq[i]));
                        pm[i] = p;
                        if (DROP) {
                            int m = __builtin_amdgcn_sbfe((int)wq, (r & 3) + 8 * (r >> 2), 1);
                            asm volatile("" : "+v"(m));
                            pm[i] = __uint_as_float(__float_as_uint(p) & (uint32_t)m);
                        }
                        ds[i] = __builtin_fmaf(pm[i], dpv[r], -v_mul(p, dq_[i]));
                    }
                    pkp[2 * e4] = pack2(pm[0], pm[1]); pkp[2 * e4 + 1] = pack2(pm[2], pm[3]);
                    pks[2 * e4] = pack2(ds[0], ds[1]); pks[2 * e4 + 1] = pack2(ds[2], ds[3]);
                }
                const bf16x8v pf = __builtin_bit_cast(bf16x8v, make_uint4(pkp[0], pkp[1], pkp[2], pkp[3]));
                const bf16x8v sf = __builtin_bit_cast(bf16x8v, make_uint4(pks[0], pks[1], pks[2], pks[3]));
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    dVt[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag(Bs, RS, ql * 32 + 16 * s2, i * 32, lane), pf, dVt[i], 0, 0, 0);
                    dKt[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(trfrag(As, RS, ql * 32 + 16 * s2, i * 32, lane), sf, dKt[i], 0, 0, 0);
                }
            }
        }
    }
    if (!active) return;
    char* tl = sct + wave * 32 * RS;
    store_tile_T<DH, DT>(tl, RS, dKt, reinterpret_cast<uint16_t*>(d.dk) + (size_t)b * Lk * d.lddk + h * DH, d.lddk, kt * 32, Lk, lane, d.scale * keep_scale);
    store_tile_T<DH, DT>(tl, RS, dVt, reinterpret_cast<uint16_t*>(d.dv) + (size_t)b * Lk * d.lddv + h * DH, d.lddv, kt * 32, Lk, lane, keep_scale);
}
size_t dkv_long_lds(int dh, int Lq, bool masked) {
    const int RS = row_stride(dh);
    return (size_t)2 * CH * RS + (size_t)2 * CH * 4 + (size_t)K_NW * 32 * RS + 64 + (masked ? mask_lds((Lq + 31) & ~31) : 0);
}

}  // namespace

int mmfm_attn_keepbits_launch(const mmfm_attn_desc& d, hipStream_t st);          // attention_fast.hip

// dh = 64 or 128 with the keep-bit workspace (MMFM_ATTN_LONG=0: never).
bool mmfm_attn_long_takes(const mmfm_attn_desc& d) {
    static const bool off = [] { const char* e = getenv("MMFM_ATTN_LONG"); return e && atoi(e) == 0; }();
    if (off || (d.dh != 64 && d.dh != 128) || d.keepbits == nullptr) return false;
    const bool masked = (d.flags & (MMFM_ATTN_CAUSAL | MMFM_ATTN_SEP)) != 0;
    if (masked && (d.Lq != d.Lk || ((d.flags & MMFM_ATTN_SEP) && d.mod_id == nullptr))) return false;
    if (d.Lq % 8 || d.Lk % 8) return false;
    // the key bias (and the MASKED kernels' second bias row, mod_id bytes and votes) grow with Lk: past what a workgroup can have,
    // the whole shape - forward and backward alike - belongs to the general kernels
    if (fwd_long_lds(d.dh, d.Lk, masked) > ATTN_LDS_MAX || dq_long_lds(d.dh, d.Lk, masked) > ATTN_LDS_MAX) return false;
    if (attn_drop_p_on(d) && d.drop_p.p >= 1.f) return false;
    return attn_io_aligned(d) && (uintptr_t)d.keepbits % 128 == 0;
}

int mmfm_attn_long_launch(const mmfm_attn_desc& d, bool backward, hipStream_t st) {
    const bool masked = (d.flags & (MMFM_ATTN_CAUSAL | MMFM_ATTN_SEP)) != 0, drop = attn_drop_p_on(d);
    const int nqt = (d.Lq + 31) / 32, nkt = (d.Lk + 31) / 32, bh = d.B * d.heads;
    const float keep_scale = drop ? 1.f / mmfm_attn_keep_prob(d.drop_p.p) : 1.f;
    // delta / dropout scale per (b, head, query): the tail of the keep-bit workspace, behind the bit tiles
    float* dl = reinterpret_cast<float*>(reinterpret_cast<char*>(d.keepbits) + (size_t)bh * nqt * nkt * 128);
#define LAUNCH(KERN, GRID, NTH, LDSB, WHAT, ...)                                                                    \
    {                                                                                                               \
        auto kern = KERN;                                                                                           \
        if (int rc = mmfm_lds_opt_in(reinterpret_cast<const void*>(kern), LDSB, WHAT)) return rc;                   \
        hipLaunchKernelGGL(kern, GRID, dim3(NTH), LDSB, st, __VA_ARGS__);                                           \
    }
    // <DH, dropout, MASKED>
#define LAUNCH3(KERN, DHV, ...)                                                                                     \
    {                                                                                                               \
        if (drop) { if (masked) LAUNCH((KERN<DHV, true, true>), __VA_ARGS__) else LAUNCH((KERN<DHV, true, false>), __VA_ARGS__) }     \
        else { if (masked) LAUNCH((KERN<DHV, false, true>), __VA_ARGS__) else LAUNCH((KERN<DHV, false, false>), __VA_ARGS__) }       \
    }
#define LAUNCH2(KERN, ...)                                                                                          \
    {                                                                                                               \
        if (d.dh == 64) LAUNCH3(KERN, 64, __VA_ARGS__) else LAUNCH3(KERN, 128, __VA_ARGS__)                         \
    }
    if (!backward) {
        if (drop) { if (int rc = mmfm_attn_keepbits_launch(d, st)) return rc; }
        const size_t lds = fwd_long_lds(d.dh, d.Lk, masked);
        const dim3 grid(bh, (nqt + F_NW - 1) / F_NW);
        LAUNCH2(attn_fwd_long_kernel, grid, F_NW * 64, lds, "mmfm_attn_fwd(bf16, keep bits)", d, keep_scale)
        MMFM_LAUNCH_CHECK("mmfm_attn_fwd(bf16, keep bits)");
        return 0;
    }
    const int64_t pieces = (int64_t)d.B * d.Lq * d.heads * (d.dh / 8);
    if (d.dh == 64) hipLaunchKernelGGL(attn_bwd_long_prep_kernel<64>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, d, dl, 1.f / keep_scale);
    else hipLaunchKernelGGL(attn_bwd_long_prep_kernel<128>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, d, dl, 1.f / keep_scale);
    {
        const size_t lds = dkv_long_lds(d.dh, d.Lq, masked);
        const dim3 grid(bh, (nkt + K_NW - 1) / K_NW);
        LAUNCH2(attn_bwd_long_dkv_kernel, grid, K_NW * 64, lds, "mmfm_attn_bwd(bf16, keep bits, dK dV)", d, dl, keep_scale)
    }
    {
        const size_t lds = dq_long_lds(d.dh, d.Lk, masked);
        const dim3 grid(bh, (nqt + Q_NW - 1) / Q_NW);
        LAUNCH2(attn_bwd_long_dq_kernel, grid, Q_NW * 64, lds, "mmfm_attn_bwd(bf16, keep bits, dQ)", d, dl, keep_scale)
    }
#undef LAUNCH2
#undef LAUNCH3
#undef LAUNCH
    MMFM_LAUNCH_CHECK("mmfm_attn_bwd(bf16, keep bits)");
    return 0;
}
