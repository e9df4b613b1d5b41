// Span packing (include/mmfm.h, MMFM_SPAN_PACK): the spans of a flat fp32 buffer named by a device table, gathered into a packed staging
// buffer and scattered back.  Data parallelism over per-session layers all-reduces the staging buffer: the sessions one step touched
// instead of the whole session block (ddp.py).
//
// Both kernels are copies and memory-bound.  The table is data of a captured launch, so nothing of the geometry may depend on it: a
// fixed grid walks all (span, chunk) pairs.  Every workgroup reads the table front to back (wave-uniform loads of 32 bytes per span,
// L2 hits after the first workgroup) and keeps the number of chunks in front of the current span; chunk c of that span belongs to
// workgroup (chunks in front + c) mod the grid size, a power of two.  Consecutive chunks therefore go to consecutive workgroups whether they belong to one
// long span or to many short ones, and no prefix table has to be built or uploaded.
// Measured on the read-out block of 8 of 40 sessions (16 spans, 20 MB moved): the map as a 64-bit modulo cost more than
// the copy (17.4 us a launch against 9.6 us with the mask), and 2048 workgroups are slower than 1024 (15.1 us): each one walks the
// whole table, so beyond a full device more workgroups only add walks.
//
// A chunk is MMFM_SPAN_CHUNK = 4096 elements: four 16-byte accesses per lane of a 256-lane workgroup, each wave instruction 1 KiB
// contiguous, the four loads issued before the first store.  A span moves in 16-byte accesses where its two addresses agree modulo 16
// bytes (ddp.py pads every packed span to a multiple of four elements and the layout's slots are 32-byte aligned, so the spans it
// builds always do): the chunks cut the aligned interior, the at most three elements of the head and of the tail ride with chunk 0.
// Where the addresses disagree the whole span moves element by element, in chunks of the same size.
#include "common.h"

#include <algorithm>

namespace {

constexpr int SPAN_BLOCK = 256;
constexpr int SPAN_GRID = 1024;                     // 4 workgroups per CU; a span block of 8 sessions is a few hundred chunks
static_assert((SPAN_GRID & (SPAN_GRID - 1)) == 0, "the chunk -> workgroup map is a mask: a 64-bit modulo per span and workgroup cost more than the copy");
constexpr int64_t SPAN_QUADS = MMFM_SPAN_CHUNK / 4;   // 16-byte accesses per chunk
constexpr int SPAN_PER_LANE = MMFM_SPAN_CHUNK / 4 / SPAN_BLOCK;      // ... and per lane
static_assert(SPAN_PER_LANE >= 1 && SPAN_PER_LANE * 4 * SPAN_BLOCK == MMFM_SPAN_CHUNK, "a chunk is a whole number of 16-byte accesses per lane");

// GATHER: dst = the staging buffer at s_off, src = G at g_off, a dead span stores zeros and loads nothing.
// SCATTER: dst = G at g_off, src = the staging buffer at s_off, every span is copied.
template <bool GATHER>
__global__ __launch_bounds__(SPAN_BLOCK) void span_pack_kernel(const float* __restrict__ from, float* __restrict__ to,
                                                               const int64_t* __restrict__ table, int n_spans) {
    const int t = threadIdx.x;
    uint32_t front = 0;                               // chunks of the spans in front of span s, modulo the grid
    for (int s = 0; s < n_spans; ++s) {               // (rows beyond n_spans are never read)
        const int64_t g_off = table[4 * s], s_off = table[4 * s + 1], len = table[4 * s + 2];
        if (len <= 0 || g_off < 0 || s_off < 0) continue;
        const bool live = !GATHER || table[4 * s + 3] != 0;
        const float* src = from + (GATHER ? g_off : s_off);
        float* dst = to + (GATHER ? s_off : g_off);
        const bool vec = (((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0;
        // [a0, a1): the interior whose quads are 16-byte aligned in both buffers (empty for an element-wise span)
        int64_t a0 = 0, a1 = 0;
        if (vec) {
            const int64_t head = (int64_t)((4 - (((uintptr_t)dst & 15) >> 2)) & 3);
            a0 = head < len ? head : len;
            a1 = a0 + ((len - a0) & ~(int64_t)3);
        }
        const int64_t nq = (a1 - a0) >> 2;
        const int64_t chunks = vec ? (nq > SPAN_QUADS ? (nq + SPAN_QUADS - 1) / SPAN_QUADS : 1) : (len + MMFM_SPAN_CHUNK - 1) / MMFM_SPAN_CHUNK;
        int64_t c = (blockIdx.x - front) & (uint32_t)(SPAN_GRID - 1);
        front = (front + (uint32_t)chunks) & (uint32_t)(SPAN_GRID - 1);
        for (; c < chunks; c += SPAN_GRID) {
            if (vec) {
                const int64_t q0 = c * SPAN_QUADS + t;
                float4 v[SPAN_PER_LANE];
#pragma unroll
                for (int j = 0; j < SPAN_PER_LANE; ++j) {
                    const int64_t q = q0 + (int64_t)j * SPAN_BLOCK;
                    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (live && q < nq) v[j] = *reinterpret_cast<const float4*>(src + a0 + 4 * q);
                }
#pragma unroll
                for (int j = 0; j < SPAN_PER_LANE; ++j) {
                    const int64_t q = q0 + (int64_t)j * SPAN_BLOCK;
                    if (q < nq) *reinterpret_cast<float4*>(dst + a0 + 4 * q) = v[j];
                }
                if (c == 0) {                         // head [0, a0) and tail [a1, len): at most three elements each
                    if (t < a0) dst[t] = live ? src[t] : 0.f;
                    const int64_t i = a1 + (t - 64);  // (the second wave: the first one has the head)
                    if (t >= 64 && i < len) dst[i] = live ? src[i] : 0.f;
                }
            } else {
                const int64_t i0 = c * MMFM_SPAN_CHUNK + t;
#pragma unroll 4
                for (int j = 0; j < 4 * SPAN_PER_LANE; ++j) {
                    const int64_t i = i0 + (int64_t)j * SPAN_BLOCK;
                    if (i < len) dst[i] = live ? src[i] : 0.f;
                }
            }
        }
    }
}

int span_check(const char* who, const void* g, const void* stage, const int64_t* table, int n_spans) {
    MMFM_REQUIRE(g && stage && table, "%s: NULL pointer (G %p, stage %p, table %p)", who, g, stage, (const void*)table);
    MMFM_REQUIRE(((uintptr_t)g & 3) == 0 && ((uintptr_t)stage & 3) == 0 && ((uintptr_t)table & 7) == 0,
                 "%s: G and stage are 4-byte aligned, the table 8-byte aligned (G %p, stage %p, table %p)", who, g, stage, (const void*)table);
    MMFM_REQUIRE(n_spans >= 0 && n_spans <= MMFM_SPAN_MAX, "%s: n_spans = %d outside [0, %d]", who, n_spans, MMFM_SPAN_MAX);
    return 0;
}

}  // namespace

extern "C" int mmfm_span_gather(const float* G, float* stage, const int64_t* table, int n_spans, mmfm_stream stream) {
    if (span_check("mmfm_span_gather", G, stage, table, n_spans)) return -1;
    if (n_spans == 0) return 0;
    hipLaunchKernelGGL(span_pack_kernel<true>, dim3(SPAN_GRID), dim3(SPAN_BLOCK), 0, (hipStream_t)stream, G, stage, table, n_spans);
    MMFM_LAUNCH_CHECK("mmfm_span_gather");
    return 0;
}

extern "C" int mmfm_span_scatter(const float* stage, float* G, const int64_t* table, int n_spans, mmfm_stream stream) {
    if (span_check("mmfm_span_scatter", G, stage, table, n_spans)) return -1;
    if (n_spans == 0) return 0;
    hipLaunchKernelGGL(span_pack_kernel<false>, dim3(SPAN_GRID), dim3(SPAN_BLOCK), 0, (hipStream_t)stream, stage, G, table, n_spans);
    MMFM_LAUNCH_CHECK("mmfm_span_scatter");
    return 0;
}
