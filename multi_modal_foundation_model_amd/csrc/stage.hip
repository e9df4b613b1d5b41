// Input staging under a per-element corruption mask (MMFM_LOSS_ELEM, include/mmfm.h): dst[b,t,n] = cm(b,t,n) ? 0 : src[b,t,n], written
// into the engine's static input buffer (its dtype, its padded row pitch) - the copy load_inputs makes, with the masker's zeroing folded
// in.  The mask is read in its compact form (any stride may be 0); the padding columns of dst are not touched.  Memory-bound: V
// elements per thread, 16-byte loads of src and 16-byte (fp32, bf16 at V = 8) or 8-byte (bf16 at V = 4) stores where the shapes allow.
#include "common.h"
#include <algorithm>

namespace {

template <typename T, int V>
__global__ __launch_bounds__(256) void stage_masked_kernel(const float* __restrict__ src, const uint8_t* __restrict__ cm, int64_t sb, int64_t st,
                                                           int64_t sn, int Tn, int64_t R, int N, T* __restrict__ dst, int ld) {
    const int cpr = N / V;                       // chunks per row: N % V == 0, so a chunk never crosses a row
    const int64_t total = R * cpr;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / cpr;
        const int c = (int)(idx - row * cpr) * V;
        const uint8_t* m = cm + (row / Tn) * sb + (row % Tn) * st + c * sn;
        const float* s = src + row * N + c;
        T* d = dst + row * ld + c;
        float v[V];
        if constexpr (V == 1) {
            v[0] = s[0];
        } else {
#pragma unroll
            for (int i = 0; i < V; i += 4) {
                const float4 f = *reinterpret_cast<const float4*>(s + i);
                v[i] = f.x; v[i + 1] = f.y; v[i + 2] = f.z; v[i + 3] = f.w;
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = m[i * sn] ? 0.f : v[i];          // a select: a NaN under the mask becomes 0
        if constexpr (V == 1) {
            io<T>::st(d, v[0]);
        } else if constexpr (V == 8) {                                       // bf16 only: one 16-byte store
            uint4 u;
            u.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
            u.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
            u.z = (uint32_t)f2bf(v[4]) | ((uint32_t)f2bf(v[5]) << 16);
            u.w = (uint32_t)f2bf(v[6]) | ((uint32_t)f2bf(v[7]) << 16);
            *reinterpret_cast<uint4*>(d) = u;
        } else {
            io<T>::st4(d, make_float4(v[0], v[1], v[2], v[3]));
        }
    }
}

template <typename T, int V>
void launch_stage(const float* src, const uint8_t* cm, int64_t sb, int64_t st, int64_t sn, int T_, int64_t R, int N, void* dst, int ld,
                  hipStream_t stream) {
    const int64_t n = R * (N / V);
    dim3 grid((int)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 255) / 256))), block(256);
    hipLaunchKernelGGL((stage_masked_kernel<T, V>), grid, block, 0, stream, src, cm, sb, st, sn, T_, R, N, (T*)dst, ld);
}

}  // namespace

extern "C" int mmfm_stage_masked(int dtype, const float* src, const uint8_t* cm, int64_t sb, int64_t st, int64_t sn, int B, int T, int N,
                                 void* dst, int ld_dst, mmfm_stream stream) {
    MMFM_REQUIRE(src && cm && dst, "mmfm_stage_masked: null pointer");
    MMFM_REQUIRE(dtype == MMFM_F32 || dtype == MMFM_BF16, "mmfm_stage_masked: bad dtype %d", dtype);
    MMFM_REQUIRE(B > 0 && T > 0 && N > 0 && ld_dst >= N && sb >= 0 && st >= 0 && sn >= 0, "mmfm_stage_masked: bad arguments");
    const int64_t R = (int64_t)B * T;
    hipStream_t s = (hipStream_t)stream;
    const bool a16 = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    if (dtype == MMFM_F32) {
        if (a16 && N % 4 == 0 && ld_dst % 4 == 0) launch_stage<float, 4>(src, cm, sb, st, sn, T, R, N, dst, ld_dst, s);
        else launch_stage<float, 1>(src, cm, sb, st, sn, T, R, N, dst, ld_dst, s);
    } else {
        if (a16 && N % 8 == 0 && ld_dst % 8 == 0) launch_stage<uint16_t, 8>(src, cm, sb, st, sn, T, R, N, dst, ld_dst, s);
        else if (a16 && N % 4 == 0 && ld_dst % 4 == 0) launch_stage<uint16_t, 4>(src, cm, sb, st, sn, T, R, N, dst, ld_dst, s);
        else launch_stage<uint16_t, 1>(src, cm, sb, st, sn, T, R, N, dst, ld_dst, s);
    }
    MMFM_LAUNCH_CHECK("mmfm_stage_masked");
    return 0;
}
