// Host side of the GEMM dispatch: which kernel family takes a descriptor (gemm_route in gemm.hip decides it once per call, for mmfm_gemm,
// mmfm_gemm_live and mmfm_gemm_pair alike) and what each family file offers the route.  No device code.
#pragma once
#include "common.h"

struct GemmRoute {
    int family = 0;              // MMFM_GEMM_FAMILY_*; the streaming kernel's tile width is part of it (DW128 / DW256)
};

// what 16-byte accesses need of an operand (an optional one may be NULL) and of its leading dimension, in bf16 elements
inline bool gemm_al16(const void* p) { return p == nullptr || (uintptr_t)p % 16 == 0; }
inline bool gemm_ld8(int ld) { return ld % 8 == 0; }

// Per family file: a predicate over the checked descriptor (gemm_check) and the live-row record of the call, and a launch that assumes
// the route chose it and returns 0 or an error.  The two predicates are disjoint by layout: big wants both operands K-contiguous, dw neither.
bool mmfm_gemm_big_takes(const mmfm_gemm_desc& d, const LiveArg& lv);                    // gemm_big.hip: 256 x 256 tiles for the compute-bound shapes
int mmfm_gemm_big_launch(const mmfm_gemm_desc& d, hipStream_t st, const LiveArg& lv);
bool mmfm_gemm_dw_takes(const mmfm_gemm_desc& d, const LiveArg& lv, bool& wide);         // gemm_dw.hip: the HBM-bound weight-gradient stream
bool mmfm_gemm_dw_pair_takes(const mmfm_gemm_desc& a, const mmfm_gemm_desc& b);          // ... and two of them in one launch (no live record)
int mmfm_gemm_dw_launch(const mmfm_gemm_desc& d, const mmfm_gemm_desc* second, bool wide, hipStream_t st, const LiveArg& lv);
int mmfm_gemm_bf16_launch(const mmfm_gemm_desc& d, hipStream_t st, const LiveArg& lv);   // gemm_bf16.hip: 128 x 128 tiles, every bf16 descriptor

// route and launch a descriptor built inside the library (stitch.hip): valid by construction, so no gemm_check
int mmfm_gemm_routed(const mmfm_gemm_desc& d, hipStream_t st);
