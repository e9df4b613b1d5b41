// Host side of the attention dispatch: which kernel family takes a descriptor (attn_route in attention.hip decides it once per call,
// forward and backward from the same predicates) and what each family file offers the route.  No device code.
#pragma once
#include "common.h"

constexpr size_t ATTN_LDS_MAX = 160 * 1024;      // dynamic LDS a workgroup can opt in to

struct AttnRoute {
    int family = 0;              // MMFM_ATTN_FAMILY_*
    int fwd_waves = 4;           // MMFM_ATTN_FAMILY_BF16 forward: waves per workgroup
    bool bwd_single = false;     // MMFM_ATTN_FAMILY_BF16 backward: the single-pass kernel, not the two-phase pair
    const mmfm_attn_window* win = nullptr;   // set by the entry point BEFORE the route runs: the launch's window (MMFM_ATTN_WINDOW), or none
};

// what the bf16 kernels' 16-byte accesses need of q / k / v / o ...
inline bool attn_io_aligned(const mmfm_attn_desc& d) {
    return d.ldq % 8 == 0 && d.ldk % 8 == 0 && d.ldv % 8 == 0 && d.ldo % 8 == 0 && (uintptr_t)d.q % 16 == 0 && (uintptr_t)d.k % 16 == 0 &&
           (uintptr_t)d.v % 16 == 0 && (uintptr_t)d.o % 16 == 0;
}
// ... and of the gradient tensors, which only the backward sees: the route, not a family, decides what their misalignment means
inline bool attn_grads_aligned(const mmfm_attn_desc& d) {
    return d.lddo % 8 == 0 && d.lddq % 8 == 0 && d.lddk % 8 == 0 && d.lddv % 8 == 0 && (uintptr_t)d.d_o % 16 == 0 && (uintptr_t)d.dq % 16 == 0 &&
           (uintptr_t)d.dk % 16 == 0 && (uintptr_t)d.dv % 16 == 0;
}
inline bool attn_drop_p_on(const mmfm_attn_desc& d) { return d.drop_p.p > 0.f && d.drop_p.state != nullptr; }

// Per family file: a predicate over what the forward sees (shape, flags, operand alignment, workspace, dropout, the LDS formulas beside
// the kernels) - never the direction - and a launch that assumes the route chose it and returns 0 or an error.
// attention_fast.hip: keep-bit kernels, dh 32; win: the launch carries a window (the WIN instantiations take it)
bool mmfm_attn_fast_takes(const mmfm_attn_desc& d, bool win = false);
int mmfm_attn_fast_launch(const mmfm_attn_desc& d, bool backward, hipStream_t st, const mmfm_attn_window* win = nullptr);
bool mmfm_attn_long_takes(const mmfm_attn_desc& d);                                      // attention_long.hip: keep-bit kernels, dh 64 / 128
int mmfm_attn_long_launch(const mmfm_attn_desc& d, bool backward, hipStream_t st);
// attention_bf16.hip: the bf16 MFMA kernels, LDS-resident or (force_tiled, dh 128, or a head that does not fit) tiled; fills r.
// r.win counts in the LDS formulas and picks the WINDOW instantiations at launch; attention_long.hip is never asked under a window.
bool mmfm_attn_bf16_takes(const mmfm_attn_desc& d, bool force_tiled, AttnRoute& r);
int mmfm_attn_bf16_launch(const mmfm_attn_desc& d, const AttnRoute& r, bool backward, hipStream_t st);
