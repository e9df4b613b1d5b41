"""ctypes binding of libmmfm_hip.so (the C-ABI declared in include/mmfm.h).

There is NO fallback: if the shared library is missing or a call fails this raises.  Build with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C multi_modal_foundation_model_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

# torch ships its own ROCm runtime (libamdhip64 under torch/lib).  It MUST be loaded before
# libmmfm_hip.so so that both resolve to the same HIP runtime instance: device pointers and streams
# handed over by torch are only meaningful inside the runtime that created them.
import torch  # noqa: F401  (load order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMFM_LIB") or os.path.join(_HERE, "libmmfm_hip.so")    # MMFM_LIB: A/B another build of the same library
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmfm.h")

F32, BF16 = 0, 1
ATTN_DIAG, ATTN_CAUSAL, ATTN_SEP = 1, 2, 4
# mmfm_attn_family (MMFM_ATTN_FAMILY_*)
ATTN_FAMILY_KEEPBIT_DH32, ATTN_FAMILY_KEEPBIT_LONG, ATTN_FAMILY_BF16, ATTN_FAMILY_BF16_TILED, ATTN_FAMILY_F32, ATTN_FAMILY_F32_TILED = range(1, 7)
ATTN_FAMILY_MASK, ATTN_FAMILY_BWD_SINGLE = 0xf, 0x10
ATTN_KEEPBIT_FAMILIES = (ATTN_FAMILY_KEEPBIT_DH32, ATTN_FAMILY_KEEPBIT_LONG)
# mmfm_gemm_family (MMFM_GEMM_FAMILY_*)
GEMM_FAMILY_F32, GEMM_FAMILY_TILE128, GEMM_FAMILY_BIG256, GEMM_FAMILY_DW128, GEMM_FAMILY_DW256 = range(1, 6)
ACT_NONE, ACT_GELU, ACT_SOFTSIGN, ACT_GELU_GRAD, ACT_SOFTSIGN_GRAD, ACT_SOFTSIGN_GRAD_OUT = 0, 1, 2, 3, 4, 5
# the other MLP activations (transformer.act): forward / gradient pairs; the sigmoid kind takes beta in act_scale
ACT_RELU, ACT_RELU_GRAD, ACT_SIGMOID, ACT_SIGMOID_GRAD, ACT_GELU_TANH, ACT_GELU_TANH_GRAD = 6, 7, 8, 9, 10, 11
# the embedder activations (embedder.act other than softsign): forward / gradient pairs, act_scale = the embedder's scale in all of them
(ACT_EMB_IDENTITY, ACT_EMB_IDENTITY_GRAD, ACT_EMB_RELU, ACT_EMB_RELU_GRAD, ACT_EMB_GELU, ACT_EMB_GELU_GRAD, ACT_EMB_SILU, ACT_EMB_SILU_GRAD,
 ACT_EMB_QUICK_GELU, ACT_EMB_QUICK_GELU_GRAD, ACT_EMB_GELU_TANH, ACT_EMB_GELU_TANH_GRAD, ACT_EMB_TANH, ACT_EMB_TANH_GRAD) = range(12, 26)
# mmfm_mlp_desc.act (MMFM_MLP_*)
MLP_GELU, MLP_RELU, MLP_SIGMOID, MLP_GELU_TANH = 0, 1, 2, 3
# masked-loss kinds (MMFM_LOSS_*) and the PoissonNLLLoss(full=True) flag
LOSS_POISSON_LOG, LOSS_MSE, LOSS_POISSON_RATE, LOSS_L1, LOSS_SMOOTH_L1, LOSS_HUBER, LOSS_BCE_LOGITS = range(7)
LOSS_FULL = 1
# softmax cross-entropy (MMFM_LOSS_SOFTMAX_CE): served by mmfm_softmax_ce_fwd / _bwd only, the kind entry points refuse it
LOSS_SOFTMAX_CE = 7


class MmfmError(RuntimeError):
    pass


class Dropout(C.Structure):
    _fields_ = [("state", C.c_void_p), ("site", C.c_uint32), ("p", C.c_float)]


NO_DROP = Dropout(None, 0, 0.0)


class GemmDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("c_f32", C.c_int), ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
                ("a_kcontig", C.c_int), ("b_kcontig", C.c_int), ("splits", C.c_int), ("kchunk", C.c_int),
                ("slab_stride", C.c_int64), ("bias", C.c_void_p), ("pre_out", C.c_void_p), ("act", C.c_int),
                ("act_scale", C.c_float), ("gradmul_pre", C.c_void_p), ("drop", Dropout), ("residual", C.c_void_p),
                ("ldr", C.c_int), ("colsum", C.c_void_p)]


class LiveRows(C.Structure):
    """mmfm_live_rows: the live-bin record of a modality slot (int32 [live_rec_ints(T)], mmfm_live_bins) and the row space B * T it compacts."""
    _fields_ = [("rec", C.c_void_p), ("B", C.c_int), ("T", C.c_int)]


OPTIM_CHUNK = 4096               # MMFM_OPTIM_CHUNK
GRAD_STASH, GRAD_ADD = 0, 1      # MMFM_GRAD_STASH, MMFM_GRAD_ADD


class OptimRange(C.Structure):
    """mmfm_optim_range: [start, end) in elements of the flat buffers and the row of the hyper table it is updated with."""
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("hyper_row", C.c_int32), ("reserved", C.c_int32)]


class OptimChunk(C.Structure):
    """mmfm_optim_chunk: one entry of the table mmfm_optim_ranges_table writes."""
    _fields_ = [("start", C.c_int64), ("len", C.c_int32), ("range", C.c_int32), ("hyper_row", C.c_int32), ("reserved", C.c_int32)]


class OptimRecord(C.Structure):
    """mmfm_optim_record: what mmfm_grad_sumsq_ranges leaves at the start of its workspace."""
    _fields_ = [("total", C.c_double), ("clip_coef", C.c_float), ("nonfinite", C.c_int32), ("skipped", C.c_int64),
                ("n_ranges", C.c_int32), ("reserved", C.c_int32)]


def live_rec_ints(T):
    """MMFM_LIVE_REC_INTS: T_live + 3 reserved, live_t[T], rank[T]."""
    return 2 * T + 4


class AttnDesc(C.Structure):
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("heads", C.c_int), ("Lq", C.c_int), ("Lk", C.c_int), ("dh", C.c_int),
                ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_int), ("ldk", C.c_int),
                ("ldv", C.c_int), ("o", C.c_void_p), ("ldo", C.c_int), ("lse", C.c_void_p), ("keypad", C.c_void_p),
                ("mod_id", C.c_void_p), ("flags", C.c_int), ("scale", C.c_float), ("drop_p", Dropout),
                ("drop_o", Dropout), ("d_o", C.c_void_p), ("lddo", C.c_int), ("dq", C.c_void_p), ("dk", C.c_void_p),
                ("dv", C.c_void_p), ("lddq", C.c_int), ("lddk", C.c_int), ("lddv", C.c_int), ("keepbits", C.c_void_p)]


class AttnWindow(C.Structure):
    """mmfm_attn_window (MMFM_ATTN_WINDOW): int32 time stamps [B][L] and the closed interval [lo, hi] of allowed pos[k] - pos[q]."""
    _fields_ = [("pos", C.c_void_p), ("lo", C.c_int), ("hi", C.c_int)]


ATTN_WINDOW_INF = 1 << 30        # lo / hi beyond it are clamped to it
ATTN_POS_CLAMP = 1 << 29         # mmfm_attn_pos_prep clamps the stamps to it


class PrepEntry(C.Structure):
    _fields_ = [("W", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("bias", C.c_void_p), ("Wp", C.c_void_p),
                ("WpT", C.c_void_p), ("bp", C.c_void_p), ("N", C.c_int), ("K", C.c_int), ("tile0", C.c_int), ("scalar_gain", C.c_int),
                ("WpP", C.c_void_p), ("WpTP", C.c_void_p)]


class ReduceEntry(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("n", C.c_int64), ("slab_stride", C.c_int64), ("nslabs", C.c_int32),
                ("accumulate", C.c_int32), ("chunk0", C.c_int32), ("pad_", C.c_int32)]


class SessionDesc(C.Structure):
    """mmfm_session_desc (MMFM_SESSION_LINEAR): the batch shape, the device session tables and the flat weight / bias buffers."""
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("T", C.c_int), ("P", C.c_int), ("N_max", C.c_int), ("S", C.c_int), ("ld_pad", C.c_int), ("ld_p", C.c_int),
                ("sid", C.c_void_p), ("n", C.c_void_p), ("w_off", C.c_void_p), ("b_off", C.c_void_p), ("w", C.c_void_p), ("w_elems", C.c_int64),
                ("bias", C.c_void_p), ("b_elems", C.c_int64)]


SESSION_MAX_PER_BATCH = 64       # distinct sessions in one batch (the capacity of mmfm_session_dw's chunk table)
SESSION_RUN_HDR, SESSION_RUN_ENT = 4, 4
SPAN_CHUNK, SPAN_MAX = 4096, 65536       # MMFM_SPAN_CHUNK, MMFM_SPAN_MAX


class RowGemmDesc(C.Structure):
    _fields_ = [("R", C.c_int64), ("K", C.c_int), ("N", C.c_int), ("x", C.c_void_p), ("ldx", C.c_int), ("w", C.c_void_p),
                ("ldw", C.c_int), ("bias", C.c_void_p), ("ln", C.c_int), ("eps", C.c_float), ("xhat", C.c_void_p),
                ("rstd", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int), ("y", C.c_void_p), ("ldy", C.c_int),
                ("stream_out", C.c_int), ("rotate", C.c_int), ("ln_bwd", C.c_int), ("bwd_xhat", C.c_void_p), ("bwd_rstd", C.c_void_p)]


ROWGEMM_MAX_GROUPS = 8
MAX_SEGMENTS = 8                 # MMFM_MAX_SEGMENTS
MT_MAX_STREAMS = 1024            # MMFM_MT_MAX_STREAMS


class RowGemmGroupsDesc(C.Structure):
    """mmfm_rowgemm_groups_desc: the row-owner linear over up to ROWGEMM_MAX_GROUPS weight sets in one launch."""
    _fields_ = [("R", C.c_int64), ("K", C.c_int), ("N", C.c_int), ("groups", C.c_int), ("x", C.c_void_p * ROWGEMM_MAX_GROUPS), ("ldx", C.c_int),
                ("w", C.c_void_p * ROWGEMM_MAX_GROUPS), ("ldw", C.c_int), ("bias", C.c_void_p * ROWGEMM_MAX_GROUPS),
                ("y", C.c_void_p * ROWGEMM_MAX_GROUPS), ("ldy", C.c_int), ("ln", C.c_int), ("eps", C.c_float), ("xhat", C.c_void_p),
                ("rstd", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int), ("stream_out", C.c_int), ("rotate", C.c_int),
                ("ln_bwd", C.c_int), ("bwd_xhat", C.c_void_p), ("bwd_rstd", C.c_void_p)]


class MlpDesc(C.Structure):
    _fields_ = [("R", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int), ("eps", C.c_float), ("w_up", C.c_void_p),
                ("b_up", C.c_void_p), ("w_down", C.c_void_p), ("b_down", C.c_void_p), ("drop", Dropout), ("y", C.c_void_p),
                ("ldy", C.c_int), ("xhat", C.c_void_p), ("rstd", C.c_void_p), ("dy", C.c_void_p), ("lddy", C.c_int),
                ("w_down_t", C.c_void_p), ("w_up_t", C.c_void_p), ("t1", C.c_void_p), ("g", C.c_void_p), ("du", C.c_void_p),
                ("dx", C.c_void_p), ("lddx", C.c_int), ("rotate", C.c_int), ("scalenorm", C.c_int),
                ("act", C.c_int), ("act_beta", C.c_float)]


_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_PROTOS = {
    "mmfm_version": (C.c_int, []),
    "mmfm_last_error": (C.c_char_p, []),
    "mmfm_device_check": (C.c_int, [_i]),
    "mmfm_rng_seed": (C.c_int, [_vp, C.c_uint64, _vp]),
    "mmfm_rng_advance": (C.c_int, [_vp, _vp]),
    "mmfm_gemm": (C.c_int, [C.POINTER(GemmDesc), _vp]),
    "mmfm_gemm_pair": (C.c_int, [_vp, _vp, _vp]),
    "mmfm_gemm_live": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(LiveRows), _vp]),
    "mmfm_gemm_family": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(LiveRows)]),
    "mmfm_gemm_pair_fused": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(GemmDesc)]),
    "mmfm_live_bins": (C.c_int, [_vp, _i, _i, _vp, _vp]),
    "mmfm_gather_live_rows": (C.c_int, [_vp, _vp, _i, _i, _i64, _vp, _vp]),
    "mmfm_gemm_dw_tiles": (C.c_int, [_i, _i, _i]),
    "mmfm_reduce_slabs": (C.c_int, [_vp, _vp, _i64, _i, _i64, _i, _vp]),
    "mmfm_reduce_slabs_multi": (C.c_int, [_vp, _i, _i, _vp]),
    "mmfm_colsum_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_colsum": (C.c_int, [_i, _vp, _i64, _i, _i, _vp, _i, _vp, _i64, _vp]),
    "mmfm_layernorm_fwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _i, _i, _vp]),
    "mmfm_layernorm_bwd_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_layernorm_bwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _vp, _i64, _vp]),
    "mmfm_scalenorm_fwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp]),
    "mmfm_scalenorm_bwd_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_scalenorm_bwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _vp, _i64, _vp]),
    "mmfm_attn_fwd": (C.c_int, [C.POINTER(AttnDesc), _vp]),
    "mmfm_attn_bwd": (C.c_int, [C.POINTER(AttnDesc), _vp]),
    "mmfm_attn_keepbits_bytes": (C.c_int64, [_i, _i, _i, _i]),
    "mmfm_attn_keep_prob": (C.c_float, [_f]),
    "mmfm_attn_family": (C.c_int, [C.POINTER(AttnDesc), _i]),
    # attention inside a window over time stamps (MMFM_ATTN_WINDOW)
    "mmfm_attn_win_fwd": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(AttnWindow), _vp]),
    "mmfm_attn_win_bwd": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(AttnWindow), _vp]),
    "mmfm_attn_win_family": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(AttnWindow), _i]),
    "mmfm_attn_pos_prep": (C.c_int, [_i, _i, C.POINTER(C.c_int32), C.POINTER(_vp), _vp, _vp]),
    "mmfm_mask_prep": (C.c_int, [_i, _i, _i, C.POINTER(_vp), C.POINTER(_i64), _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp, _vp]),
    "mmfm_collate_csr": (C.c_int, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mmfm_stitch_fwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mmfm_stitch_fwd_live": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mmfm_stitch_bwd_live": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, Dropout, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "mmfm_stitch_bwd_workspace": (C.c_int64, [_i, _i, _i, _i, _i, _i]),
    "mmfm_stitch_bwd": (C.c_int, [_i, _vp, _vp, _vp, _vp, Dropout, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    # modality segments (MMFM_MOD_SEGMENTS)
    "mmfm_mask_prep_seg": (C.c_int, [_i, _i, C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64), _vp, _vp, _vp, _vp,
                                     _vp, _vp]),
    "mmfm_stitch_fwd_seg": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mmfm_stitch_bwd_seg_workspace": (C.c_int64, [_i, _i, _i, _i, _i, _i, _i]),
    "mmfm_stitch_bwd_seg": (C.c_int, [_i, _vp, _vp, _vp, _vp, Dropout, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    # per-sample token masks (MMFM_TOKEN_MASK_ROWS)
    "mmfm_mask_prep_rows": (C.c_int, [_i, _i, C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64), _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp]),
    "mmfm_stitch_fwd_rows": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mmfm_stitch_bwd_rows": (C.c_int, [_i, _vp, _vp, _vp, _vp, _i, _vp, Dropout, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "mmfm_layernorm_fwd_seg": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _i, C.POINTER(C.c_int32), _vp]),
    "mmfm_layernorm_bwd_seg": (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i, C.POINTER(C.c_int32), _vp, _i64, _vp]),
    "mmfm_masked_loss_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_masked_loss_fwd": (C.c_int, [_i, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _i64, _vp]),
    "mmfm_masked_loss_kind_fwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _i64, _vp]),
    "mmfm_loss_finalize": (C.c_int, [_vp, _vp, _i, _vp, _vp, _vp]),
    "mmfm_masked_loss_bwd": (C.c_int, [_i, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp]),
    "mmfm_masked_loss_kind_bwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp]),
    # per-element masks: base pointer + (sb, st, sn) element strides (MMFM_LOSS_ELEM)
    "mmfm_masked_loss_elem_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_masked_loss_elem_fwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    "mmfm_masked_loss_elem_bwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mmfm_stage_masked": (C.c_int, [_i, _vp, _vp, _i64, _i64, _i64, _i, _i, _i, _vp, _i, _vp]),
    # row mask x channel mask (MMFM_LOSS_CHAN)
    "mmfm_masked_loss_chan_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_masked_loss_chan_fwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _i, _vp, _vp, _vp, _i64, _vp]),
    "mmfm_masked_loss_chan_bwd": (C.c_int, [_i, _i, _f, _i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    # softmax cross-entropy and the arg-max confusion matrix (MMFM_SOFTMAX_CE)
    "mmfm_softmax_ce_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_softmax_ce_fwd": (C.c_int, [_i, _vp, _vp, _vp, _f, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _i64, _vp]),
    "mmfm_softmax_ce_bwd": (C.c_int, [_i, _vp, _vp, _vp, _f, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    "mmfm_argmax_confusion": (C.c_int, [_i, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _vp]),
    "mmfm_dropout_apply": (C.c_int, [_i, _vp, _vp, _i64, _i, Dropout, _vp]),
    "mmfm_cast_f32_to_bf16": (C.c_int, [_vp, _vp, _i64, _vp]),
    "mmfm_adamw_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "mmfm_optim_ranges_chunks": (C.c_int64, [C.POINTER(OptimRange), _i, _i64, _i]),
    "mmfm_optim_ranges_table_bytes": (C.c_int64, [_i64, _i]),
    "mmfm_optim_ranges_table": (C.c_int, [C.POINTER(OptimRange), _i, _i64, _i, _vp, _i64]),
    "mmfm_optim_ranges_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_grad_sumsq_ranges": (C.c_int, [_vp, _i64, C.POINTER(OptimRange), _i, _vp, _i64, _f, _f, _i, _vp, _i64, _vp]),
    "mmfm_adamw_step_ranges": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(OptimRange), _i, _vp, _i64, _vp, _i, _vp, _i, _vp]),
    "mmfm_grad_accumulate": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i, _vp]),
    # per-session linear layers (MMFM_SESSION_LINEAR)
    "mmfm_session_reduce": (C.c_int, [C.POINTER(SessionDesc), _vp, _vp, _vp]),
    "mmfm_session_expand": (C.c_int, [C.POINTER(SessionDesc), _vp, _vp, _vp]),
    "mmfm_session_dw_chunks": (C.c_int, [_i, _i, _i]),
    "mmfm_session_runs_ints": (C.c_int64, [_i, _i, _i]),
    "mmfm_session_dw_workspace": (C.c_int64, [_i, _i, _i, _i, _i]),
    "mmfm_session_dw": (C.c_int, [C.POINTER(SessionDesc), _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i64, _vp]),
    # span packing for the sparse session all-reduce (MMFM_SPAN_PACK)
    "mmfm_span_gather": (C.c_int, [_vp, _vp, _vp, _i, _vp]),
    "mmfm_span_scatter": (C.c_int, [_vp, _vp, _vp, _i, _vp]),
    "mmfm_prep_weights": (C.c_int, [_vp, _i, _i, _vp]),
    "mmfm_rowgemm": (C.c_int, [C.POINTER(RowGemmDesc), _vp]),
    "mmfm_rowgemm_groups": (C.c_int, [C.POINTER(RowGemmGroupsDesc), _vp]),
    "mmfm_rowgemm_lnbwd_form": (C.c_int, [_i64, _i]),
    "mmfm_mlp_fwd": (C.c_int, [C.POINTER(MlpDesc), _vp]),
    "mmfm_mlp_bwd": (C.c_int, [C.POINTER(MlpDesc), _vp]),
    "mmfm_ln_linear_grad_workspace": (C.c_int64, [_i]),
    "mmfm_ln_linear_grad": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp]),
    "mmfm_sn_linear_grad": (C.c_int, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i64, _vp]),
    "mmfm_r2_series": (C.c_int, [_vp, C.POINTER(_i64), _vp, C.POINTER(_i64), _i, _i, _i, _vp, _vp]),
    "mmfm_bits_per_spike_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_bits_per_spike": (C.c_int, [_vp, _vp, _i64, _i, _vp, _vp, _i64, _vp]),
    "mmfm_bits_per_spike_neurons_workspace": (C.c_int64, [_i64, _i]),
    "mmfm_bits_per_spike_neurons": (C.c_int, [_vp, _vp, _i64, _i, _vp, _vp, _i64, _vp]),
    "mmfm_mt19937_jump": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_uint64]),
    "mmfm_mt19937_jump_reset": (C.c_int, []),
    # MT19937 on the device (MMFM_MT_DEVICE)
    "mmfm_mt_plan": (C.c_int, [C.c_uint64, _i, C.POINTER(C.c_int32), C.POINTER(_i64)]),
    "mmfm_mt_workspace": (C.c_int64, [C.c_uint64, _i]),
    "mmfm_mt_uniform": (C.c_int, [_vp, C.c_int32, C.c_uint64, C.c_uint64, _vp, _i, _vp, _i64, _vp]),
    "mmfm_mt_bernoulli": (C.c_int, [_vp, C.c_int32, C.c_uint64, C.c_uint64, _f, _vp, _i, _vp, _i64, _vp]),
    "mmfm_mt_corrupt": (C.c_int, [_vp, C.c_int32, _i, _i, _i, _vp, _vp, _i64, _i64, _i64, _f, _f, _vp, _i, _vp, _i64, _vp]),
}

_lib = None


def header_symbols():
    """Every function the C header declares (used by the CPU export test)."""
    with open(HEADER_PATH) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmfm_[a-z0-9_]+)\s*\(", src)))


def lib():
    """The loaded library with typed prototypes.  Raises ImportError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension is not built and there is no CPU "
                              "fallback.  Run `python -c 'import __graft_entry__ as g; g.build()'`.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise MmfmError(f"{what} failed (code {rc}): {lib().mmfm_last_error().decode(errors='replace')}")
