"""Shared by tests/test_embedder_opts_*.py: model configs with `embedder.act`, `pos` and `bias` set, built from the switches
tests/golden/embedder_opts_fwd_bwd.npz records (scripts/make_embedder_goldens.py: case -> side -> section -> keys)."""
from conftest import load_npz
from helpers import tiny_config
from side_config import with_sides

CASES = ("IDENTITY", "RELU", "GELU", "SILU", "QUICK_GELU", "GELU_NEW", "TANH", "POS_OFF", "BIAS_OFF", "POS_BIAS_OFF", "ASYM", "SCALE")
OBJECTIVES = ("encoding", "decoding", "token_masking")
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("embedder_opts_fwd_bwd.npz")
    return _Z


def case_config(case, **kw):
    return with_sides(tiny_config(**kw), fixture()[1]["switches"][case])


# ---- the bounds tests/test_kernels_gpu.py applies to the mmfm_gemm epilogues (copied: a test module is not imported from another)
def close(a, b, rtol=2e-5, atol=2e-5, msg=""):
    import torch
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{msg}: max abs err {err:.3e} (ref max {ref:.3e})"


def close_bf16(a, b, msg, tol=1.5e-2):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * scale, f"{msg}: max abs err {err:.3e} vs scale {scale:.3e}"
