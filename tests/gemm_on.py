"""For kernel tests that name their GEMM kernel: launch a descriptor after asserting the family the library routes that very descriptor
to (mmfm_gemm_family), so that a test "on the 256-tile kernel" fails when a gate moves instead of passing on another kernel."""
import ctypes as C

from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops


def gemm_on(family, A, B, Cout, M, N, K, *, live=None, **kw):
    """ops.gemm - with `live`, ops.gemm_live - of one descriptor, asserted to run on `family` (L.GEMM_FAMILY_*) first."""
    d = ops.gemm_desc(A, B, Cout, M, N, K, **kw)
    got = ops.gemm_family(d, live)
    assert got == family, f"[{M}, {N}, {K}] runs on GEMM family {got}, the test is about family {family}"
    if live is None:
        ops.run_plan([(L.lib().mmfm_gemm, (C.byref(d),), (d,))])
    else:
        ops.run_plan([(L.lib().mmfm_gemm_live, (C.byref(d), C.byref(live)), (d, live))])
