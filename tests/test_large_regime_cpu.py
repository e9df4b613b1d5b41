"""tests/large_regime.py without a GPU: B_BIG stands on the B = 1024 side of every size gate of the step plan and is the smallest batch
that does; the gates `host_gates` restates agree with the product's own functions wherever those run on the host (plan.live_rows_on /
ctx_group_on, Engine._fused_mask and Engine._dw_split on a stand-in engine, the library's mmfm_colsum_workspace and mmfm_gemm_dw_tiles);
and the per-descriptor rules give the kernels DESIGN.md names for the shapes of the default model."""
import types

import pytest

import large_regime as LR
from helpers import model_config
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import plan as P
from multi_modal_foundation_model_amd.engine import Engine, EngineConfig

SW = P.Switches(fused=None, gemm_big=True, gemm_dw=True, batch_reduce=True, dw_pair=True, attn_keepbits=True, mlp_bwd_split=True)


def test_b_big_and_the_benchmark_batch_are_on_the_large_side_of_every_gate():
    for B in (LR.B_BIG, LR.B_BENCH):
        gates = LR.host_gates(B)
        assert len(gates) == 11 and all(gates.values()), (B, gates)


def test_b_big_is_minimal():
    """Every smaller batch is on the small side of at least one gate.  Below 328 (R = 65,400 <= 65,536 rows, B T = 32,700 < 32,768 tokeniser
    rows) of the two last thresholds; from 328 to B_BIG - 1 every threshold is crossed and the cross-attention out_proj + query weight
    gradients, which pair into one launch at 1024, leave one after the other."""
    assert {g for g, on in LR.host_gates(327).items() if not on} == {"dw_wide_tiles", "second_row_pass_everywhere"}
    for B in range(328, LR.B_BIG):
        assert {g for g, on in LR.host_gates(B).items() if not on} == {"dw_pairs_one_launch"}, B
        a, b = LR.pair_descs(*LR.DW_PAIRS[2], B * LR.MODS * LR.T)
        assert (2 * a.splits) % 8 and not LR.pair_one_launch(a, b), B             # 2 tiles x an odd or singly even slab count
    for B in range(1, LR.B_BIG):
        assert not all(LR.host_gates(B).values()), B
    assert LR.B_BIG == 343 and [d.splits for a, b in LR.DW_PAIRS for d in LR.pair_descs(a, b, LR.B_BIG * 200)] == [32, 32, 40, 29, 64, 64]
    assert [d.splits for a, b in LR.DW_PAIRS for d in LR.pair_descs(a, b, LR.B_BENCH * 200)] == [32, 32, 40, 29, 64, 64]
    assert [d.splits for d in LR.pair_descs(*LR.DW_PAIRS[2], 328 * 200)] == [61, 61]        # 64 asked for, slabs of 1,088 rows: 61


def test_the_signature_rows_of_the_regime_are_at_b_big():
    import plan_sig as S
    rows = {c["name"]: c for c in S.CASES}
    big = [n for n in rows if n.endswith("_B343")]
    assert len(big) == 4 and all(rows[n]["B"] == LR.B_BIG and rows[n]["T"] == LR.T and not rows[n]["env"] for n in big)
    assert rows["default_B1024"]["B"] == LR.B_BENCH and not rows["default_B1024"]["env"]
    assert not set(S.AUTO) & set(S.SWITCHES)


def test_every_gate_flips_where_the_table_says():
    """First batch on the large side of each gate (T = 100, two modalities): the table of DESIGN.md §6."""
    first = {}
    for B in range(1, LR.B_BIG + 1):
        for g, on in LR.host_gates(B).items():
            if on and g != "dw_pairs_one_launch":          # no threshold: see test_b_big_is_minimal
                first.setdefault(g, B)
    assert first == {"fused_mask_15": 62, "batch_red_off_pairing_on": 41, "dw_split_large_branch": 82, "ctx_group": 82, "live_rows": 164,
                     "rowgemm_column_blocks_off": 82, "dw_wide_tiles": 328, "gemm_big_rows": 244, "reduce_large_branch": 82,
                     "second_row_pass_everywhere": 328}


def test_host_gates_against_the_products_own_functions(monkeypatch):
    for k in ("MMFM_LIVE_ROWS", "MMFM_CTX_GROUP", "MMFM_FUSED"):
        monkeypatch.delenv(k, raising=False)
    cfg = EngineConfig.from_model_config(model_config(), [("ap", LR.N_AP), ("behavior", LR.N_BEH)])
    bf16 = types.SimpleNamespace(cfg=cfg, dtype="bf16", code=L.BF16)
    fp32 = types.SimpleNamespace(cfg=cfg, dtype="fp32", code=L.F32)
    lib = L.lib()
    for B in (16, 40, 41, 61, 62, 81, 82, 163, 164, 243, 244, LR.B_BIG - 1, LR.B_BIG, LR.B_BENCH):
        R, BT = B * LR.MODS * LR.T, B * LR.T
        g = LR.host_gates(B)
        assert g["fused_mask_15"] == (Engine._fused_mask(bf16, R, SW) == 15)
        assert g["ctx_group"] == P.ctx_group_on(R) and g["live_rows"] == P.live_rows_on(BT)
        # Engine._dw_split on the 128-tile kernel's shapes (fp32: no streaming): 66 tiles -> at most 768 // 66 = 11 slabs beyond 8,192 rows,
        # min(rows // 256, 15) up to there
        for rows in (R, BT):
            S, kchunk = Engine._dw_split(fp32, 1336, 668, rows, sw=SW)
            want = max(1, min(rows // 256, 15)) if rows <= 8192 else min(rows // 512, 11)
            assert kchunk % 64 == 0 and S == LR.cdiv(rows, kchunk) and kchunk == LR.cdiv(LR.cdiv(rows, want), 64) * 64, (B, rows, S, kchunk)
        assert g["dw_split_large_branch"] == (min(R, BT) > 8192) == g["reduce_large_branch"]
        for rows in (R, BT):
            S = lib.mmfm_colsum_workspace(rows, 1) // 4
            assert S == (min(256, rows // 64) if LR.colsum_gates(rows, 256)["large_branch"] else max(1, min(15, rows // 256)))
        # the streaming kernel's tiles of a [128, 256] gradient: one 256-wide tile from 32,768 rows, two 128-wide ones below
        assert g["dw_wide_tiles"] == all(lib.mmfm_gemm_dw_tiles(128, 256, rows) == 1 for rows in (R, BT))
        assert lib.mmfm_gemm_dw_tiles(256, 128, R) == 2          # N <= 128: never wide
    for rows, S in ((8192, 15), (8193, 128)):
        assert lib.mmfm_colsum_workspace(rows, 1) // 4 == S
    assert Engine._fused_mask(bf16, 12287, SW) == 11 and Engine._fused_mask(bf16, 12288, SW) == 15
    assert (lib.mmfm_gemm_dw_tiles(128, 256, 32767), lib.mmfm_gemm_dw_tiles(128, 256, 32768)) == (2, 1)


@pytest.mark.parametrize("B,wide", [(327, False), (328, True), (LR.B_BIG, True), (LR.B_BENCH, True)])
def test_descriptor_rules_on_the_default_models_shapes(B, wide):
    R, BT = B * LR.MODS * LR.T, B * LR.T
    # slabs long enough for the fewest splits below (29) to cover R rows: the library checks the descriptors it is asked about
    dw = dict(a_kcontig=0, b_kcontig=0, c_f32=1, splits=32, kchunk=LR.cdiv(LR.cdiv(R, 29), 64) * 64)
    # dW of qkv [768, 256] over R rows and of the ap token embedding [1336, 668] over B T rows (input rows padded to 672)
    qkv = LR.gemm_desc(M=768, N=256, K=R, lda=768, ldb=256, ldc=256, **dw)
    tok = LR.gemm_desc(M=1336, N=668, K=BT, lda=1336, ldb=672, ldc=668, **dw)
    assert LR.gemm_kernel(qkv) == "dw256" and LR.gemm_kernel(tok) == ("dw256" if wide else "dw128")
    # the ap head's gradient [668, 256]: dY rows of 668 bf16 are not 16-byte aligned -> the general kernel; fp32 -> its own
    assert LR.gemm_kernel(LR.gemm_desc(M=668, N=256, K=BT, lda=668, ldb=256, ldc=256, **dw)) == "tile128"
    assert LR.gemm_kernel(LR.gemm_desc(dtype=L.F32, M=768, N=256, K=R, lda=768, ldb=256, ldc=256, **dw)) == "f32"
    # forward products: K = 256 and the tokeniser's K = 668 / 1336 (no multiple of 64) stay off the 256-tile kernel, K = 512 rides it
    fwd = lambda N, K, **kw: LR.gemm_desc(M=BT, N=N, K=K, lda=K, ldb=K, ldc=N, **kw)
    assert [LR.gemm_kernel(fwd(*nk)) for nk in ((668, 256), (1336, 668), (256, 1336))] == ["tile128"] * 3
    assert LR.gemm_kernel(fwd(256, 512)) == "big" and LR.gemm_kernel(LR.gemm_desc(M=1000, N=256, K=512, lda=512, ldb=512, ldc=256)) == "tile128"
    # out_proj [256, 256] + qkv [768, 256] as a pair: 2 x 40 + 6 x 29 items (plan.PlanBuilder.pair_splits at 256-wide tiles)
    a = LR.gemm_desc(M=256, N=256, K=R, lda=256, ldb=256, ldc=256, **dict(dw, splits=40))
    b = LR.gemm_desc(M=768, N=256, K=R, lda=768, ldb=256, ldc=256, **dict(dw, splits=29))
    assert LR.pair_one_launch(a, b) and not LR.pair_one_launch(a, tok if not wide else LR.gemm_desc(M=768, N=128, K=R, lda=768, ldb=128, ldc=128, **dw))
    assert not LR.pair_one_launch(LR.gemm_desc(M=256, N=256, K=R, lda=256, ldb=256, ldc=256, **dict(dw, splits=41)), b)       # 82 items: no multiple of 8


def test_reduction_and_row_pass_rules():
    # 64 slabs of the [256, 4] behavior projection gradient (+ bias): 5 chunks -> 16 groups of 4 first; of a [256, 256] one: 257 chunks,
    # 512 // 257 = 1 group -> one stage; the [1336, 668] one has 3,492 chunks -> one stage
    assert LR.two_stage(1280, 64, 1280) and not LR.two_stage(256 * 256 + 256, 64, 256 * 256 + 256)
    assert not LR.two_stage(1336 * 668 + 1336, 64, 1336 * 668 + 1336) and LR.two_stage(256 * 256 + 256, 64, 256 * 256 + 256) is False
    assert not LR.two_stage(65792, 15, 65792) and not LR.two_stage(10, 64, 10)          # < 16 slabs; n % 4: the scalar kernel
    rg = lambda R, **kw: types.SimpleNamespace(**dict(dict(R=R, K=256, N=768, ln=1, ln_bwd=0, residual=None, groups=1), **kw))
    mlp = lambda R, dx: types.SimpleNamespace(R=R, dx=dx)
    for R, blocks, second_fwd, second_one_per_cu in ((3200, True, False, False), (16256, True, False, False), (16257, False, False, False),
                                                     (32769, False, False, True), (65536, False, False, True), (65537, False, True, True)):
        g = LR.rowowner_gates("mmfm_rowgemm", rg(R))
        assert (g["column_blocks"], g["second_pass"]) == (blocks, second_fwd), R
        assert LR.rowowner_gates("mmfm_rowgemm", rg(R, K=512, N=256, ln=0, ln_bwd=1))["second_pass"] == second_one_per_cu, R
        assert LR.rowowner_gates("mmfm_mlp_fwd", mlp(R, None))["second_pass"] == second_one_per_cu, R
        assert LR.rowowner_gates("mmfm_mlp_bwd", mlp(R, None))["second_pass"] == second_fwd, R           # front half: 256-row passes
        assert LR.rowowner_gates("mmfm_mlp_bwd", mlp(R, 1))["second_pass"] == second_one_per_cu, R
    # LayerNorm + residual in one launch stays on the register-staged ring: no column blocks at any size; out_proj + residual: four or none
    assert not LR.rowowner_gates("mmfm_rowgemm", rg(3200, N=256, residual=1))["column_blocks"]
    assert LR.rowowner_gates("mmfm_rowgemm", rg(3200, N=256, ln=0, residual=1))["column_blocks"]
    assert not LR.rowowner_gates("mmfm_rowgemm", rg(16500, N=256, ln=0, residual=1))["column_blocks"]
