"""embedder.act / pos / bias, per kernel on the MI355X against torch fp64: the embedder act codes 12 .. 25 of mmfm_gemm at every epilogue
site, mmfm_stitch_fwd / _bwd without a position table, and a bias-free token_embed (forward, dX, dW without colsum)."""
import math

import pytest
import torch

from embedder_opts import close, close_bf16
from gemm_on import gemm_on
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K

pytestmark = pytest.mark.gpu
K_TANH = (2.0 / math.pi) ** 0.5
ACTS = ["identity", "relu", "gelu", "silu", "quick_gelu", "gelu_new", "tanh"]
SCALES = (1.0, 0.7, 16.0)


def f_ref(name, u):
    if name == "identity":
        return u.clone()
    if name == "relu":
        return torch.relu(u)
    if name == "gelu":
        return torch.nn.functional.gelu(u)
    if name in ("silu", "quick_gelu"):
        return u * torch.sigmoid((1.702 if name == "quick_gelu" else 1.0) * u)
    if name == "gelu_new":
        return 0.5 * u * (1 + torch.tanh(K_TANH * (u + 0.044715 * u ** 3)))
    return torch.tanh(u)


def df_ref(name, u):
    u = u.double().clone().requires_grad_(True)
    f_ref(name, u).backward(torch.ones_like(u))
    return u.grad


def counts(M, Kd, ld, dt, seed):
    """Integer spike counts in [0, 20], rows padded with zeros to `ld` columns (the engine's 16-B aligned input rows)."""
    x = torch.zeros(M, ld)
    x[:, :Kd] = torch.randint(0, 21, (M, Kd), generator=torch.Generator().manual_seed(seed)).float()
    return x.to(dt).cuda()


def dyadic(gen, shape, scale, dt, q=64):
    """randn * scale rounded to multiples of 1 / q (a few significant bits: exact in bf16 too).  With count-valued inputs every product and
    every partial sum of the GEMM is then exact in fp32 whatever the order of the reduction, so what a comparison shows is the epilogue."""
    return (torch.round(torch.randn(*shape, generator=gen) * scale * q) / q).to(dt).cuda()


# (mode, M, N, K, ld of the input rows): what selects each epilogue site (csrc/gemm.hip, gemm_bf16.hip, gemm_big.hip)
SITES = [
    ("fp32", 70, 24, 12, 16),        # the scalar epilogue of gemm.hip at the tiny tokeniser's ragged shape
    ("fp32", 70, 4, 2, 8),           # ... the behaviour path
    ("fp32", 300, 264, 64, 64),      # ... 3 x 3 tiles
    ("bf16", 70, 24, 12, 16),        # gemm_bf16.hip's 8-wide vector epilogue, 16-B rows
    ("bf16", 70, 4, 2, 8),           # ... its 4-column half mode (N % 8 == 4): the behaviour path
    ("bf16", 70, 6, 12, 16),         # ... its scalar-edge epilogue (N % 4 != 0)
    ("bf16", 300, 264, 64, 64),      # ... 3 x 3 tiles
    ("big", 1024, 128, 512, 512),    # the 256-tile kernel: the smallest shape mmfm_gemm_big_takes accepts (M >= 1024, N >= 128, K >= 512)
]
FAMILY = {"fp32": L.GEMM_FAMILY_F32, "bf16": L.GEMM_FAMILY_TILE128, "big": L.GEMM_FAMILY_BIG256}      # asserted of every launch (gemm_on)


@pytest.mark.parametrize("site", SITES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}x{s[3]}")
@pytest.mark.parametrize("name", ACTS)
def test_gemm_embedder_act_codes(monkeypatch, site, name):
    """forward: C = f(x W^T + b) * act_scale with the pre-activation stored through pre_out; gradient: C = (dY Wg^T) * f'(u) * act_scale with
    u = the stored pre-activation (identity: no gradmul_pre).  Count-valued inputs, act_scale in {1, 0.7, 16}; weights, bias and dY are
    small dyadic rationals (`dyadic`): x W^T + b and dY Wg^T are exact in fp32, so the fp32 bounds - made for unit-scale data - test the
    epilogue at pre-activations of tens and outputs of hundreds, not the rounding of a reduction over count-sized terms."""
    mode, M, N, Kd, ld = site
    fwd, grad = K.EMBED_ACTS[name]
    if mode == "big":
        monkeypatch.setenv("MMFM_GEMM_BIG_MIN_TILES", "1")
    code, dt = (L.F32, torch.float32) if mode == "fp32" else (L.BF16, torch.bfloat16)
    chk = (lambda a, b, msg: close(a, b, msg=msg)) if mode == "fp32" else close_bf16
    gen = torch.Generator().manual_seed(5)
    q = 256 if Kd > 64 else 64
    x = counts(M, Kd, ld, dt, seed=1)
    W = dyadic(gen, (N, Kd), Kd ** -0.5, dt, q)
    bias = dyadic(gen, (N,), 1.0, torch.float32)
    z = x[:, :Kd].double() @ W.double().t() + bias.double()
    dY, Wg = dyadic(gen, (M, Kd), 0.3, dt, 16), dyadic(gen, (N, Kd), 0.2, dt, 16)
    g0 = dY.double() @ Wg.double().t()
    assert torch.equal(z.float().double(), z) and torch.equal(g0.float().double(), g0)         # both products are exact in fp32
    for s in SCALES:
        what = f"{name} scale {s} {mode} {M}x{N}x{Kd}"
        C = torch.full((M + 1, N), 9.0, dtype=dt, device="cuda")
        pre = torch.empty(M, N, dtype=dt, device="cuda")
        gemm_on(FAMILY[mode], x, W, C, M, N, Kd, lda=ld, ldb=Kd, ldc=N, bias=bias, pre_out=pre, act=fwd, act_scale=s, dtype=code)
        assert torch.all(C[M:] == 9.0), "rows beyond M written"
        assert torch.isfinite(C.float()).all()
        chk(pre, z, what + " pre-activation")
        chk(C[:M], f_ref(name, z) * s, what + " forward")
        u = None if name == "identity" else pre
        D = torch.empty(M, N, dtype=dt, device="cuda")
        gemm_on(FAMILY[mode], dY, Wg, D, M, N, Kd, lda=Kd, ldb=Kd, ldc=N, act=grad, act_scale=s, gradmul_pre=u, dtype=code)
        assert torch.isfinite(D.float()).all()
        chk(D, g0 * df_ref(name, pre.double()) * s, what + " gradient")


def test_gemm_embedder_act_argument_checks():
    x, W, C = (torch.zeros(8, 8, device="cuda") for _ in range(3))
    with pytest.raises(L.MmfmError, match="needs gradmul_pre"):
        K.gemm(x, W, C, 8, 8, 8, lda=8, ldb=8, ldc=8, act=L.ACT_EMB_TANH_GRAD)
    with pytest.raises(L.MmfmError, match="gradient act"):
        K.gemm(x, W, C, 8, 8, 8, lda=8, ldb=8, ldc=8, act=L.ACT_EMB_TANH, gradmul_pre=x)
    with pytest.raises(L.MmfmError, match="bad act"):
        K.gemm(x, W, C, 8, 8, 8, lda=8, ldb=8, ldc=8, act=26)
    K.gemm(x, W, C, 8, 8, 8, lda=8, ldb=8, ldc=8, act=L.ACT_EMB_IDENTITY_GRAD, act_scale=2.0)      # reads no pre-activation


# ---------------------------------------------------------------------------------------------- stitch without a position table
@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stitch_fwd_null_table(dt, H):
    """pos_emb NULL: emb is the modality row, broadcast, exactly; x = keep0 * tok + row.  With a table: (row + pos[ts]) + keep0 * tok, the
    fp32 operations of the kernel in its order, so bit for bit (bf16: after the one rounding of the store)."""
    B, T, M, max_F = 3, 8, 2, 9
    Lq = M * T
    g = torch.Generator().manual_seed(3)
    ts = torch.randint(0, max_F, (B, T), generator=g).cuda()
    keep0 = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1] + [0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8).cuda()
    for table in (False, True):
        x, emb = torch.zeros(B, Lq, H, device="cuda", dtype=dt), torch.zeros(B, Lq, H, device="cuda", dtype=dt)
        want_x, want_e = [], []
        for m in range(M):
            tok = torch.randn(B * T, H, generator=g).to(dt).cuda()
            row = torch.randn(H, generator=g).cuda()
            pos = torch.randn(max_F, H, generator=g).cuda()
            K.stitch_fwd(tok, row, pos if table else None, ts if (table or m == 0) else None, keep0, x, emb, B, T, Lq, m, H, max_F)
            e = (row[None, None, :] + pos[ts]) if table else row[None, None, :].expand(B, T, H)
            want_e.append(e.to(dt))
            want_x.append((e + tok.float().view(B, T, H) * keep0[m * T:(m + 1) * T, None].float()).to(dt))
            # (x = e where keep0 is 0: the kernel does not add there; adding 0 * tok gives the same bits for finite tok)
        assert torch.equal(emb, torch.cat(want_e, 1)), f"emb table={table}"
        assert torch.equal(x, torch.cat(want_x, 1)), f"x table={table}"


@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_stitch_bwd_null_table(dt, H):
    """d_pos NULL: d_tok = keep0 * dx exactly, d_mod_row = sum over (b, t) of dx + dextra within the bounds of test_stitch_fwd_bwd (fp32:
    atol 1e-4) / test_stitch_bwd_bf16_onehot_gemm (bf16: rtol 1e-5, atol 1e-4 sqrt(B T)); two launches give the same bits; acc_mod adds.
    With a table the outputs keep those bounds, d_tok stays exact, and in fp32 mode d_mod_row has the bits of the table-free launch (the
    same chunks in the same order)."""
    B, T, M, max_F = 3, 8, 2, 9
    Lq = M * T
    g = torch.Generator().manual_seed(4)
    ts = torch.randint(0, max_F, (B, T), generator=g).cuda()
    keep0 = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1] + [0, 1, 1, 1, 1, 0, 1, 1], dtype=torch.uint8).cuda()
    dx, dextra = torch.randn(B, Lq, H, generator=g).to(dt).cuda(), torch.randn(B, Lq, H, generator=g).to(dt).cuda()
    ws = torch.empty(L.lib().mmfm_stitch_bwd_workspace(K.dt(dx), B, T, Lq, H, max_F), dtype=torch.uint8, device="cuda")
    tol = dict(atol=1e-4) if dt == torch.float32 else dict(rtol=1e-5, atol=1e-4 * math.sqrt(B * T))
    for m in range(M):
        for extra in (dextra, None):
            what = f"m={m} dextra={extra is not None}"
            e = dx[:, m * T:(m + 1) * T].double() + (extra[:, m * T:(m + 1) * T].double() if extra is not None else 0)
            tok_ref = (dx[:, m * T:(m + 1) * T].float() * keep0[m * T:(m + 1) * T, None].float()).reshape(B * T, H).to(dt)
            runs = []
            for _ in range(2):
                d_tok = torch.full((B * T, H), float("nan"), device="cuda", dtype=dt)
                d_mod = torch.full((H,), float("nan"), device="cuda")
                K.stitch_bwd(dx, extra, None, keep0, None, d_tok, d_mod, None, False, False, B, T, Lq, m, H, max_F, ws)
                runs.append((d_tok, d_mod))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what + ": two launches differ"
            d_tok, d_mod = runs[0]
            assert torch.equal(d_tok, tok_ref), what + " d_tok"
            close(d_mod, e.sum((0, 1)), msg=what + " d_mod", **tol)
            acc = d_mod.clone()
            K.stitch_bwd(dx, extra, ts, keep0, None, None, acc, None, True, False, B, T, Lq, m, H, max_F, ws)        # ts passed, not read
            close(acc, 2 * e.sum((0, 1)), msg=what + " d_mod accumulated", rtol=tol.get("rtol", 2e-5), atol=2 * tol["atol"])
            # with a table
            d_tok2 = torch.full((B * T, H), float("nan"), device="cuda", dtype=dt)
            d_mod2, d_pos = torch.full((H,), float("nan"), device="cuda"), torch.full((max_F, H), float("nan"), device="cuda")
            K.stitch_bwd(dx, extra, ts, keep0, None, d_tok2, d_mod2, d_pos, False, False, B, T, Lq, m, H, max_F, ws)
            ref_pos = torch.zeros(max_F, H, dtype=torch.float64, device="cuda").index_add_(0, ts.reshape(-1), e.reshape(B * T, H))
            assert torch.equal(d_tok2, tok_ref), what + " d_tok (table)"
            close(d_mod2, e.sum((0, 1)), msg=what + " d_mod (table)", **tol)
            close(d_pos, ref_pos, msg=what + " d_pos (table)", **tol)
            if dt == torch.float32:
                assert torch.equal(d_mod2, d_mod), what + ": d_mod with and without a table"


# ---------------------------------------------------------------------------------------------- bias-free token_embed
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,Kd", [(70, 24, 12), (333, 1336, 668)], ids=["tiny", "K668"])
def test_bias_free_token_embed(mode, M, N, Kd):
    """token_embed = nn.Linear(bias=False) on the NULL-bias contract of mmfm_gemm at the tokeniser's ragged shapes (input rows padded to
    16 B): forward with an embedder activation, dX, and the weight gradient dW = dY^T X launched without colsum, as the plan does.
    Operands as in test_gemm_embedder_act_codes (counts and dyadic rationals: the three products are exact in fp32)."""
    code, dt = (L.F32, torch.float32) if mode == "fp32" else (L.BF16, torch.bfloat16)
    chk = (lambda a, b, msg: close(a, b, msg=msg)) if mode == "fp32" else close_bf16
    ld = (Kd + 7) // 8 * 8
    gen = torch.Generator().manual_seed(7)
    x = counts(M, Kd, ld, dt, seed=2)
    W = dyadic(gen, (N, Kd), Kd ** -0.5, dt, 256 if Kd > 64 else 64)
    z = x[:, :Kd].double() @ W.double().t()
    C, pre = torch.empty(M, N, dtype=dt, device="cuda"), torch.empty(M, N, dtype=dt, device="cuda")
    K.gemm(x, W, C, M, N, Kd, lda=ld, ldb=Kd, ldc=N, bias=None, pre_out=pre, act=L.ACT_EMB_TANH, act_scale=0.7, dtype=code)
    chk(pre, z, "pre-activation")
    chk(C, torch.tanh(z) * 0.7, "forward")
    dY = dyadic(gen, (M, N), 0.3, dt, 16)
    dX = torch.empty(M, Kd, dtype=dt, device="cuda")
    K.gemm(dY, W, dX, M, Kd, N, lda=N, ldb=Kd, ldc=Kd, b_kcontig=0, dtype=code)
    chk(dX, dY.double() @ W.double(), "dX")
    dW = torch.full((N * Kd + 8,), float("nan"), device="cuda")
    K.gemm(dY, x, dW, N, Kd, M, lda=N, ldb=ld, ldc=Kd, a_kcontig=0, b_kcontig=0, dtype=code, c_f32=1, colsum=None)
    ref = dY.double().t() @ x[:, :Kd].double()
    chk(dW[:N * Kd].view(N, Kd), ref, "dW")
    assert torch.isnan(dW[N * Kd:]).all(), "written behind the weight gradient"
