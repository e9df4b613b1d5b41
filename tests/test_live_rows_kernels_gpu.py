"""Live rows (include/mmfm.h), kernel by kernel: mmfm_live_bins against edge_refs.mask_prep's keep0, and every live
product form of mmfm_gemm_live against the plain mmfm_gemm run on host-gathered operands.

x.W^T (+ activation + dropout) and dY.W (+ gradmul_pre): the live rows bit for bit, the rows of the output beyond B * T_live untouched
(sentinel), the dropout decisions those of the full-row launch gathered afterwards.  dY^T.X + colsum (streaming kernel at 256 x 64, the
generic split-K kernel at 4 x 2): bit for bit with every bin live, exact zeros with none, and with some bins dead - the split ranges
then differ from the plain launch's, so only the grouping of the fp32 sums does - both launches against the fp64 product of the same
bf16 operands at edge_refs.check_sum's bound: K_live terms per element."""
import pytest
import torch

import edge_refs as ER
from gemm_on import gemm_on
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 7.0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def record(T, live):
    """keep0 u8 [T] with the bins of `live` kept, and its record off the kernel."""
    keep0 = torch.zeros(T, dtype=torch.uint8)
    keep0[list(live)] = 1
    keep0 = keep0.cuda()
    rec = torch.full((L.live_rec_ints(T),), -9, dtype=torch.int32, device="cuda")
    K.live_bins(keep0, T, 1, rec)
    torch.cuda.synchronize()
    return keep0, rec


def live_index(B, T, live):
    """Original rows of the compact rows, in order: b * T + live_t[j]."""
    lt = torch.tensor(sorted(live), dtype=torch.int64)
    return (torch.arange(B)[:, None] * T + lt[None, :]).reshape(-1).cuda()


# ---------------------------------------------------------------------------------------------- the record
@pytest.mark.parametrize("T", [7, 64, 100, 130])
def test_live_bins_against_mask_prep_keep0(T):
    """Two modalities; sample 0's masks differ from the other samples' (which must not matter), one padded bin in sample 0 (attn = 0:
    mask & attn = 0, so the bin is live).  T = 64 / 130: one full ballot round / a third, ragged one."""
    B, M = 3, 2
    t = torch.arange(T)
    masks = [((t % k == 1)[None] | (torch.arange(B)[:, None] > 0)).to(torch.int64).cuda() for k in (2, 3)]     # samples 1, 2: every bin masked
    masks[1][1:] = 1 - masks[1][:1]                       # ... or the opposite of sample 0
    attn = torch.ones(B, T, dtype=torch.int64).cuda()
    attn[0, T - 1] = 0
    masks[0][0, T - 1] = 1
    keep0 = ER.mask_prep(masks, [1] * M, attn, [3, 2])[2]
    assert keep0.shape == (M * T,) and int(keep0[T - 1]) == 1
    rec = torch.full((M, L.live_rec_ints(T)), -9, dtype=torch.int32, device="cuda")
    K.live_bins(keep0, T, M, rec)
    torch.cuda.synchronize()
    for m in range(M):
        k = keep0[m * T:(m + 1) * T].cpu()
        lt = torch.nonzero(k).reshape(-1).to(torch.int32)
        r = rec[m].cpu()
        assert 0 < len(lt) < T
        assert r[:4].tolist() == [len(lt), 0, 0, 0]
        assert torch.equal(r[4:4 + len(lt)], lt)
        rank = torch.full((T,), -1, dtype=torch.int32)
        rank[lt.long()] = torch.arange(len(lt), dtype=torch.int32)
        assert torch.equal(r[4 + T:4 + 2 * T], rank)


def test_gather_live_rows():
    """16-B pieces (672 bf16 a row) and 4-B pieces (6 bf16 a row); rows beyond B * T_live untouched."""
    B, T, live = 5, 7, (0, 3, 6)
    _, rec = record(T, live)
    for n in (672, 6):
        src = rnd(B * T, n, seed=n).to(BF)
        dst = torch.full((B * T, n), SENT, device="cuda", dtype=BF)
        K.gather_live_rows(src, dst, B, T, n * 2, rec)
        torch.cuda.synchronize()
        assert torch.equal(dst[:B * len(live)], src[live_index(B, T, live)]) and torch.all(dst[B * len(live):] == SENT)


# ---------------------------------------------------------------------------------------------- x.W^T and dY.W
SHAPES = [(5, 7, tuple(range(7))), (5, 7, ()), (5, 7, (0, 3, 6)), (37, 9, (1, 2, 5, 8))]       # 37 x 4 = 148 rows: past a 128-row tile, not a multiple of 32


def drop_desc(p=0.3):
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    K.rng_seed(state, 5)
    return state, K.dropout(state, 9, p)


@pytest.mark.parametrize("B,T,live", SHAPES)
@pytest.mark.parametrize("N,Kd,vec", [(64, 40, True), (36, 20, True), (6, 10, False)])
def test_forward_product_with_activation_and_dropout(B, T, live, N, Kd, vec):
    """C = dropout(softsign(x W^T + bias) * scale), N = 64 / 36 / 6: the 8-column, the 4-column and the scalar epilogue."""
    R, Rl = B * T, B * len(live)
    _, rec = record(T, live)
    idx = live_index(B, T, live)
    x, W, bias = rnd(R, Kd, seed=1).to(BF), rnd(N, Kd, seed=2, scale=0.2).to(BF), rnd(N, seed=3)
    state, drop = drop_desc()
    kw = dict(lda=Kd, ldb=Kd, ldc=N, bias=bias, act=L.ACT_SOFTSIGN, act_scale=1.5, drop=drop, dtype=L.BF16)
    full = torch.full((R, N), SENT, device="cuda", dtype=BF)
    K.gemm(x, W, full, R, N, Kd, **kw)                                   # all rows, original counters
    xg = torch.zeros(R, Kd, device="cuda", dtype=BF)
    xg[:Rl] = x[idx]
    out = torch.full((R + 1, N), SENT, device="cuda", dtype=BF)
    K.gemm_live(xg, W, out, R, N, Kd, live=K.live_rows(rec, B, T), **kw)
    torch.cuda.synchronize()
    assert torch.all(out[Rl:] == SENT), "rows beyond B * T_live were written"
    ER.check_exact(ER.bits(out[:Rl]), ER.bits(full[idx]), "live x.W^T + act + dropout vs the full-row launch, gathered")
    if Rl:
        # ... and, without dropout, against mmfm_gemm on the gathered operand
        plain, nodrop = torch.empty(Rl, N, device="cuda", dtype=BF), torch.full((R + 1, N), SENT, device="cuda", dtype=BF)
        K.gemm(xg, W, plain, Rl, N, Kd, **{**kw, "drop": None})
        K.gemm_live(xg, W, nodrop, R, N, Kd, live=K.live_rows(rec, B, T), **{**kw, "drop": None})
        torch.cuda.synchronize()
        ER.check_exact(ER.bits(nodrop[:Rl]), ER.bits(plain), "live x.W^T + act vs mmfm_gemm on gathered rows")
        dropped = (out[:Rl] == 0) & (plain != 0)
        assert 0.1 < float(dropped.double().mean()) < 0.5 and torch.all(nodrop[Rl:] == SENT)


@pytest.mark.parametrize("live", [(1, 2, 5, 8, 11, 12, 19), (), tuple(range(20))])
def test_forward_product_on_the_256_tile_kernel(monkeypatch, live):
    """K = 512, 1280 rows: the 256 x 256 kernel (csrc/gemm_big.hip; its tile-count floor lowered as in its own test).  7 live bins = 448
    rows, a full and a ragged row tile; against the full-row launch of the same kernel, gathered - dropout decisions included."""
    monkeypatch.setenv("MMFM_GEMM_BIG_MIN_TILES", "1")
    B, T, N, Kd = 64, 20, 256, 512
    R, Rl = B * T, B * len(live)
    _, rec = record(T, live)
    idx = live_index(B, T, live)
    x, W, bias = rnd(R, Kd, seed=1).to(BF), rnd(N, Kd, seed=2, scale=0.05).to(BF), rnd(N, seed=3)
    state, drop = drop_desc()
    kw = dict(lda=Kd, ldb=Kd, ldc=N, bias=bias, act=L.ACT_SOFTSIGN, act_scale=1.5, drop=drop, dtype=L.BF16)
    full = torch.full((R, N), SENT, device="cuda", dtype=BF)
    gemm_on(L.GEMM_FAMILY_BIG256, x, W, full, R, N, Kd, **kw)
    xg = torch.zeros(R, Kd, device="cuda", dtype=BF)
    xg[:Rl] = x[idx]
    out = torch.full((R + 1, N), SENT, device="cuda", dtype=BF)
    gemm_on(L.GEMM_FAMILY_BIG256, xg, W, out, R, N, Kd, live=K.live_rows(rec, B, T), **kw)
    torch.cuda.synchronize()
    assert torch.all(out[Rl:] == SENT), "rows beyond B * T_live were written"
    ER.check_exact(ER.bits(out[:Rl]), ER.bits(full[idx]), "live x.W^T on the 256-tile kernel vs the full-row launch, gathered")


@pytest.mark.parametrize("B,T,live", SHAPES)
@pytest.mark.parametrize("N,Kd", [(64, 40), (36, 24)])
def test_dx_product_with_gradmul_pre(B, T, live, N, Kd):
    """dX[R, N] = (dY[R, Kd] W[Kd, N]) * softsign'(y) * scale with y the saved activation (act 5), against mmfm_gemm on gathered rows."""
    R, Rl = B * T, B * len(live)
    _, rec = record(T, live)
    idx = live_index(B, T, live)
    dY, W = rnd(R, Kd, seed=4).to(BF), rnd(Kd, N, seed=5, scale=0.2).to(BF)
    y = (torch.tanh(rnd(R, N, seed=6)) * 1.4).to(BF)
    dYg, yg = torch.zeros_like(dY), torch.zeros_like(y)
    dYg[:Rl], yg[:Rl] = dY[idx], y[idx]
    kw = dict(lda=Kd, ldb=N, ldc=N, b_kcontig=0, act=L.ACT_SOFTSIGN_GRAD_OUT, act_scale=1.5, dtype=L.BF16)
    out = torch.full((R + 1, N), SENT, device="cuda", dtype=BF)
    K.gemm_live(dYg, W, out, R, N, Kd, live=K.live_rows(rec, B, T), gradmul_pre=yg, **kw)
    torch.cuda.synchronize()
    assert torch.all(out[Rl:] == SENT), "rows beyond B * T_live were written"
    if Rl:
        ref = torch.empty(Rl, N, device="cuda", dtype=BF)
        K.gemm(dYg, W, ref, Rl, N, Kd, gradmul_pre=yg, **kw)
        torch.cuda.synchronize()
        ER.check_exact(ER.bits(out[:Rl]), ER.bits(ref), "live dY.W + gradmul_pre vs mmfm_gemm on gathered rows")


# ---------------------------------------------------------------------------------------------- dY^T.X + colsum
def run_dw(family, dY, X, M, N, Kfull, S, kchunk, live=None):
    """[M, N] = dY^T X with the column sums of dY behind each slab, reduced: (dW, db); on kernel `family`, asserted."""
    n = M * N + M
    stride = (n + 7) // 8 * 8
    slab = torch.full((S * stride,), SENT, device="cuda")
    kw = dict(lda=M, ldb=X.shape[1], ldc=N, a_kcontig=0, b_kcontig=0, dtype=L.BF16, c_f32=1, colsum=slab.data_ptr() + 4 * M * N,
              splits=S, kchunk=kchunk, slab_stride=stride)
    gemm_on(family, dY, X, slab, M, N, Kfull, live=live, **kw)
    dst = torch.empty(n, device="cuda")
    K.reduce_slabs(dst, slab, n, S, stride)
    torch.cuda.synchronize()
    return dst[:M * N].view(M, N), dst[M * N:]


# B * T = 1600 rows in S = 8 splits of 256 (the host's rounding of 1600 / 8 = 200 up to 64).  T_live: 100 -> K_live = K;
# 0; 12 -> 192 < 32 * 8: kchunk 64, five splits empty; 33 -> 528, not a multiple of 32 (kchunk 128: four full splits, 16 rows, three empty)
@pytest.mark.parametrize("t_live", [100, 0, 12, 33])
@pytest.mark.parametrize("M,N", [(256, 64), (4, 2)])
def test_weight_gradient_with_colsum(M, N, t_live):
    B, T, S, kchunk = 16, 100, 8, 256
    Kfull, Kl = B * T, B * t_live
    family = L.GEMM_FAMILY_DW128 if (M, N) == (256, 64) else L.GEMM_FAMILY_TILE128            # run_dw asserts it of each launch
    assert L.lib().mmfm_gemm_dw_tiles(256, 64, Kfull) == 2
    live = tuple(range(0, T, 1))[:t_live] if t_live in (0, 100) else tuple(sorted(torch.randperm(T, generator=torch.Generator().manual_seed(t_live))[:t_live].tolist()))
    _, rec = record(T, live)
    ldn = (N + 7) // 8 * 8
    dY = rnd(Kfull, M, seed=7).to(BF)
    X = torch.zeros(Kfull, ldn, device="cuda", dtype=BF)
    X[:, :N] = rnd(Kfull, N, seed=8).to(BF)
    # compact operands: the live rows first; the rows behind them hold NaN - nobody may read them
    idx = live_index(B, T, live)
    dYg, Xg = torch.full_like(dY, float("nan")), torch.full_like(X, float("nan"))
    dYg[:Kl], Xg[:Kl] = dY[idx], X[idx]
    dW, db = run_dw(family, dYg, Xg, M, N, Kfull, S, kchunk, live=K.live_rows(rec, B, T))
    if t_live == 0:
        assert torch.equal(dW, torch.zeros_like(dW)) and torch.equal(db, torch.zeros_like(db))
        assert not torch.signbit(dW).any() and not torch.signbit(db).any()
        return
    # the parent launch on the gathered operands (zero rows behind them would change nothing: it reads Kl rows)
    Sp = -(-Kl // kchunk)
    pW, pb = run_dw(family, dYg[:Kl].contiguous(), Xg[:Kl].contiguous(), M, N, Kl, Sp, kchunk)
    if t_live == T:
        ER.check_exact(dW, pW, "dW, every bin live")
        ER.check_exact(db, pb, "db, every bin live")
        return
    a, b = ER.f64(dYg[:Kl]), ER.f64(Xg[:Kl, :N])
    ref, mag = a.t() @ b, a.abs().t() @ b.abs()
    for what, got, gb in (("live", dW, db), ("parent", pW, pb)):
        ER.check_sum(got, ref, Kl, mag, f"dW ({what}) vs fp64, K_live = {Kl}")
        ER.check_sum(gb, a.sum(0), Kl, a.abs().sum(0), f"db ({what}) vs fp64, K_live = {Kl}")
