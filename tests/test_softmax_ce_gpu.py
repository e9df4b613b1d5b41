"""Softmax cross-entropy and the arg-max confusion matrix through the C ABI (mmfm_softmax_ce_fwd / _bwd, mmfm_argmax_confusion), fp32
and bf16, against the fp64 reference and the derived bounds of tests/ce_refs.py on the kernels' own inputs (the bounds are judged on
the same inputs by tests/test_softmax_ce_cpu.py).  Runs on the MI355X only."""
import pytest
import torch

import ce_refs as R
import edge_refs as E

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
GUARD, SENT = 4096, 0xA5


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"R{s[0]}")
@pytest.mark.parametrize("Cn", R.CLASSES)
def test_softmax_ce_fwd_bwd(ops, Cn, shape, dtype):
    from multi_modal_foundation_model_amd import _lib as Lb
    Rr, T, ld, off = shape
    nbytes = Lb.lib().mmfm_softmax_ce_workspace(Rr, Cn)
    gout = torch.tensor([0.5], device="cuda")
    masks = {k: v.cuda() for k, v in R.make_masks(Rr, T, ld, off).items()}
    for variant in R.VARIANTS:
        pred, tgt = (x.cuda() for x in R.make_inputs(variant, Cn, Rr, dtype))
        w, eps = R.variant_params(variant, Cn)
        w = None if w is None else w.cuda()
        for name, store in masks.items():
            what = f"softmax_ce {variant} [{Rr}x{Cn}] {name}"
            rowmask = store[:, off:off + T]
            assert rowmask.data_ptr() == store.data_ptr() + off and store.stride(0) == ld
            on = (rowmask != 0).reshape(-1)
            outs, stats = [], []
            for call in range(2):                          # two calls: the same bits
                out = torch.full((1,), float("nan"), device="cuda")
                stat = torch.full((Rr, 2), -7.0, device="cuda")
                buf, ws = guarded(nbytes)
                ops.softmax_ce_fwd(pred, tgt, w, eps, rowmask, ld, T, Rr, Cn, out, stat, ws)
                assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"
                outs.append(out)
                stats.append(stat)
            E.check_exact(bits(outs[1]), bits(outs[0]), f"{what}: sum bits of two calls")
            E.check_exact(bits(stats[1]), bits(stats[0]), f"{what}: rowstat bits of two calls")
            out, stat = outs[0], stats[0]
            out_nostat = torch.full((1,), float("nan"), device="cuda")
            ops.softmax_ce_fwd(pred, tgt, w, eps, rowmask, ld, T, Rr, Cn, out_nostat, None, guarded(nbytes)[1])
            E.check_exact(bits(out_nostat), bits(out), f"{what}: sum bits without rowstat")
            s, n, sabs, terr = R.masked_ce_sum(pred, tgt, rowmask, w, eps)
            E.check_sum(out, s.reshape(1), n, sabs, f"{what} sum", term_err=terr)
            if n == 0:
                assert out.item() == 0.0
            assert bool((stat[~on] == -7.0).all()), f"{what}: rowstat of un-masked rows must not be written"
            sref, sbound = R.rowstat(pred, tgt, w, eps)
            assert R.within(stat[on], sref[on], sbound[on]), f"{what}: rowstat outside its bound"
            # the backward behind a finalize that also counts another modality
            cnt = torch.tensor([7, int(on.sum().item()) * Cn], dtype=torch.int64, device="cuda")
            loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
            ops.loss_finalize(torch.stack([torch.tensor(3.0, device="cuda"), out[0]]), cnt, 2, loss, inv_n)
            ref, bound = R.masked_ce_bwd(pred, tgt, rowmask, gout, inv_n, w, eps)
            grads = []
            for st in (stat, None, stat):                  # rowstat given, recomputed, and given again: the same bits
                dpred = torch.full((Rr, Cn), 7.0, dtype=dtype, device="cuda")
                ops.softmax_ce_bwd(pred, tgt, w, eps, rowmask, ld, T, Rr, Cn, st, gout, inv_n, dpred)
                grads.append(dpred)
            E.check_exact(bits(grads[1]), bits(grads[0]), f"{what}: dpred bits, rowstat NULL against given")
            E.check_exact(bits(grads[2]), bits(grads[0]), f"{what}: dpred bits of two calls")
            R.check_dpred(grads[0], ref, bound, f"{what} dpred")
            assert bool((grads[0][~on] == 0).all()), f"{what}: dpred must be exactly zero on un-masked rows"
    # nothing masked in any modality: 0 / 0 = NaN, inv_n = inf, and every gradient NaN
    loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.loss_finalize(torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), 2, loss, inv_n)
    assert bool(torch.isnan(loss[0])) and bool(torch.isinf(inv_n[0]))
    none = masks["none"][:, off:off + T]
    for st in (None, torch.zeros(Rr, 2, device="cuda")):
        dpred = torch.full((Rr, Cn), 7.0, dtype=dtype, device="cuda")
        ops.softmax_ce_bwd(pred, tgt, w, eps, none, ld, T, Rr, Cn, st, gout, inv_n, dpred)
        assert bool(torch.isnan(R.masked_ce_bwd(pred, tgt, none, gout, inv_n, w, eps)[0]).all())
        assert bool(torch.isnan(dpred).all()), "nothing masked: dpred must be NaN everywhere"


def test_softmax_ce_many_rows_more_than_one_block_and_grid_step(ops):
    """R beyond one grid step of the 2048 workgroups at N = 64 (4 rows a workgroup): 8300 rows, both dtypes against the reference."""
    from multi_modal_foundation_model_amd import _lib as Lb
    Rr, Cn, T = 8300, 64, 100
    g = torch.Generator().manual_seed(5)
    tgt = torch.softmax(torch.randn(Rr, Cn, generator=g), -1).cuda()
    rowmask = (torch.rand(Rr // T, T, generator=g) < 0.5).to(torch.uint8).cuda()
    rowmask.view(-1)[[0, 8191, 8192, Rr - 1]] = 1
    for dtype in (F32, BF16):
        pred = (torch.randn(Rr, Cn, generator=g) * 3).to(dtype).cuda()
        out = torch.empty(1, device="cuda")
        ws = torch.empty(Lb.lib().mmfm_softmax_ce_workspace(Rr, Cn), dtype=torch.uint8, device="cuda")
        ops.softmax_ce_fwd(pred, tgt, None, 0.0, rowmask, T, T, Rr, Cn, out, None, ws)
        s, n, sabs, terr = R.masked_ce_sum(pred, tgt, rowmask, None, 0.0)
        E.check_sum(out, s.reshape(1), n, sabs, f"softmax_ce [{Rr}x{Cn}] sum", term_err=terr)
        inv_n = torch.tensor([1.0 / n], device="cuda")
        dpred = torch.full((Rr, Cn), 7.0, dtype=dtype, device="cuda")
        ops.softmax_ce_bwd(pred, tgt, None, 0.0, rowmask, T, T, Rr, Cn, None, torch.ones(1, device="cuda"), inv_n, dpred)
        ref, bound = R.masked_ce_bwd(pred, tgt, rowmask, torch.ones(1, device="cuda"), inv_n, None, 0.0)
        R.check_dpred(dpred, ref, bound, f"softmax_ce [{Rr}x{Cn}] dpred")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"R{s[0]}")
@pytest.mark.parametrize("Cn", R.CLASSES)
def test_argmax_confusion_counts_are_exact(ops, Cn, shape, dtype):
    Rr, T, ld, off = shape
    g = torch.Generator().manual_seed(11 * Cn + Rr)
    pred = torch.randint(-3, 4, (Rr, Cn), generator=g).float()          # small integers: ties in most rows, exact in bf16
    tgt = torch.nn.functional.one_hot(torch.randint(0, Cn, (Rr,), generator=g), Cn).float()
    if Cn > 1:                                                           # planted: a tied pair whose higher index must lose, in both
        pred[0] = -5.0
        pred[0, [0, Cn - 1]] = 4.0
        tgt[Rr - 1] = 0.0
        tgt[Rr - 1, [Cn // 2, Cn - 1]] = 0.5
    pred, tgt = pred.to(dtype).cuda(), tgt.cuda()
    store = R.make_masks(Rr, T, ld, off)["mixed"].cuda()
    for rowmask in (None, store[:, off:off + T]):
        if rowmask is not None:
            rowmask[0, 0] = 1
            rowmask[-1, -1] = 1
        conf = torch.full((Cn, Cn), -1, dtype=torch.int64, device="cuda")
        for _ in range(2):                                               # overwritten, not accumulated
            ops.argmax_confusion(pred, tgt, rowmask, ld, T, Rr, Cn, conf)
        ref = R.confusion(pred, tgt, rowmask)
        assert int(ref.sum()) == (Rr if rowmask is None else int(rowmask.sum()))
        E.check_exact(conf, ref, f"confusion [{Rr}x{Cn}] mask={'none' if rowmask is None else 'mixed'}")
    if Cn > 1:
        assert R.first_argmax(pred.float())[0].item() == 0 and R.first_argmax(tgt)[Rr - 1].item() == Cn // 2


def test_metrics_confusion_accuracy_balanced_accuracy():
    from multi_modal_foundation_model_amd import metrics as Mx
    g = torch.Generator().manual_seed(2)
    B, T, Cn = 4, 6, 5
    labels = torch.randint(0, Cn, (B, T), generator=g)
    pred = torch.randn(B, T, Cn, generator=g)
    pred[0, :3] = torch.nn.functional.one_hot(labels[0, :3], Cn).float() * 9          # some certainly right
    tgt = torch.nn.functional.one_hot(labels, Cn).float()
    mask = (torch.rand(B, T, generator=g) < 0.7).to(torch.int64)
    mask[0, :3] = 1
    for m in (None, mask):
        for p in (pred, pred.to(BF16), pred.transpose(0, 1)):
            t_, m_ = (tgt.transpose(0, 1), None if m is None else m.transpose(0, 1)) if p.shape[0] == T else (tgt, m)
            conf = Mx.confusion(p.cuda(), t_.cuda(), None if m_ is None else m_.cuda())
            ref = R.confusion(p.float(), t_, m_)
            assert conf.dtype == torch.int64 and conf.is_cuda
            E.check_exact(conf.cpu(), ref, "metrics.confusion")
            pi, ti = R.first_argmax(p.float().reshape(-1, Cn)), labels.transpose(0, 1).reshape(-1) if p.shape[0] == T else labels.reshape(-1)
            on = torch.ones_like(ti, dtype=torch.bool) if m_ is None else m_.reshape(-1) != 0
            acc = float((pi[on] == ti[on]).double().mean())
            assert abs(Mx.accuracy(p.cuda(), t_.cuda(), None if m_ is None else m_.cuda()) - acc) < 1e-12
            recalls = [float((pi[on & (ti == c)] == c).double().mean()) for c in range(Cn) if bool((on & (ti == c)).any())]
            assert abs(Mx.balanced_accuracy(p.cuda(), t_.cuda(), None if m_ is None else m_.cuda()) - sum(recalls) / len(recalls)) < 1e-12
    with pytest.raises(RuntimeError, match="move the tensors to the GPU"):
        Mx.confusion(pred, tgt)
