"""The loss family without a GPU: the fp64 references of tests/loss_refs.py against the torch modules they restate, the
`loss_mod` mapping of MultiModal (src/multi_modal/mm.py: _loss_spec / _loss_kind), the engine's call choice, and the argument
checks of the new entry points (they return before anything is launched)."""
import pytest
import torch
import torch.nn as nn

import conftest  # noqa: F401  (puts the repo root and the API mirror on sys.path)
import edge_refs as E
import loss_refs as R

D = torch.float64
FULL = R.FULL


def same(a, b, what, rtol=1e-12, atol=1e-13):
    assert a.dtype == D, f"{what}: the reference must return fp64, got {a.dtype}"
    assert torch.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True), f"{what}: max abs err {(a - b).abs().max().item():.3e}"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D) * scale


def _inputs(case, Rr, N):
    """(pred, target) in fp64 with the tie points of the kind on the first columns."""
    g = torch.Generator().manual_seed(7)
    if case in ("poisson_rate", "poisson_rate_full", "poisson_log_full"):
        tgt = torch.poisson(torch.full((Rr, N), 0.8, dtype=D), generator=g)
        tgt[0, :3] = torch.tensor([0.0, 1.0, 2.0], dtype=D)                      # t == 1 is outside Stirling's term, t == 2 inside
        pred = 1e-3 + 20 * torch.rand(Rr, N, generator=g, dtype=D) if case.startswith("poisson_rate") else rnd(Rr, N, seed=1, scale=2.0)
        assert (tgt >= 2).any()
    elif case == "bce":
        pred, tgt = rnd(Rr, N, seed=1, scale=4.0), (torch.rand(Rr, N, generator=g) < 0.5).to(D)
        pred[0, :3] = torch.tensor([0.0, 9.0, -9.0], dtype=D)
    else:
        tgt = torch.randint(-3, 4, (Rr, N), generator=g).to(D)
        pred = tgt + rnd(Rr, N, seed=1)
        pred[:, 0], pred[:, 1], pred[:, 2] = tgt[:, 0], tgt[:, 1] + 0.5, tgt[:, 2] - 0.5          # d == 0, |d| == beta == delta
    return pred, tgt


CASES = {  # name: (kind, param, flags, the torch module)
    "poisson_rate": (R.POISSON_RATE, 1e-8, 0, lambda: nn.PoissonNLLLoss(log_input=False, full=False, eps=R.f32(1e-8), reduction="none")),
    "poisson_rate_full": (R.POISSON_RATE, 1e-6, FULL, lambda: nn.PoissonNLLLoss(log_input=False, full=True, eps=R.f32(1e-6), reduction="none")),
    "poisson_log_full": (R.POISSON_LOG, 0.0, FULL, lambda: nn.PoissonNLLLoss(log_input=True, full=True, reduction="none")),
    "l1": (R.L1, 0.0, 0, lambda: nn.L1Loss(reduction="none")),
    "smooth_l1": (R.SMOOTH_L1, 0.5, 0, lambda: nn.SmoothL1Loss(reduction="none", beta=0.5)),
    "smooth_l1_beta0": (R.SMOOTH_L1, 0.0, 0, lambda: nn.SmoothL1Loss(reduction="none", beta=0.0)),
    "huber": (R.HUBER, 0.5, 0, lambda: nn.HuberLoss(reduction="none", delta=0.5)),
    "bce": (R.BCE_LOGITS, 0.0, 0, lambda: nn.BCEWithLogitsLoss(reduction="none")),
}


@pytest.mark.parametrize("case", list(CASES))
def test_loss_refs_match_torch_modules(case):
    kind, param, flags, make = CASES[case]
    B, T, M, N = 4, 5, 2, 6
    Rr = B * T
    pred, tgt = _inputs(case, Rr, N)
    crit = make()                                                                # eps: the fp32 value the reference rounds it to
    tokmask = (torch.rand(B, M * T, generator=torch.Generator().manual_seed(5)) < 0.5).to(torch.uint8)
    tokmask[0, T] = 1                                                            # row 0 carries the tie points
    rowmask = tokmask[:, T:]
    pr = pred.clone().requires_grad_(True)
    mk = rowmask.reshape(Rr, 1).to(D).expand(Rr, N)
    el_t = crit(pr, tgt)
    el, mag, err = R.loss_elem(kind, pred, tgt, param, flags)
    same(el, el_t.detach(), f"{case} elements")
    assert (mag >= el.abs() - 1e-12).all() and (err >= 0).all() and float(err.max()) < 1e-4 * (1 + float(mag.max()))
    other_sum, other_n = torch.tensor(3.0, dtype=D), 7
    total = (el_t * mk).sum()
    loss = (total + other_sum) / (mk.sum() + other_n)
    (0.5 * loss).backward()
    s, n, sabs, terr = R.masked_loss_sum(kind, pred, tgt, rowmask, param, flags)
    same(s, total.detach(), f"{case} sum")
    assert n == int(mk.sum()) and float(sabs) >= abs(float(s)) and 0 < float(terr) < 1e-5 * float(sabs)
    _, inv_n = E.loss_finalize(torch.stack([s, other_sum]), torch.tensor([int(mk.sum()), other_n]))
    same(R.masked_loss_bwd(kind, pred, tgt, rowmask, torch.tensor([0.5]), inv_n, param), pr.grad, f"{case} dpred")
    # nothing masked anywhere: NaN gradients, as autograd gives upstream
    none = torch.zeros(B, T, dtype=torch.uint8)
    s0, n0, _, _ = R.masked_loss_sum(kind, pred, tgt, none, param, flags)
    _, inv0 = E.loss_finalize(torch.stack([s0, s0]), torch.zeros(2, dtype=torch.int64))
    assert float(s0) == 0 and n0 == 0 and torch.isinf(inv0)
    assert torch.isnan(R.masked_loss_bwd(kind, pred, tgt, none, torch.ones(1), inv0, param)).all()


def test_refs_restate_the_two_original_kinds():
    """loss_refs carries kinds 0 / 1 only so that kind 0 can take the Stirling flag: without it they are edge_refs' terms."""
    pred, tgt = rnd(20, 6, seed=1, scale=2.0), torch.poisson(torch.full((20, 6), 0.3, dtype=D))
    rowmask = (torch.rand(4, 5, generator=torch.Generator().manual_seed(5)) < 0.5).to(torch.uint8)
    for kind in (0, 1):
        for a, b in zip(R.masked_loss_sum(kind, pred, tgt, rowmask), E.masked_loss_sum(kind, pred, tgt, rowmask)):
            assert float(a) == pytest.approx(float(b), rel=1e-14)


def test_tie_conventions():
    """sign(0) = 0; |d| == beta takes smooth-L1's linear branch, |d| == delta Huber's quadratic one (equal values and slopes)."""
    t = torch.zeros(5, dtype=D)
    p = torch.tensor([0.0, 0.5, -0.5, 0.25, 2.0], dtype=D)
    assert R.loss_grad(R.L1, p, t).tolist() == [0.0, 1.0, -1.0, 1.0, 1.0]
    assert R.loss_grad(R.SMOOTH_L1, p, t, 0.5).tolist() == [0.0, 1.0, -1.0, 0.5, 1.0]
    assert R.loss_grad(R.SMOOTH_L1, p, t, 0.0).tolist() == [0.0, 1.0, -1.0, 1.0, 1.0]
    assert R.loss_grad(R.HUBER, p, t, 0.5).tolist() == [0.0, 0.5, -0.5, 0.25, 0.5]
    assert R.loss_elem(R.SMOOTH_L1, p, t, 0.5)[0].tolist() == [0.0, 0.25, 0.25, 0.0625, 1.75]
    assert R.loss_elem(R.HUBER, p, t, 0.5)[0].tolist() == [0.0, 0.125, 0.125, 0.03125, 0.875]


# ------------------------------------------------------------------------------------------------- loss_mod mapping
def _mm():
    from multi_modal import mm
    return mm


NEW_SPECS = [
    (lambda: nn.PoissonNLLLoss(log_input=False, reduction="none"), (2, 1e-8, 0)),
    (lambda: nn.PoissonNLLLoss(log_input=False, full=True, eps=1e-6, reduction="none"), (2, 1e-6, FULL)),
    (lambda: nn.PoissonNLLLoss(log_input=True, full=True, reduction="none"), (0, 0.0, FULL)),
    (lambda: nn.L1Loss(reduction="none"), (3, 0.0, 0)),
    (lambda: nn.SmoothL1Loss(reduction="none"), (4, 1.0, 0)),
    (lambda: nn.SmoothL1Loss(reduction="none", beta=0.0), (4, 0.0, 0)),
    (lambda: nn.SmoothL1Loss(reduction="none", beta=0.25), (4, 0.25, 0)),
    (lambda: nn.HuberLoss(reduction="none"), (5, 1.0, 0)),
    (lambda: nn.HuberLoss(reduction="none", delta=0.5), (5, 0.5, 0)),
    (lambda: nn.BCEWithLogitsLoss(reduction="none"), (6, 0.0, 0)),
    (lambda: "poisson_nll_rate", (2, 1e-8, 0)),
    (lambda: "l1", (3, 0.0, 0)),
    (lambda: "smooth_l1", (4, 1.0, 0)),
    (lambda: "huber", (5, 1.0, 0)),
    (lambda: "bce_with_logits", (6, 0.0, 0)),
]


@pytest.mark.parametrize("i", range(len(NEW_SPECS)))
def test_loss_mod_maps_the_new_modules_and_strings(i):
    make, want = NEW_SPECS[i]
    mm = _mm()
    assert mm._loss_spec(make()) == want
    assert mm._loss_kind(make()) == want[0]


def test_loss_mod_maps_what_it_accepted_before_as_before():
    """Everything the two-kind _loss_kind took: the model's own strings, the substring rule, the reference's modules (whatever their
    reduction - it was never read), and classes named like them."""
    mm = _mm()

    class MyMSELoss(nn.Module):
        pass

    class PoissonLike(nn.Module):
        log_input = True

    before = [("poisson_nll_log_input", 0), ("mse", 1), ("Poisson", 0), ("my_mse_loss", 1), ("poisson_mse", 0),
              (nn.PoissonNLLLoss(reduction="none", log_input=True), 0), (nn.PoissonNLLLoss(), 0), (nn.MSELoss(reduction="none"), 1),
              (nn.MSELoss(), 1), (MyMSELoss(), 1), (PoissonLike(), 0)]
    for spec, kind in before:
        assert mm._loss_kind(spec) == kind and type(mm._loss_kind(spec)) is int, spec
        assert mm._loss_spec(spec) == (kind, 0.0, 0), spec                      # and so the engine issues the two-kind calls

    class PoissonRateLike(nn.Module):
        log_input = False
    with pytest.raises(NotImplementedError):
        mm._loss_kind(PoissonRateLike())
    with pytest.raises(NotImplementedError):
        mm._loss_kind("cross_entropy")


def test_loss_mod_rejections_name_the_cause():
    mm = _mm()
    for make in (lambda: nn.HuberLoss(reduction="mean"), lambda: nn.L1Loss(reduction="sum"), lambda: nn.BCEWithLogitsLoss(),
                 lambda: nn.SmoothL1Loss(), lambda: nn.PoissonNLLLoss(log_input=False), lambda: nn.PoissonNLLLoss(full=True)):
        with pytest.raises(NotImplementedError, match="reduction"):
            mm._loss_spec(make())
    with pytest.raises(NotImplementedError, match="pos_weight"):
        mm._loss_spec(nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.ones(3)))
    with pytest.raises(NotImplementedError, match="pos_weight"):
        mm._loss_spec(nn.BCEWithLogitsLoss(reduction="none", weight=torch.ones(3)))
    for spec in (nn.GaussianNLLLoss(reduction="none"), nn.CrossEntropyLoss(reduction="none"), nn.BCELoss(reduction="none")):
        with pytest.raises(NotImplementedError, match="no HIP kernel for this class"):
            mm._loss_spec(spec)

    class MyHuber(nn.HuberLoss):                 # exact class only: a subclass may compute anything
        pass
    with pytest.raises(NotImplementedError, match="no HIP kernel for this class"):
        mm._loss_spec(MyHuber(reduction="none"))
    with pytest.raises(ValueError):
        mm._loss_spec(nn.SmoothL1Loss(reduction="none", beta=-1.0))


def test_engine_config_carries_kind_param_and_flags():
    from multi_modal_foundation_model_amd.engine import EngineConfig
    from helpers import load_config
    ec = EngineConfig.from_model_config(load_config().model, [("ap", 668), ("behavior", 2)])
    assert ec.loss_kind == {"ap": 0, "behavior": 1} and ec.loss_param == {} and ec.loss_flags == {}
    ec.loss_kind, ec.loss_param, ec.loss_flags = {"ap": 2, "behavior": 5}, {"ap": 1e-8, "behavior": 0.5}, {"ap": FULL}
    assert (ec.loss_kind["behavior"], ec.loss_param["behavior"], ec.loss_flags.get("behavior", 0)) == (5, 0.5, 0)


# ------------------------------------------------------------------------------------------------- argument checks
def test_new_entry_points_check_their_arguments():
    """Bad kinds, a negative parameter, the Stirling flag on a kind without it, an unknown flag and null pointers return -1 with a
    message, before any launch (so this runs without a GPU); the two-kind entry points still refuse the new kinds."""
    from multi_modal_foundation_model_amd import _lib as L
    lib = L.lib()
    p = 4096                                     # a non-null address: no check below gets as far as using it

    def fwd(kind, param, flags, pred=p, ws=p, dtype=0, R=8, T=4):
        return lib.mmfm_masked_loss_kind_fwd(dtype, kind, param, flags, pred, p, p, T, T, R, 3, p, ws, 1 << 20, None)

    def bwd(kind, param, flags, dpred=p, R=8, T=4):
        return lib.mmfm_masked_loss_kind_bwd(0, kind, param, flags, p, p, p, T, T, R, 3, p, p, dpred, None)

    for call in (fwd, bwd):
        for kind, param, flags in ((-1, 0.0, 0), (7, 0.0, 0), (L.LOSS_HUBER, -0.5, 0), (L.LOSS_SMOOTH_L1, -1e-3, 0),
                                   (L.LOSS_POISSON_RATE, -1e-8, 0), (L.LOSS_HUBER, float("nan"), 0), (L.LOSS_HUBER, 0.5, L.LOSS_FULL),
                                   (L.LOSS_BCE_LOGITS, 0.0, L.LOSS_FULL), (L.LOSS_POISSON_RATE, 1e-8, 2)):
            assert call(kind, param, flags) == -1, (call.__name__, kind, param, flags)
            assert b"bad kind" in lib.mmfm_last_error()
        assert call(L.LOSS_HUBER, 0.5, 0, R=7) == -1 and b"bad arguments" in lib.mmfm_last_error()        # R % T != 0
    assert fwd(L.LOSS_L1, 0.0, 0, pred=None) == -1 and b"null pointer" in lib.mmfm_last_error()
    assert bwd(L.LOSS_L1, 0.0, 0, dpred=None) == -1 and b"null pointer" in lib.mmfm_last_error()
    assert fwd(L.LOSS_L1, 0.0, 0, ws=None) == -1 and b"workspace" in lib.mmfm_last_error()
    assert fwd(L.LOSS_L1, 0.0, 0, dtype=2) == -1 and b"bad dtype" in lib.mmfm_last_error()
    for kind in range(2, 7):
        assert lib.mmfm_masked_loss_fwd(0, kind, p, p, p, 4, 4, 8, 3, p, p, 1 << 20, None) == -1
        assert b"mmfm_masked_loss_fwd: bad arguments" in lib.mmfm_last_error()
        assert lib.mmfm_masked_loss_bwd(0, kind, p, p, p, 4, 4, 8, 3, p, p, p, None) == -1
        assert b"mmfm_masked_loss_bwd: bad arguments" in lib.mmfm_last_error()
