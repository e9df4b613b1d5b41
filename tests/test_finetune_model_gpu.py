"""FusedAdamW with param groups, frozen parameters and gradient clipping through the whole model path (optim.py, engine.py, mm.py).

The tiny model of tests/test_model_gpu.py: build_model(tiny_config(), 12, 2, seed=7), B = 2, T = 8, fp32 - and bf16 where the bf16 weight
copy matters.  Updates are compared with torch.optim.AdamW on the CPU in fp64, fed the engine's own gradients read from G, at
edge_refs.TOL_ADAMW (the bound of the existing AdamW kernel test), or bit for bit with the existing one-launch kernel."""
import math

import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR

import edge_refs as E
import optim_refs as R
from helpers import build_model, tiny_config
from model_checks import to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

LR, WD, EPS = 1e-3, 0.01, 1e-8
LATE = "decoder.0.mlp.up_proj.weight"


@pytest.fixture(scope="module")
def K():
    from multi_modal_foundation_model_amd import ops
    return ops


def mk(model, **kw):
    from multi_modal_foundation_model_amd.optim import make_optimizer
    return make_optimizer(model, lr=LR, weight_decay=WD, eps=EPS, **kw)


def fresh(dtype="fp32"):
    model = build_model(tiny_config(), 12, 2, seed=7).cuda().train()
    model.compute_dtype = dtype
    return model


def fwd_bwd(model, s):
    torch.manual_seed(1000 + s)                             # token masking draws from torch's stream
    out = model(to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=s), "encoding")))
    if out.loss.requires_grad:
        out.loss.backward()
    return out


def span(eng, name):
    off, shape = eng.layout.entries[name]
    return int(off), int(off) + int(math.prod(shape))


def raw(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def two_groups(named):
    """The usual AdamW recipe: biases, norm gains and the ScaleNorm scale (everything below two dimensions) take no weight decay."""
    return [dict(params=[p for p in named.values() if p.ndim >= 2], weight_decay=WD),
            dict(params=[p for p in named.values() if p.ndim < 2], weight_decay=0.0)]


def cpu_twin(model):
    return {k: torch.nn.Parameter(p.detach().double().cpu().clone()) for k, p in model.named_parameters()}


def feed(ref, eng, live=None):
    for k, p in ref.items():
        p.grad = eng.Gv(k).detach().double().cpu().clone() if (live is None or k in live) else None


def check_params(model, ref, what):
    for k, p in model.named_parameters():
        E.check_close(p.detach().cpu(), ref[k].detach(), E.TOL_ADAMW, f"{what}: {k}")


# ------------------------------------------------------------------------------------------------- param groups
def test_two_groups_with_onecycle_match_torch_adamw():
    model = fresh()
    named = dict(model.named_parameters())
    opt = mk(model, param_groups=two_groups(named))
    sch = OneCycleLR(opt, total_steps=10, max_lr=[1e-3, 3e-3], pct_start=0.3, div_factor=10)
    ref = cpu_twin(model)
    ropt = torch.optim.AdamW(two_groups(ref), lr=LR, eps=EPS)
    rsch = OneCycleLR(ropt, total_steps=10, max_lr=[1e-3, 3e-3], pct_start=0.3, div_factor=10)
    for s in range(5):
        fwd_bwd(model, s)
        feed(ref, model._engine)
        opt.step(); sch.step(); opt.zero_grad()
        ropt.step(); rsch.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ropt.param_groups]
        assert opt.param_groups[0]["lr"] != opt.param_groups[1]["lr"]
    assert opt._t == 5 and opt._steps is None and opt._tab.hyper_rows == 2 and opt._tab.n_ranges == len(named)
    check_params(model, ref, "two groups, 5 steps")


# ------------------------------------------------------------------------------------------------- frozen parameters
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_encoder_keeps_its_bytes_and_the_rest_steps_like_the_unfrozen_twin(K, dtype):
    model, twin = fresh(dtype), fresh(dtype)
    named = dict(model.named_parameters())
    frozen = [k for k in named if k.startswith(("encoder.", "encoder_embeddings."))]
    trainable = [k for k in named if k not in frozen]
    assert frozen and trainable
    for k in frozen:
        named[k].requires_grad_(False)
    opt = mk(model)                                           # model.parameters(): the frozen ones are owned and skipped (.grad is None)
    m2 = v2 = None
    for s in range(3):
        fwd_bwd(model, s)
        fwd_bwd(twin, s)
        eng, eng2 = model._engine, twin._engine
        if s == 0:
            P0, Pw0 = eng.P.clone(), eng.Pw.clone()
            m2, v2 = torch.zeros_like(eng2.P), torch.zeros_like(eng2.P)
        assert all(named[k].grad is None for k in frozen) and all(named[k].grad is not None for k in trainable)
        opt.step(); opt.zero_grad()
        # the twin: the existing kernel on each trainable parameter's slice, same gradients (its own G, the same bits)
        from multi_modal_foundation_model_amd.optim import adamw_hyper_row
        h = torch.tensor(adamw_hyper_row(LR, (0.9, 0.999), EPS, WD, s + 1), dtype=torch.float64).to(torch.float32).cuda()
        for k in trainable:
            a, b = span(eng2, k)
            E.check_exact(raw(eng.G[a:b]), raw(eng2.G[a:b]), f"gradient of {k}, step {s}")
            K.adamw_step(eng2.P[a:b], eng2.G[a:b], m2[a:b], v2[a:b], eng2.Pw[a:b] if dtype == "bf16" else None, b - a, h)
        twin.zero_grad(set_to_none=True)
    for k in frozen:
        a, b = span(eng, k)
        E.check_exact(raw(eng.P[a:b]), raw(P0[a:b]), f"frozen {k}")
        E.check_exact(raw(eng.Pw[a:b]), raw(Pw0[a:b]), f"frozen {k} (weight copy)")
        assert float(opt._m[a:b].abs().sum()) == 0.0 and float(opt._v[a:b].abs().sum()) == 0.0
    for k in trainable:
        a, b = span(eng, k)
        E.check_exact(raw(eng.P[a:b]), raw(eng2.P[a:b]), f"trainable {k}")
        E.check_exact(raw(eng.Pw[a:b]), raw(eng2.Pw[a:b]), f"trainable {k} (weight copy)")
        assert not torch.equal(eng.P[a:b], P0[a:b]), k
    assert opt._steps[trainable[0]] == 3 and opt._steps[frozen[0]] == 0 and opt._t == 3


def test_freezing_the_anchor_parameter_still_trains_the_rest():
    model = fresh()
    model.decoder_norm.weight.requires_grad_(False)
    opt = mk(model)
    out = fwd_bwd(model, 0)
    assert out.loss.grad_fn is not None
    eng = model._engine
    before = eng.P.clone()
    assert model.decoder_norm.weight.grad is None and model.decoder_norm.bias.grad is not None
    opt.step()
    a, b = span(eng, "decoder_norm.weight")
    assert torch.equal(eng.P[a:b], before[a:b])
    for k in ("decoder_norm.bias", "encoder.0.attn.query.weight", "decoder_embeddings.ap.out.weight"):
        a, b = span(eng, k)
        assert not torch.equal(eng.P[a:b], before[a:b]), k


def test_nothing_trainable_gives_a_loss_without_grad_fn():
    model = fresh()
    for p in model.parameters():
        p.requires_grad_(False)
    out = fwd_bwd(model, 0)
    assert out.loss.grad_fn is None and not out.loss.requires_grad and math.isfinite(out.loss.item())
    assert model._engine._last["bwd"] is None               # the forward-only plan


def test_parameter_unfrozen_at_step_3_takes_its_own_step_count():
    model = fresh()
    named = dict(model.named_parameters())
    named[LATE].requires_grad_(False)
    opt = mk(model)
    ref = cpu_twin(model)
    ref[LATE].requires_grad_(False)
    ropt = torch.optim.AdamW(list(ref.values()), lr=LR, weight_decay=WD, eps=EPS)
    for s in range(5):
        if s == 2:
            named[LATE].requires_grad_(True)
            ref[LATE].requires_grad_(True)
        fwd_bwd(model, s)
        feed(ref, model._engine, live={k for k, p in named.items() if p.requires_grad})
        opt.step(); opt.zero_grad()
        ropt.step()
    assert opt._steps[LATE] == 3 and ropt.state[ref[LATE]]["step"] == 3 and opt._steps["decoder_norm.bias"] == 5 and opt._t == 5
    assert opt._tab.hyper_rows == 2                         # (group 0, step 5) and (group 0, step 3)
    check_params(model, ref, "unfrozen at step 3 of 5")


# ------------------------------------------------------------------------------------------------- gradient clipping
def test_last_grad_norm_and_the_clipped_step():
    """The norm against the exactly rounded fp64 sum of the squares: the sum is within (n - 1) 2^-53 (any order, optim_refs.sumsq_bound),
    the square root halves a relative error and adds one rounding, 2^-53: together below the sum's bound for every n >= 3.  Then a step
    at half that norm equals the un-clipped one-launch optimiser fed G * clip_coef, bit for bit (bf16: the weight copy too)."""
    x, y = fresh("bf16"), fresh("bf16")
    ox, oy = mk(x, max_grad_norm=1e30), mk(y)
    fwd_bwd(x, 0)
    ox.step(); ox.zero_grad()
    fwd_bwd(y, 0)
    oy.step(); oy.zero_grad()
    ex, ey = x._engine, y._engine
    E.check_exact(raw(ex.P), raw(ey.P), "max_grad_norm above the norm: the plain step")
    fwd_bwd(x, 1)
    names = list(dict(x.named_parameters()))
    terms = [v for k in names for v in ex.Gv(k).detach().double().reshape(-1).cpu().tolist()]
    want = math.sqrt(math.fsum(v * v for v in terms))
    ox.max_grad_norm = 0.5 * want
    ox.step(); ox.zero_grad()
    got, coef = ox.last_grad_norm(), ox.last_clip_coef()
    print(f"[clip] grad norm {got!r} reference {want!r} rel err {abs(got - want) / want:.3e} bound {R.sumsq_bound(len(terms)):.3e}; clip_coef {coef!r}")
    assert abs(got - want) <= R.sumsq_bound(len(terms)) * want
    assert abs(coef - 0.5 * want / (got + 1e-6)) <= 2.0 ** -23 * coef and coef < 1.0
    norms = ox.grad_norms()
    assert sorted(norms) == sorted(names) and abs(math.sqrt(sum(v * v for v in norms.values())) - got) <= 1e-12 * got
    one = ex.Gv(LATE).detach().double().reshape(-1).cpu().tolist()
    assert abs(norms[LATE] - math.sqrt(math.fsum(v * v for v in one))) <= R.sumsq_bound(len(one)) * norms[LATE]
    assert ox.skipped_steps() == 0
    fwd_bwd(y, 1)
    E.check_exact(raw(ex.G), raw(ey.G), "the twins' gradients")     # G keeps the un-clipped gradient
    ey.G.mul_(coef)                                           # one fp32 multiply by the float in the record
    oy.step(); oy.zero_grad()
    E.check_exact(raw(ex.P), raw(ey.P), "clipped step against the plain optimiser on G * clip_coef")
    E.check_exact(raw(ex.Pw), raw(ey.Pw), "clipped step: the bf16 weight copy")


def test_skip_nonfinite_leaves_the_device_untouched_and_counts():
    model = fresh("bf16")
    opt = mk(model, skip_nonfinite=True)
    fwd_bwd(model, 0)
    eng = model._engine
    a, _ = span(eng, LATE)
    eng.G[a + 3] = float("inf")
    before = (eng.P.clone(), eng.Pw.clone())
    opt.step(); opt.zero_grad()
    assert opt.skipped_steps() == 1 and opt._t == 1          # the host counts the step: it cannot know without a sync
    E.check_exact(raw(eng.P), raw(before[0]), "skipped step")
    E.check_exact(raw(eng.Pw), raw(before[1]), "skipped step (weight copy)")
    assert float(opt._m.abs().sum()) == 0.0
    fwd_bwd(model, 1)
    opt.step()
    assert opt.skipped_steps() == 1 and not torch.equal(eng.P, before[0]) and math.isfinite(opt.last_grad_norm())


# ------------------------------------------------------------------------------------------------- resume
def test_resume_with_groups_clipping_and_uneven_step_counts_is_bit_identical(tmp_path):
    def make(model):
        named = dict(model.named_parameters())
        opt = mk(model, param_groups=two_groups(named), max_grad_norm=1e-3)
        return named, opt, OneCycleLR(opt, total_steps=10, max_lr=[1e-3, 3e-3], pct_start=0.3, div_factor=10)

    def steps(model, opt, sch, lo, hi):
        for s in range(lo, hi):
            fwd_bwd(model, s)
            opt.step(); sch.step(); opt.zero_grad()

    m1 = fresh()
    named, o1, s1 = make(m1)
    named[LATE].requires_grad_(False)                       # frozen for the first step only: the checkpoint holds uneven step counts
    steps(m1, o1, s1, 0, 1)
    named[LATE].requires_grad_(True)
    steps(m1, o1, s1, 1, 3)
    torch.save(dict(model=m1.state_dict(), opt=o1.state_dict(), sch=s1.state_dict()), tmp_path / "ck.pt")
    steps(m1, o1, s1, 3, 5)
    assert o1.last_clip_coef() < 1.0 and o1._steps[LATE] == 4 and o1._t == 5
    ck = torch.load(tmp_path / "ck.pt", weights_only=False)   # our own file
    assert ck["opt"]["fused"]["t"] == 3 and ck["opt"]["fused"]["steps"][LATE] == 2
    m2 = fresh()
    m2.load_state_dict(ck["model"])
    _, o2, s2 = make(m2)
    o2.load_state_dict(ck["opt"]); s2.load_state_dict(ck["sch"])
    steps(m2, o2, s2, 3, 5)
    assert o2._steps == o1._steps and o2._t == 5
    E.check_exact(raw(m2._engine.P), raw(m1._engine.P), "resumed run")
    E.check_exact(raw(o2._m), raw(o1._m), "resumed run: exp_avg")
    E.check_exact(raw(o2._v), raw(o1._v), "resumed run: exp_avg_sq")


def test_pre_change_checkpoint_with_only_t_loads_and_steps():
    model, twin = fresh(), fresh()
    o1, o2 = mk(model), mk(twin)
    for s in range(2):
        fwd_bwd(model, s)
        o1.step(); o1.zero_grad()
    sd = o1.state_dict()
    del sd["fused"]["steps"]                                # what state_dict wrote before per-parameter counts: t, m, v
    fwd_bwd(twin, 0)                                        # builds the twin's engine
    twin.zero_grad(set_to_none=True)
    twin.load_state_dict(model.state_dict())
    o2.load_state_dict(sd)
    assert o2._t == 2 and o2._steps is None
    for m, o in ((model, o1), (twin, o2)):
        fwd_bwd(m, 2)
        o.step(); o.zero_grad()
    E.check_exact(raw(twin._engine.P), raw(model._engine.P), "step 3 after loading a checkpoint without 'steps'")


# ------------------------------------------------------------------------------------------------- the default is untouched
def test_default_optimizer_issues_exactly_one_adamw_step(K, monkeypatch):
    calls = dict(adamw_step=0, adamw_step_ranges=0, grad_sumsq_ranges=0)
    for name in calls:
        def wrapped(*a, _f=getattr(K, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, wrapped)
    model = fresh()
    opt = mk(model)                                           # the four-argument make_optimizer
    fwd_bwd(model, 0)
    opt.step()
    assert calls == dict(adamw_step=1, adamw_step_ranges=0, grad_sumsq_ranges=0)
    assert opt._tab is None and opt._steps is None and opt._t == 1
    want = torch.tensor(E.adamw_hyper(1, LR, 0.9, 0.999, EPS, WD, 1.0), dtype=torch.float64).to(torch.float32)
    assert torch.equal(opt._hyper.cpu(), want)                # today's hyper vector
