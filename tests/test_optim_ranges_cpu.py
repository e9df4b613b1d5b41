"""The range-table optimiser without a GPU: the fp64 restatement of tests/optim_refs.py against torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_, the chunk table (the library's against the restatement's), the argument checks of the new entry
points (they return before anything is launched) and FusedAdamW's construction / binding rules."""
import ctypes as C
import math
import types

import pytest
import torch

import conftest  # noqa: F401  (puts the repo root and the API mirror on sys.path)
import optim_refs as R

D = torch.float64
CH = R.CHUNK


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D) * scale


def same(a, b, what, rtol=1e-12, atol=1e-13):
    assert a.dtype == D
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {(a - b).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------------- the restatement against torch
@pytest.mark.parametrize("max_norm_factor", [None, 2.0, 0.5], ids=["noclip", "above", "below"])
def test_range_adamw_ref_matches_torch_adamw_and_clip(max_norm_factor):
    """Two groups (own lr / weight decay / betas, rewritten every step as OneCycleLR does), one tensor frozen until step 3 (its first
    update takes bias correction 1), and max_norm above and below the measured norm; five steps, fp64 on both sides."""
    shapes = dict(w=(7, 5), b=(5,), gain=(1,), late=(4, 3))
    p0 = {k: rnd(*s, seed=i + 1) for i, (k, s) in enumerate(shapes.items())}
    tp = {k: torch.nn.Parameter(v.clone()) for k, v in p0.items()}
    tp["late"].requires_grad_(False)
    topt = torch.optim.AdamW([dict(params=[tp["w"], tp["late"]], lr=1e-3, weight_decay=0.01),
                              dict(params=[tp["b"], tp["gain"]], lr=3e-3, weight_decay=0.0)], eps=1e-8)
    params = {k: v.clone() for k, v in p0.items()}
    groups = [dict(names=["w", "late"], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
              dict(names=["b", "gain"], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)]
    grads0 = {k: rnd(*s, seed=100 + i, scale=0.3) for i, (k, s) in enumerate(shapes.items())}
    norm0 = math.sqrt(sum(float(g.pow(2).sum()) for k, g in grads0.items() if k != "late"))
    max_norm = None if max_norm_factor is None else max_norm_factor * norm0
    ref = R.RangeAdamW(params, groups, max_grad_norm=max_norm)
    for step in range(1, 6):
        if step == 3:
            tp["late"].requires_grad_(True)
        for gi, (lr, b1) in enumerate([(1e-3 * step, 0.95 - 0.01 * step), (3e-3 / step, 0.85 + 0.01 * step)]):
            topt.param_groups[gi]["lr"], topt.param_groups[gi]["betas"] = lr, (b1, 0.999)
            groups[gi]["lr"], groups[gi]["betas"] = lr, (b1, 0.999)
        grads = {k: grads0[k] * (1.0 + 0.1 * step) + rnd(*shapes[k], seed=1000 * step + i, scale=0.05)
                 for i, k in enumerate(shapes)}
        live = {k: (g if tp[k].requires_grad else None) for k, g in grads.items()}
        for k, p in tp.items():
            p.grad = None if live[k] is None else live[k].clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for p in tp.values() if p.grad is not None], max_norm)
        topt.step()
        ref.step(live)
        for k in shapes:
            same(params[k], tp[k].data, f"{k}, step {step}")
        if max_norm is not None:
            assert (ref.last_coef < 1.0) == (max_norm_factor < 1.0), "the case must sit on its side of the threshold"
    assert ref.steps == dict(w=5, b=5, gain=5, late=3)
    assert topt.state[tp["late"]]["step"] == 3 and topt.state[tp["w"]]["step"] == 5
    same(ref.m["late"], topt.state[tp["late"]]["exp_avg"], "late exp_avg")


def test_range_adamw_ref_skip_nonfinite_changes_nothing_but_counts():
    params = dict(a=rnd(6, seed=1), b=rnd(3, seed=2))
    before = {k: v.clone() for k, v in params.items()}
    ref = R.RangeAdamW(params, [dict(names=["a", "b"], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)], skip_nonfinite=True)
    g = dict(a=rnd(6, seed=3), b=rnd(3, seed=4))
    g["b"][1] = float("inf")
    ref.step(g)
    assert ref.skipped == 1 and ref.steps == dict(a=1, b=1)
    assert all(torch.equal(params[k], before[k]) for k in params) and float(ref.m["a"].abs().sum()) == 0.0


def test_range_step_is_the_single_range_update_per_range_and_leaves_the_gap():
    import edge_refs as E
    n = 50
    P, G, M, V = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3, scale=0.1), rnd(n, seed=4).abs()
    hyper = [E.adamw_hyper(3, 1e-3, 0.9), E.adamw_hyper(1, 5e-3, 0.8, wd=0.0)]
    ranges = [(0, 1, 0), (1, 8, 1), (20, 50, 0)]
    want = [t.clone() for t in (P, M, V)]
    for s, e, row in ranges:
        E.adamw_step(want[0][s:e], G[s:e] * 0.5, want[1][s:e], want[2][s:e], torch.tensor(hyper[row], dtype=D))
    gap = [t[8:20].clone() for t in (P, M, V)]
    R.range_step(P, G, M, V, ranges, hyper, clip=0.5)
    for got, w, g0 in zip((P, M, V), want, gap):
        assert torch.equal(got, w) and torch.equal(got[8:20], g0)


def test_clip_coef_is_torchs_formula():
    assert R.clip_coef(4.0, None) == 1.0 and R.clip_coef(4.0, 0.0) == 1.0 and R.clip_coef(4.0, float("inf")) == 1.0
    assert R.clip_coef(4.0, 3.0) == 1.0
    assert R.clip_coef(4.0, 1.0) == 1.0 / (2.0 + 1e-6)


# ------------------------------------------------------------------------------------------------- the chunk table
@pytest.fixture(scope="module")
def lib():
    from multi_modal_foundation_model_amd import _lib as L
    return L


CHUNK_CASES = {
    "length 1": [(0, 1, 0), (5, 6, 1), (CH - 1, CH, 0), (CH, CH + 1, 1)],
    "one past a boundary": [(0, CH + 1, 0), (CH + 1, 3 * CH + 1, 1)],
    "gap": [(3, 40, 0), (2 * CH + 5, 3 * CH + 37, 1)],
    "the kernel test's": [(0, 1, 0), (1, 8, 1), (8, CH + 9, 0), (2 * CH + 5, 3 * CH + 37, 1)],
    "exact chunks": [(0, CH, 0), (CH, 2 * CH, 0)],
}


@pytest.mark.parametrize("case", list(CHUNK_CASES))
def test_chunk_table_matches_the_restatement(lib, case):
    from multi_modal_foundation_model_amd import ops as K
    ranges = CHUNK_CASES[case]
    n = 3 * CH + 37
    assert lib.OPTIM_CHUNK == CH and C.sizeof(lib.OptimChunk) == 24 and C.sizeof(lib.OptimRecord) == 32 and C.sizeof(lib.OptimRange) == 24
    tab = K.OptimRanges(ranges, n, 2)                       # host only: no device
    chunks, first = tab.chunks()
    want_chunks, want_first = R.build_chunks(ranges)
    assert chunks == want_chunks and first == want_first
    # every chunk is non-empty, inside one CHUNK-aligned window, inside its range; together they tile the ranges exactly
    covered = []
    for s, ln, r, row in chunks:
        assert 1 <= ln <= CH and s // CH == (s + ln - 1) // CH
        assert ranges[r][0] <= s and s + ln <= ranges[r][1] and row == ranges[r][2]
        covered.append((s, s + ln))
    assert sum(e - s for s, e in covered) == sum(e - s for s, e, _ in ranges)
    assert all(a[1] <= b[0] for a, b in zip(covered, covered[1:]))
    assert lib.lib().mmfm_optim_ranges_workspace(len(chunks), len(ranges)) == 32 + 8 * (len(ranges) + len(chunks))
    assert lib.lib().mmfm_optim_ranges_table_bytes(len(chunks), len(ranges)) == 24 * len(chunks) + 4 * (len(ranges) + 1)


def test_chunk_table_exact_values_for_a_boundary_crossing(lib):
    from multi_modal_foundation_model_amd import ops as K
    chunks, first = K.OptimRanges([(8, CH + 9, 1)], 2 * CH, 2).chunks()
    assert chunks == [(8, CH - 8, 0, 1), (CH, 9, 0, 1)] and first == [0, 2]


# ------------------------------------------------------------------------------------------------- argument checks (no launch)
def _ranges(lib, rs):
    return (lib.OptimRange * len(rs))(*[lib.OptimRange(s, e, row, 0) for s, e, row in rs])


BAD_RANGES = {
    "overlapping": ([(0, 10, 0), (9, 20, 0)], "overlaps"),
    "unsorted": ([(10, 20, 0), (0, 5, 0)], "overlaps or precedes"),
    "past n": ([(0, 10, 0), (90, 101, 0)], "past n"),
    "empty": ([(5, 5, 0)], "empty"),
    "hyper row": ([(0, 10, 2)], "hyper row"),
    "negative row": ([(0, 10, -1)], "hyper row"),
}
FAKE = 0x1000            # a non-NULL "device pointer": the checks return before anything dereferences or launches


@pytest.mark.parametrize("case", list(BAD_RANGES))
def test_range_entry_points_refuse_bad_ranges_before_launching(lib, case):
    rs, msg = BAD_RANGES[case]
    l, arr = lib.lib(), _ranges(lib, rs)
    n, rows = 100, 2
    assert l.mmfm_optim_ranges_chunks(arr, len(rs), n, rows) == -1
    assert msg in l.mmfm_last_error().decode()
    assert l.mmfm_optim_ranges_table(arr, len(rs), n, rows, FAKE, 1 << 20) == -1
    assert msg in l.mmfm_last_error().decode()
    rc = l.mmfm_adamw_step_ranges(FAKE, FAKE, FAKE, FAKE, None, n, arr, len(rs), FAKE, len(rs), FAKE, rows, None, 0, None)
    assert rc == -1 and msg in l.mmfm_last_error().decode()
    if "row" not in case:                                   # the sum of squares reads no hyper row
        rc = l.mmfm_grad_sumsq_ranges(FAKE, n, arr, len(rs), FAKE, len(rs), 1.0, 0.0, 0, FAKE, 1 << 20, None)
        assert rc == -1 and msg in l.mmfm_last_error().decode()


def test_range_entry_points_refuse_null_pointers_and_a_foreign_table(lib):
    l, arr = lib.lib(), _ranges(lib, [(0, 10, 0), (20, 30, 1)])
    ok = dict(p=FAKE, g=FAKE, m=FAKE, v=FAKE, table=FAKE, hyper=FAKE)

    def step(n_chunks=2, ranges=arr, **kw):
        a = dict(ok, **kw)
        return l.mmfm_adamw_step_ranges(a["p"], a["g"], a["m"], a["v"], None, 100, ranges, 2, a["table"], n_chunks, a["hyper"], 2, None, 0, None)

    for name in ok:
        assert step(**{name: None}) == -1 and "NULL pointer" in l.mmfm_last_error().decode(), name
    assert step(ranges=None) == -1
    assert step(n_chunks=3) == -1 and "chunks" in l.mmfm_last_error().decode()

    def sumsq(g=FAKE, table=FAKE, ws=FAKE, ws_bytes=1 << 20, n_chunks=2, ranges=arr):
        return l.mmfm_grad_sumsq_ranges(g, 100, ranges, 2, table, n_chunks, 1.0, 1.0, 1, ws, ws_bytes, None)

    for kw in (dict(g=None), dict(table=None), dict(ws=None)):
        assert sumsq(**kw) == -1 and "NULL pointer" in l.mmfm_last_error().decode(), kw
    assert sumsq(ranges=None) == -1
    assert sumsq(n_chunks=1) == -1 and "chunks" in l.mmfm_last_error().decode()
    assert sumsq(ws_bytes=l.mmfm_optim_ranges_workspace(2, 2) - 1) == -1 and "workspace" in l.mmfm_last_error().decode()
    assert l.mmfm_optim_ranges_table(arr, 2, 100, 2, None, 1 << 20) == -1
    assert l.mmfm_optim_ranges_table(arr, 2, 100, 2, FAKE, l.mmfm_optim_ranges_table_bytes(2, 2) - 1) == -1


def test_header_declares_the_feature_macro(lib):
    with open(lib.HEADER_PATH) as f:
        src = f.read()
    assert "#define MMFM_OPTIM_RANGES 1" in src and f"#define MMFM_OPTIM_CHUNK {CH}" in src and "#define MMFM_VERSION 401" in src


# ------------------------------------------------------------------------------------------------- FusedAdamW: construction, binding
def _fake_engine(named, offsets):
    """What FusedAdamW._bind reads of an engine: the flat buffer (for its size and device), the parameters by name, the layout's
    (offset, shape) entries and the adoption count."""
    n = max(off + p.numel() for (name, p), off in zip(named.items(), offsets))
    return types.SimpleNamespace(P=torch.zeros(n), params=dict(named), adoptions=1, dtype="fp32",
                                 layout=types.SimpleNamespace(entries={k: (off, tuple(p.shape)) for (k, p), off in zip(named.items(), offsets)}))


def _named():
    return {"w": torch.nn.Parameter(torch.zeros(4, 3)), "b": torch.nn.Parameter(torch.zeros(3)), "g": torch.nn.Parameter(torch.zeros(1))}


def test_fused_adamw_accepts_param_groups_and_subsets():
    from multi_modal_foundation_model_amd.optim import FusedAdamW
    named = _named()
    opt = FusedAdamW([dict(params=[named["w"]], weight_decay=0.01), dict(params=[named["g"]], weight_decay=0.0, lr=5e-3)],
                     lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.attach(_fake_engine(named, [64, 0, 16]))
    opt._bind()                                                                   # two groups, and "b" is not owned
    assert [(o[0], o[2], o[3], o[4]) for o in opt._owned] == [("g", 16, 1, 1), ("w", 64, 12, 0)]     # buffer order
    assert not opt._covers_all and opt.max_grad_norm == 1.0 and opt.skip_nonfinite
    assert opt.param_groups[1]["lr"] == 5e-3 and opt.param_groups[0]["lr"] == 1e-3
    sd = opt.state_dict()
    assert sd["fused"]["t"] == 0 and sd["fused"]["steps"] is None and len(sd["param_groups"]) == 2
    assert FusedAdamW(list(named.values()), max_grad_norm=float("inf")).max_grad_norm is None     # torch: inf never clips


def test_fused_adamw_refuses_duplicates_and_foreign_tensors():
    from multi_modal_foundation_model_amd.optim import FusedAdamW
    named = _named()
    with pytest.raises(ValueError):
        FusedAdamW([dict(params=[named["w"]]), dict(params=[named["w"], named["b"]])])
    with pytest.warns(UserWarning), pytest.raises(ValueError):
        FusedAdamW([named["w"], named["w"]])
    opt = FusedAdamW([named["w"], torch.nn.Parameter(torch.zeros(2))])
    opt.attach(_fake_engine(named, [0, 16, 32]))
    with pytest.raises(RuntimeError, match="not one of the engine's parameters"):
        opt._bind()


def test_pre_change_checkpoint_loads_as_every_parameter_at_t():
    from multi_modal_foundation_model_amd.optim import FusedAdamW
    named = _named()
    eng = _fake_engine(named, [0, 16, 32])
    opt = FusedAdamW(list(named.values()), lr=1e-3).attach(eng)
    old = torch.optim.Optimizer.state_dict(opt)
    n = eng.P.numel()
    old["fused"] = dict(t=7, m=torch.full((n,), 0.5), v=torch.full((n,), 0.25))     # what the earlier state_dict wrote: no "steps"
    opt.load_state_dict(old)
    assert opt._t == 7 and opt._steps is None and float(opt._m[0]) == 0.5 and float(opt._v[-1]) == 0.25
    new = opt.state_dict()
    new["fused"]["steps"] = dict(w=7, b=7, g=2)
    opt2 = FusedAdamW(list(named.values()), lr=1e-3).attach(eng)
    opt2.load_state_dict(new)
    assert opt2._steps == dict(w=7, b=7, g=2) and opt2.state_dict()["fused"]["steps"] == dict(w=7, b=7, g=2)


def test_reference_config_builds_todays_optimizer():
    """The YAML keeps the reference's keys: optimizer.max_grad_norm is absent, the entry script reads it with .get and make_optimizer's
    first four parameters are what they were."""
    import inspect
    from helpers import load_config
    from multi_modal_foundation_model_amd.optim import make_optimizer
    assert load_config().optimizer.get("max_grad_norm", None) is None
    assert list(inspect.signature(make_optimizer).parameters) == ["model", "lr", "weight_decay", "eps", "param_groups", "max_grad_norm",
                                                                  "skip_nonfinite"]
