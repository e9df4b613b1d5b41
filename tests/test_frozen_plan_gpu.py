"""The backward plan pruned to what the trainable parameters need (plan.py, engine.py, ddp.py).

fp32: the tiny model of tests/test_finetune_model_gpu.py with two layers per stack (pattern (h) names decoder.1, and with two decoder
layers "the last layer writes d/ctx, the others add" is in play) and dropout on at every site, B = 2, T = 8.  Each freeze pattern runs one
step on the batch and seeds of an all-trainable twin: every trainable parameter's slice of G is the twin's bit for bit (a dropout mask
depends on its site and the RNG state only), every frozen parameter's .grad is None, and the report says what was pruned.  The launches
are compared through tests/plan_sig.py records: a pruned backward is a sub-sequence of the all-trainable one, but for three named kinds.

bf16 at the default widths: the same comparison at the smallest batch whose large-regime record shows every weight-gradient pair of the
all-trainable plan leaving in one launch; a product that lost its partner is compared with the all-trainable plan under MMFM_DW_PAIR=0."""
import difflib
import fnmatch
import json
import math

import pytest
import torch

import edge_refs as E
import large_regime as LR
import plan_sig as PS
from helpers import build_model, model_config, tiny_config
from model_checks import to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

B, T = 2, 8
ENC_TOK = "encoder_embeddings.*"
# pattern -> (fnmatch patterns, True: they name the trainable parameters / False: the frozen ones)
PATTERNS = {
    "a_encoder_frozen": (["encoder.*", ENC_TOK], False),
    "b_trunk_frozen": ([ENC_TOK, "decoder_embeddings.*"], True),                   # tokenisers + heads
    "c_heads_only": (["decoder_embeddings.*.out.*"], True),
    "d_encoder0_only": (["encoder.0.*"], True),
    "e_decoder_norm_weight": (["decoder_norm.weight"], True),
    "f_enc_mod_pos": (["encoder_embeddings.*.mod_emb.*", "encoder_embeddings.*.pos_embed.*"], True),
    "g_dec0_cross_kv": (["decoder.0.cross_attn.key.*", "decoder.0.cross_attn.value.*"], True),      # the fused projection cross_attn.kv
    "h_dec1_down_proj": (["decoder.1.mlp.down_proj.*"], True),
}


def split(names, pats, trainable):
    hit = [k for k in names if any(fnmatch.fnmatchcase(k, p) for p in pats)]
    assert hit, pats
    return [k for k in names if (k in hit) != trainable]          # the frozen names


def fresh(mc, dtype="fp32", share=True, n_ap=12):
    model = build_model(mc, n_ap, 2, seed=7, share_modality_embeddings=share).cuda().train()
    model.compute_dtype = dtype
    return model


def freeze(model, frozen):
    named = dict(model.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    return named


def fwd_bwd(model, s, b=B, t=T, n_ap=12):
    torch.manual_seed(1000 + s)                             # token masking draws from torch's stream
    out = model(to_dev(O.make_mod_dict(O.synth_batch(b, t, n_ap, 2, seed=s), "encoding")))
    out.loss.backward()
    return out


def span(eng, name):
    off, shape = eng.layout.entries[name]
    return int(off), int(off) + int(math.prod(shape))


def raw(t):
    return t.view(torch.int32)


def tiny():
    return tiny_config(n_enc=2, n_dec=2, dropout=0.1, emb_dropout=0.1)


_TWINS = {}


def twin_grads(key, make):
    """G of the all-trainable twin after one step, computed once per configuration and left unchanged."""
    if key not in _TWINS:
        twin = make()
        fwd_bwd(twin, 0)
        _TWINS[key] = (twin._engine.G.clone(), twin)
    return _TWINS[key]


# ------------------------------------------------------------------------------------------------ structure, through plan_sig records
def _strip(rec):
    """A reduce_slabs_multi record without the rows' running chunk offsets (they shift when a row in front leaves)."""
    return [{k: v for k, v in row.items() if k != "chunk0"} for row in rec["keep"][0]]


def _subsequence(small, big):
    it = iter(big)
    return all(any(x == y for y in it) for x in small)


def check_structure(eng, pruned, full, frozen):
    """Every launch of `pruned` is a launch of `full`, argument for argument and in the same relative order, or one of three kinds: the
    survivor of a weight-gradient pair (the product alone, with the reduction of its slabs), an MLP front half with t1 = g = NULL, a
    batched slab reduction whose table is a sub-sequence of the full one's.  The forward records are identical, and no pointer of the
    pruned backward resolves into G inside the span of a parameter whose group was pruned."""
    sp, sf = PS.plan_signature(eng, pruned, full=True), PS.plan_signature(eng, full, full=True)
    assert sp["fwd"]["sha256"] == sf["fwd"]["sha256"], "the forward of a pruned plan is the all-trainable forward"
    assert list(sp) == list(sf)                               # every segment keeps its name and place
    kinds = dict(same=0, survivor=0, dx_only=0, table=0)
    for unit in sp:
        if unit == "fwd":
            continue
        recs, ref = sp[unit]["records"], sf[unit]["records"]
        pair_ops = [(d["A"], d["B"]) for r in ref if r["fn"] == "mmfm_gemm_pair" for d in r["keep"]]
        # the longest run of the pruned launches that is a sub-sequence of the full ones; what it leaves out must be of a named kind
        key = lambda r: json.dumps(r, sort_keys=True)
        blocks = difflib.SequenceMatcher(None, [key(r) for r in recs], [key(r) for r in ref], autojunk=False).get_matching_blocks()
        matched = {i for a, _, n in blocks for i in range(a, a + n)}
        for i, r in enumerate(recs):
            if i in matched:
                kinds["same"] += 1
            elif r["fn"] == "mmfm_gemm" and (r["keep"][0]["A"], r["keep"][0]["B"]) in pair_ops:
                kinds["survivor"] += 1
            elif r["fn"] == "mmfm_reduce_slabs" and any(q["fn"] == "mmfm_reduce_slabs" and q["args"][0] == r["args"][0] for q in ref):
                kinds["survivor"] += 1                        # the survivor's slabs, summed into the destination the pair's reduction had
            elif r["fn"] == "mmfm_mlp_bwd" and r["keep"][0]["t1"] is None and r["keep"][0]["g"] is None:
                twin = [q for q in ref if q["fn"] == "mmfm_mlp_bwd" and {**q["keep"][0], "t1": None, "g": None} == r["keep"][0]]
                assert len(twin) == 1, (unit, r)
                kinds["dx_only"] += 1
            elif r["fn"] == "mmfm_reduce_slabs_multi":
                tabs = [q for q in ref if q["fn"] == "mmfm_reduce_slabs_multi"]
                assert len(tabs) == 1 and _subsequence(_strip(r), _strip(tabs[0])), (unit, r)
                kinds["table"] += 1
            else:
                raise AssertionError(f"{unit}: {r['fn']} is no launch of the all-trainable plan (or out of order): {r}")
    rep = pruned["report"]
    dead = sorted(span(eng, k) for k in rep["pruned_params"])
    assert set(rep["pruned_params"]) <= set(frozen)

    def walk(v):
        if isinstance(v, list) and len(v) == 2 and v[0] == "G" and isinstance(v[1], int):
            off = v[1] // 4
            assert not any(a <= off < b for a, b in dead), f"a launch of the pruned backward points into G at {off}, inside a pruned group"
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, list):
            for x in v:
                walk(x)
    for unit in sp:
        if unit != "fwd":
            walk(sp[unit]["records"])
    return kinds


def live_segments(rep):
    return [name for name, n, _ in rep["segments"] if n]


# ------------------------------------------------------------------------------------------------ fp32, the tiny model
CASES = [(k, True) for k in PATTERNS] + [("f_enc_mod_pos", False)]


@pytest.mark.parametrize("pattern,share", CASES, ids=[f"{k}{'' if s else '_unshared'}" for k, s in CASES])
def test_pruned_step_gives_the_twins_gradients_bit_for_bit(pattern, share):
    G2, _ = twin_grads(("fp32", share), lambda: fresh(tiny(), share=share))
    model = fresh(tiny(), share=share)
    names = list(dict(model.named_parameters()))
    pats, trainable = PATTERNS[pattern]
    frozen = split(names, pats, trainable)
    named = freeze(model, frozen)
    fwd_bwd(model, 0)
    eng = model._engine
    rep = eng.backward_report(B, T)
    print(f"[{pattern}{'' if share else ' unshared'}] {eng.backward_summary(B, T)}; pruned {rep['pruned']}")
    for k in names:
        if k in frozen:
            assert named[k].grad is None, k
        else:
            a, b = span(eng, k)
            assert named[k].grad is not None and named[k].grad.data_ptr() == eng.Gv(k).data_ptr()
            E.check_exact(raw(eng.G[a:b]), raw(G2[a:b]), f"{pattern}: gradient of {k}")
    # pruning happened, and what the rule says
    full = [n for _, _, n in rep["segments"]]
    assert rep["launches"] < rep["full"] == sum(full) and all(n <= f for _, n, f in rep["segments"])
    assert [s for s, _, _ in rep["segments"]] == ["head", "decoder.1", "decoder.0", "bridge", "encoder.1", "encoder.0", "embed"]
    live = live_segments(rep)
    counts = {s: (n, f) for s, n, f in rep["segments"]}
    if pattern == "a_encoder_frozen":
        # nothing below the decoder stack but the decoder's own tokenisers (they are trainable: their launches stay in `embed`)
        # (and the bridge: encoder_norm and decoder_proj_context are no part of `encoder.*`)
        assert live == ["head", "decoder.1", "decoder.0", "bridge", "embed"] and counts["embed"][0] < counts["embed"][1]
        assert not [g for g in rep["pruned"] if g.startswith("decoder")] and "encoder_embeddings.ap.embedder.token_embed" in rep["pruned"]
    if pattern == "b_trunk_frozen":
        assert counts["embed"][0] == counts["embed"][1] and all(0 < counts[s][0] < counts[s][1] for s in counts if s not in ("embed", "head"))
    if pattern == "c_heads_only":
        assert live == ["head"]
    if pattern == "d_encoder0_only":
        assert live == ["head", "decoder.1", "decoder.0", "bridge", "encoder.1", "encoder.0"]
        # every weight gradient above encoder.0 is pruned, the dX chain (with the un-fused norms' backwards) is whole
        lins = [l.name for l in eng.linears] + ["decoder_embeddings.ap.out", "decoder_embeddings.behavior.out"]
        assert {g for g in lins if g in rep["pruned"]} == {g for g in lins if not g.startswith("encoder.0.")}
        # ... of the context / encoder stream; the decoder stream ends at decoder.0's cross-attention, whose d/kvc is the last thing needed of it
        assert [g for g in rep["pruned"] if g.endswith(("ln1", "ln2", "_norm"))] == ["decoder.0.query_norm", "decoder.0.ln1"]
    if pattern == "e_decoder_norm_weight":
        assert live == ["head"] and counts["head"][0] < counts["head"][1]
    if pattern == "f_enc_mod_pos":
        # the shared table's decoder-side writer needs the decoder stream down to the tokenisers; an unshared one is pruned with it
        assert ("decoder_embeddings.ap.embedder.mod_emb+pos_embed" in rep["pruned"]) == (not share)
        assert live[-1] == "embed" and "encoder.0" in live
    if pattern == "g_dec0_cross_kv":
        assert live == ["head", "decoder.1", "decoder.0"]
    if pattern == "h_dec1_down_proj":
        assert live == ["head", "decoder.1"]
    full_plan = eng._plan(B, T, True, True)                   # builds the all-trainable plan beside the pruned one, launches nothing
    assert full_plan is not eng._last and full_plan["report"]["pruned"] == []
    assert [(s, f) for s, _, f in rep["segments"]] == [(s, len(seg)) for s, seg in full_plan["bwd"]]
    kinds = check_structure(eng, eng._last, full_plan, frozen)
    assert kinds["same"] == rep["launches"]                   # fp32, one slab: no pairs, no fused MLP, no reduction tables


def test_all_trainable_keeps_todays_key_and_plan():
    model = fresh(tiny())
    fwd_bwd(model, 0)
    eng = model._engine
    assert eng.freeze_pattern() is None and list(eng.plans) == [(B, T, True, True)] and eng._last is eng.plans[(B, T, True, True)]
    rep = eng.backward_report(B, T)
    assert rep["pruned"] == [] and rep["launches"] == rep["full"] and all(n == f for _, n, f in rep["segments"])


# ------------------------------------------------------------------------------------------------ unfreezing, the pattern cache
def test_unfreezing_selects_the_full_plan_and_a_fifth_pattern_evicts_the_oldest():
    model, twin = fresh(tiny()), fresh(tiny())
    names = list(dict(model.named_parameters()))
    enc = split(names, ["encoder.*", ENC_TOK], False)
    named = freeze(model, enc)
    for s in range(2):
        fwd_bwd(model, s)
        model.zero_grad(set_to_none=True)
        fwd_bwd(twin, s)                                      # (no optimiser: the parameters stay the same; the RNG state moves alike)
        twin.zero_grad(set_to_none=True)
    for k in enc:
        named[k].requires_grad_(True)
    fwd_bwd(model, 2)
    fwd_bwd(twin, 2)
    eng = model._engine
    assert eng._last is eng.plans[(B, T, True, True)] and len(eng.plans) == 2
    for k in names:
        a, b = span(eng, k)
        E.check_exact(raw(eng.G[a:b]), raw(twin._engine.G[a:b]), f"third step, unfrozen: gradient of {k}")
    # gradual unfreezing: patterns 3, 4 are kept beside the first two, a fifth drops the least recently used (the frozen encoder)
    first = next(k for k in eng.plans if len(k) == 5)
    model.zero_grad(set_to_none=True)
    for i, k in enumerate(["decoder_norm.weight", "decoder_norm.bias", "encoder_norm.weight"]):
        named[k].requires_grad_(False)
        fwd_bwd(model, 3 + i)
        model.zero_grad(set_to_none=True)
        assert (first in eng.plans) == (i < 2) and len(eng.plans) == min(3 + i, 4)
    assert (B, T, True, True) in eng.plans and eng._pattern_lru[(B, T)][0] is None


# ------------------------------------------------------------------------------------------------ hipGraph replay
@pytest.mark.parametrize("pattern", ["a_encoder_frozen", "c_heads_only"])
def test_three_pruned_steps_replayed_equal_three_eager_ones(pattern, monkeypatch):
    from multi_modal_foundation_model_amd.optim import make_optimizer
    final = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = fresh(tiny())
        names = list(dict(model.named_parameters()))
        freeze(model, split(names, *PATTERNS[pattern]))
        opt = make_optimizer(model, lr=1e-3, weight_decay=0.01, eps=1e-8)
        for s in range(3):
            fwd_bwd(model, s)
            opt.step(); opt.zero_grad()
        plan = model._engine._last
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["bwd"] == 3
        if pattern == "c_heads_only":
            assert [name for name, seg in plan["bwd"] if seg] == ["head"] and len(plan["bwd"]) == 7
        final[mode] = model._engine.P.clone()
    E.check_exact(raw(final["1"]), raw(final["0"]), f"{pattern}: parameters after three steps, hipGraph against eager")


# ------------------------------------------------------------------------------------------------ DDP: the ranges issued
@pytest.mark.parametrize("pattern", ["a_encoder_frozen", "c_heads_only"])
def test_engine_ddp_all_reduces_the_trainable_spans_only(pattern, monkeypatch, tmp_path):
    import torch.distributed as dist
    from multi_modal_foundation_model_amd import ddp as D
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rdv", rank=0, world_size=1)
    try:
        model = fresh(tiny())
        names = list(dict(model.named_parameters()))
        frozen = split(names, *PATTERNS[pattern])
        freeze(model, frozen)
        eng = model.engine()
        wrap = D.EngineDDP(eng, bucket_bytes=16 << 10, broadcast=False)
        issued, real = [], dist.all_reduce

        def recorded(t, *a, **kw):
            issued.append(((t.data_ptr() - eng.G.data_ptr()) // 4, (t.data_ptr() - eng.G.data_ptr()) // 4 + t.numel()))
            return real(t, *a, **kw)
        monkeypatch.setattr(dist, "all_reduce", recorded)
        fired = []
        eng.grad_ready_hooks.append(fired.append)
        fwd_bwd(model, 0)
        spans = D.trainable_spans(eng.layout, wrap.buckets.buckets, [k for k in names if k not in frozen])
        assert len(wrap.buckets.buckets) >= 3
        assert issued == [spans[name] for name, _, _ in wrap.buckets.buckets if spans[name] is not None]
        assert fired == D.backward_order(eng.layout, eng.cfg)             # every segment's hook fires, in order, empty or not
        if pattern == "c_heads_only":
            assert len(issued) == 1 and sum(v is None for v in spans.values()) == len(spans) - 1
        assert not wrap.works
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ bf16, default widths, pairs
def smallest_paired_batch():
    """The smallest batch at T = 100 whose weight-gradient pairs all leave in one launch (large_regime.host_gates; pairs need
    R = 200 B > 8192, and R >= 12,288 for the row-owner MLP kernels whose down / up products pair), by the library's own answer - and the test then reads the same off the built plan's record."""
    for b in range(8192 // 200 + 1, LR.B_BIG + 1):
        g = LR.host_gates(b)
        if g["fused_mask_15"] and g["batch_red_off_pairing_on"] and g["dw_pairs_one_launch"]:      # (mask 15: the MLP blocks pair too)
            return b
    raise AssertionError("no batch up to B_BIG pairs every weight gradient")


BF16 = {
    "a_encoder_frozen": PATTERNS["a_encoder_frozen"],
    "b_trunk_frozen": PATTERNS["b_trunk_frozen"],
    "h_dec1_down_proj": PATTERNS["h_dec1_down_proj"],
    "down_proj_frozen_everywhere": (["*.mlp.down_proj.*"], False),
}
_BF = {}


def bf16_twins(monkeypatch):
    """G of the all-trainable plan, and of the all-trainable plan under MMFM_DW_PAIR=0, one step each; computed once."""
    if not _BF:
        bb = smallest_paired_batch()
        mc = model_config(n_enc=2, n_dec=2, dropout=0.1, emb_dropout=0.1)
        for pair in ("1", "0"):
            monkeypatch.setenv("MMFM_DW_PAIR", pair)
            m = fresh(mc, "bf16", n_ap=668)
            fwd_bwd(m, 0, bb, 100, 668)
            _BF[pair] = (m._engine.G.clone(), m)
        monkeypatch.delenv("MMFM_DW_PAIR")
        eng = _BF["1"][1]._engine
        rec = LR.regime_record(eng, eng._last)
        pairs = [g for unit in rec["launches"].values() for g in unit if g["fn"] == "mmfm_gemm_pair"]
        assert rec["decisions"]["pair_ok"] and rec["decisions"]["fm"] == 15 and len(pairs) == 2 * 2 + 3 * 2 and all(g["one_launch"] for g in pairs)
        _BF["B"], _BF["mc"] = bb, mc
    return _BF


@pytest.mark.parametrize("pattern", list(BF16))
def test_bf16_pruned_step_with_broken_pairs(pattern, monkeypatch):
    for k in PS.SWITCHES + PS.AUTO:
        monkeypatch.delenv(k, raising=False)
    tw = bf16_twins(monkeypatch)
    bb = tw["B"]
    model = fresh(tw["mc"], "bf16", n_ap=668)
    names = list(dict(model.named_parameters()))
    frozen = split(names, *BF16[pattern])
    freeze(model, frozen)
    fwd_bwd(model, 0, bb, 100, 668)
    eng = model._engine
    rep = eng.backward_report(bb, 100)
    print(f"[bf16 {pattern} B={bb}] {eng.backward_summary(bb, 100)}")
    full_plan = eng._plan(bb, 100, True, True)
    kinds = check_structure(eng, eng._last, full_plan, frozen)
    print(f"[bf16 {pattern}] launches by kind {kinds}")
    # which weight gradients lost their partner: the members of the full plan's pairs exactly one of which is still launched
    pruned = set(rep["pruned"])
    lone = set()
    for blk, n in (("encoder", 2), ("decoder", 2)):
        for i in range(n):
            p = f"{blk}.{i}"
            pairs = [(p + ".mlp.down_proj", p + ".mlp.up_proj"), (p + ".attn.out_proj", p + ".attn.qkv")]
            pairs += [(p + ".cross_attn.out_proj", p + ".cross_attn.query")] if blk == "decoder" else []
            for a, b in pairs:
                if (a in pruned) != (b in pruned):
                    lone.add(b if a in pruned else a)
    assert (kinds["survivor"] > 0) == bool(lone)
    if pattern == "down_proj_frozen_everywhere":
        assert lone == {f"{blk}.{i}.mlp.up_proj" for blk in ("encoder", "decoder") for i in range(2)}
    for k in names:
        if k in frozen:
            continue
        a, b = span(eng, k)
        owner = next((w for w in lone if k in eng_group_names(eng, w)), None)
        want = tw["0" if owner else "1"][0]
        E.check_exact(raw(eng.G[a:b]), raw(want[a:b]), f"bf16 {pattern}: gradient of {k}" + (" (lost its partner: MMFM_DW_PAIR=0)" if owner else ""))


def eng_group_names(eng, wname):
    """The parameters the weight-gradient group of the norm-fed or plain linear `wname` writes."""
    from multi_modal_foundation_model_amd.plan import PlanBuilder
    lin = next(l for l in eng.linears if l.name == wname)
    pb = PlanBuilder.__new__(PlanBuilder)
    pb.e, pb.parts = eng, {l.name: l.parts for l in eng.linears if l.parts}
    return pb.lin_names(wname) + (pb.norm_names(lin.norm) if lin.norm else [])


# ------------------------------------------------------------------------------------------------ bf16, the batched slab reduction
BATCHED = {
    "h_dec1_down_proj": PATTERNS["h_dec1_down_proj"],
    # the first product of every block segment leaves: the products behind it keep their slab regions
    "down_proj_frozen_everywhere": (["*.mlp.down_proj.*"], False),
    # the first norm-fed fused linear of every decoder segment leaves (the MLP is un-fused at this size): the sites behind it, cross_attn.kv
    # and attn.qkv, keep their reduced buffers (ws/gdb/{i})
    "cross_query_group_frozen_everywhere": (["*.cross_attn.query.*", "*.query_norm.*"], False),
}


@pytest.mark.parametrize("pattern", list(BATCHED))
def test_bf16_pruned_step_in_the_batched_reduction_regime(pattern, monkeypatch):
    """B = 16 at T = 100 (R = 3,200 <= 8,192): every weight gradient keeps its own slab region and ONE mmfm_reduce_slabs_multi per segment
    sums them, with mmfm_ln_linear_grad behind it.  A pruned product still takes its region and its reduced buffer's index, so the
    survivors keep the all-trainable arguments and the table is a sub-sequence of the full one's; no pairs here, so every trainable
    gradient is the all-trainable twin's bit for bit."""
    for k in PS.SWITCHES + PS.AUTO:
        monkeypatch.delenv(k, raising=False)
    bb, mc = 16, model_config(n_enc=2, n_dec=2, dropout=0.1, emb_dropout=0.1)
    step = lambda m: fwd_bwd(m, 0, bb, 100, 668)
    if "B16" not in _BF:
        twin = fresh(mc, "bf16", n_ap=668)
        step(twin)
        rec = LR.regime_record(twin._engine, twin._engine._last)
        assert rec["decisions"]["batch_red"] and not rec["decisions"]["pair_ok"]
        assert sum(names.count("mmfm_reduce_slabs_multi") for names in rec["names"].values()) == 7          # one per backward segment
        _BF["B16"] = twin._engine.G.clone()
    model = fresh(mc, "bf16", n_ap=668)
    names = list(dict(model.named_parameters()))
    frozen = split(names, *BATCHED[pattern])
    freeze(model, frozen)
    step(model)
    eng = model._engine
    print(f"[bf16 batched {pattern}] {eng.backward_summary(bb, 100)}")
    kinds = check_structure(eng, eng._last, eng._plan(bb, 100, True, True), frozen)
    print(f"[bf16 batched {pattern}] launches by kind {kinds}")
    assert kinds["table"] > 0 and kinds["survivor"] == 0
    for k in names:
        if k not in frozen:
            a, b = span(eng, k)
            E.check_exact(raw(eng.G[a:b]), raw(_BF["B16"][a:b]), f"bf16 batched {pattern}: gradient of {k}")
