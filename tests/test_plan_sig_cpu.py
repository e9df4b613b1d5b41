"""tests/plan_sig.py on hand-made plans (CPU tensors, stand-in function objects with `__name__` and `argtypes`; no GPU, no library):
the signature does not see where buffers lie or in which order the pool was filled, and does see every integer, offset, dropout
site, struct field, table row and the order of the entries; a pointer into nothing raises."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import plan_sig as S
from multi_modal_foundation_model_amd import _lib as L

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_HOLD = []           # every tensor ever made stays alive, so a rebuilt plan cannot land on the addresses of an earlier one


def fn(name, *argtypes):
    return types.SimpleNamespace(__name__=name, argtypes=list(argtypes) + [_vp])     # + the stream


GEMM = fn("mmfm_gemm", C.POINTER(L.GemmDesc))
APPLY = fn("mmfm_dropout_apply", _i, _vp, _vp, _i64, _i, L.Dropout)
NORM = fn("mmfm_layernorm_fwd", _vp, _vp, _f)
REDUCE = fn("mmfm_reduce_slabs_multi", _vp, _i, _i)
MASKS = fn("mmfm_mask_prep", _i, C.POINTER(_vp), C.POINTER(_i64), _vp)


def make(reverse_pool=False, **mut):
    """A two-unit plan over freshly allocated buffers.  `mut` names one thing to change."""
    def t(n, dtype=torch.float32):
        x = torch.zeros(n, dtype=dtype)
        _HOLD.append(x)
        return x
    eng = types.SimpleNamespace(P=t(64), G=t(64), Pw=t(64, torch.bfloat16), rng=t(2, torch.int32), _prep=None, _wt=None)
    base = {k: t(32) for k in ("x", "slab", "dec0/cn/xh", "mask/0", "mask/1", "out")}
    items = list(base.items()) + [("dec1/cn/xh", base["dec0/cn/xh"])]          # two keys, one storage
    pool = dict(reversed(items) if reverse_pool else items)
    p = {k: v.data_ptr() for k, v in pool.items()}

    d = L.GemmDesc()
    d.dtype, d.M, d.N, d.K = L.BF16, 8, 4, mut.get("field", 16)
    d.A, d.B, d.C = p["x"] + mut.get("offset", 8), eng.Pw.data_ptr() + 2 * 8, p["slab"]
    d.colsum = p["slab"] + 4 * 16                 # a raw int, as the engine passes it
    d.act_scale = 0.1
    d.drop = L.Dropout(eng.rng.data_ptr(), mut.get("site", 3), 0.25)
    gemm = (GEMM, (C.byref(d),), (d,))

    apply_ = (APPLY, (L.BF16, p["dec1/cn/xh"], p["out"], mut.get("int_arg", 32), 4, L.Dropout(eng.rng.data_ptr(), 5, 0.5)), ())
    norm = (NORM, (eng.P.data_ptr() + 4 * 3, mut.get("null", None), 1e-5), ())

    rows = (L.ReduceEntry * 2)()
    for r, (dst, n) in zip(rows, ((eng.G.data_ptr(), 16), (eng.G.data_ptr() + 4 * 16, mut.get("table_field", 8)))):
        r.dst, r.src, r.n, r.slab_stride, r.nslabs = dst, p["slab"], n, 16, 2
    table = torch.from_numpy(np.frombuffer(bytes(rows), dtype=np.uint8).copy())
    _HOLD.append(table)
    reduce_ = (REDUCE, (table.data_ptr(), 2, 2), (table,))

    src = (_vp * 2)(p["mask/0"], p["mask/1"])
    st = (_i64 * 2)(1, 1)
    masks = (MASKS, (2, src, st, p["out"]), (src, st))

    seg = [apply_, norm] if mut.get("swap") else [norm, apply_]
    return eng, dict(fwd=[masks, gemm], bwd=[("head", seg), ("embed", [reduce_])], b=pool)


def hashes(eng_plan, **kw):
    return {u: v["sha256"] for u, v in S.plan_signature(*eng_plan, **kw).items()}


def test_units_and_names():
    sig = S.plan_signature(*make(), full=True)
    assert list(sig) == ["fwd", "bwd/head", "bwd/embed"]
    assert sig["fwd"]["names"] == ["mmfm_mask_prep", "mmfm_gemm"]
    gemm = sig["fwd"]["records"][1]
    assert gemm["args"] == ["ref"]
    desc = gemm["keep"][0]
    assert desc["A"] == ["b:x", 8] and desc["B"] == ["Pw", 16] and desc["colsum"] == ["b:slab", 64] and desc["bias"] is None
    assert desc["drop"] == dict(state=["rng", 0], site=3, p=(0.25).hex())
    assert desc["act_scale"] == float(np.float32(0.1)).hex() != (0.1).hex()        # the value the C float holds
    assert sig["fwd"]["records"][0]["keep"] == [[["b:mask/0", 0], ["b:mask/1", 0]], [1, 1]]
    norm, apply_ = sig["bwd/head"]["records"]
    assert norm["args"] == [["P", 12], None, float(np.float32(1e-5)).hex()]
    assert apply_["args"][1] == ["b:dec0/cn/xh", 0], "two keys on one storage: the smallest names it"
    assert apply_["args"][5] == dict(state=["rng", 0], site=5, p=(0.5).hex())
    table = sig["bwd/embed"]["records"][0]
    assert table["args"] == [["keep:0", 0], 2, 2]
    assert [r["dst"] for r in table["keep"][0]] == [["G", 0], ["G", 64]] and table["keep"][0][1]["n"] == 8


def test_addresses_and_pool_order_do_not_matter():
    a, b, c = make(), make(), make(reverse_pool=True)
    assert a[1]["b"]["x"].data_ptr() != b[1]["b"]["x"].data_ptr()
    assert list(a[1]["b"]) != list(c[1]["b"])
    assert hashes(a) == hashes(b) == hashes(c)
    assert S.plan_signature(*a, full=True) == S.plan_signature(*c, full=True)


@pytest.mark.parametrize("mut,unit", [(dict(int_arg=33), "bwd/head"), (dict(offset=12), "fwd"), (dict(site=4), "fwd"), (dict(field=17), "fwd"),
                                      (dict(table_field=9), "bwd/embed"), (dict(swap=True), "bwd/head")],
                         ids=["integer", "offset", "dropout_site", "struct_field", "table_row_field", "entry_order"])
def test_one_change_changes_the_signature(mut, unit):
    base, changed = hashes(make()), hashes(make(**mut))
    assert [u for u in base if base[u] != changed[u]] == [unit]
    if "swap" in mut:
        assert S.plan_signature(*make(**mut))[unit]["names"] == ["mmfm_dropout_apply", "mmfm_layernorm_fwd"]


def test_unresolvable_pointer_raises():
    stray = torch.zeros(4)                         # alive, but in no pool
    with pytest.raises(LookupError):
        S.plan_signature(*make(null=stray.data_ptr()))
    eng, plan = make()
    end = plan["b"]["out"]
    plan["fwd"].append((NORM, (end.data_ptr() + end.numel() * 4 + (1 << 40), None, 0.0), ()))
    with pytest.raises(LookupError):
        S.plan_signature(eng, plan)


def test_array_fields_of_a_descriptor_are_resolved_element_by_element():
    """mmfm_rowgemm_groups_desc holds its per-group operands as pointer arrays: each is an (owner, offset), NULL stays None, and moving
    one group's pointer changes the signature."""
    groups = fn("mmfm_rowgemm_groups", C.POINTER(L.RowGemmGroupsDesc))

    def with_groups(off):
        eng, plan = make()
        d = L.RowGemmGroupsDesc()
        d.R, d.K, d.N, d.groups = 32, 256, 512, 2
        d.x[0] = plan["b"]["x"].data_ptr()
        d.w[0], d.w[1] = eng.Pw.data_ptr(), eng.Pw.data_ptr() + off
        d.y[0], d.y[1] = plan["b"]["out"].data_ptr(), plan["b"]["slab"].data_ptr() + 16
        plan["fwd"].append((groups, (C.byref(d),), (d,)))
        return eng, plan
    rec = S.plan_signature(*with_groups(64), full=True)["fwd"]["records"][-1]["keep"][0]
    assert rec["w"] == [["Pw", 0], ["Pw", 64]] + [None] * (L.ROWGEMM_MAX_GROUPS - 2) and rec["bias"] == [None] * L.ROWGEMM_MAX_GROUPS
    assert rec["y"][:2] == [["b:out", 0], ["b:slab", 16]] and rec["x"][0] == ["b:x", 0] and rec["groups"] == 2
    assert hashes(with_groups(64))["fwd"] != hashes(with_groups(32))["fwd"] and hashes(with_groups(64)) == hashes(with_groups(64))


def test_argument_count_is_checked():
    eng, plan = make()
    plan["fwd"].append((NORM, (None, None), ()))
    with pytest.raises(TypeError):
        S.plan_signature(eng, plan)
