"""Every attention kernel family, element by element against fp64 (tests/attn_refs.py):

  (a) the mask read-out: single-pair inputs show allowed(q, k) itself - o and dv nonzero EXACTLY where the rule of include/mmfm.h allows
      the pair, dq and dk exactly 0 where it does not - for all 8 flag combinations, every mod_id recipe under SEP (boundaries inside a
      tile, on a tile edge, alternating tiles, every tile mixed, a uniform ragged last tile) and every key-padding recipe;
  (b) per-element derived bounds on random inputs (the inputs of test_attention_masks_gpu.py plus a sample whose first key tile holds the row
      maxima): o and lse against attn_fwd_ref, dq / dk / dv against attn_bwd_ref fed the kernel's own stored o and lse.

Every launch asserts its kernel family (and BWD_SINGLE) in both directions through ops.attn_family; families are reached through shapes,
dtype and the workspace only.  Outputs start as NaN sentinels with guard rows behind them, padded leading dimensions carry NaN in the
pads of the inputs: every output element must be written, pads and guards must stay untouched.  B = 3, heads = 3 (9 workgroups:
attn_xcd_remap with q = 1, r = 1), plus one B = 1, heads = 2 and one padded-leading-dimension case per family.  No element is excluded and no
norm is taken.  The worst err / bound per family and tensor is printed by the last test (DESIGN.md records it)."""
import pytest
import torch

import attn_refs as AR
import dropout_refs as DR

pytestmark = pytest.mark.gpu

GUARD = 4                   # sentinel rows behind every output
WORST = {}                  # (family name, tensor) -> worst err / bound over everything this file ran


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Launch:
    """One descriptor's forward + backward as `run(q, k, v, d_o) -> dict` over [B, heads, L, dh] tensors: packs them into [B * L, ld] rows (NaN in
    the pad columns), launches into NaN-filled outputs with guard rows, asserts the family, and checks sentinels, pads and guards."""

    def __init__(self, ops, fam, single, dt, B, heads, Lq, Lk, dh, flags, kp, mod, ws, pad_ld=False, drop_p=0.0):
        from multi_modal_foundation_model_amd import _lib as Lb
        self.ops, self.Lb = ops, Lb
        self.fam, self.single = fam, single
        self.dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        self.code = Lb.BF16 if dt == "bf16" else Lb.F32
        self.B, self.heads, self.Lq, self.Lk, self.dh, self.flags = B, heads, Lq, Lk, dh, flags
        self.H = heads * dh
        self.ld = self.H + (8 if pad_ld else 0)
        self.kp, self.mod = kp.cuda(), (None if mod is None else mod.cuda())
        self.kb = torch.zeros(ops.attn_keepbits_bytes(B, heads, Lq, Lk), dtype=torch.uint8, device="cuda") if (ws or drop_p > 0) else None
        self.p, self.drop, self.mult_p, self.tiles = drop_p, None, None, None
        if drop_p > 0:
            self.state = torch.zeros(2, dtype=torch.int32, device="cuda")
            ops.rng_seed(self.state, 4321)
            self.drop = ops.dropout(self.state, 7, drop_p)
        self.what = f"{fam} {dt} dh {dh} B {B} heads {heads} L {Lq}x{Lk} flags {flags} ld {self.ld}" + (f" drop_p {drop_p}" if drop_p else "")

    def _rows(self, x, L):                      # [B, heads, L, dh] -> [B * L, ld], NaN pads
        buf = torch.full((self.B * L, self.ld), float("nan"), dtype=self.dtype, device="cuda")
        buf[:, :self.H] = x.transpose(1, 2).reshape(self.B * L, self.H)
        return buf

    def _out(self, L):
        return torch.full((self.B * L + GUARD, self.ld), float("nan"), dtype=self.dtype, device="cuda")

    def _take(self, buf, L, name):              # sentinels, pads and guards, then [B * L, ld] -> [B, heads, L, dh]
        body = buf[:self.B * L]
        AR.assert_written(body[:, :self.H], f"{self.what} {name}")
        nanbits = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device="cuda"))[0]
        assert bool((_bits(buf[self.B * L:]) == nanbits).all()), f"{self.what} {name}: guard rows written"
        assert bool((_bits(body[:, self.H:].contiguous()) == nanbits).all()), f"{self.what} {name}: pad columns written"
        return body[:, :self.H].reshape(self.B, L, self.heads, self.dh).transpose(1, 2).contiguous()

    def __call__(self, q, k, v, d_o):
        ops, Lb, B, heads, Lq, Lk, dh, ld = self.ops, self.Lb, self.B, self.heads, self.Lq, self.Lk, self.dh, self.ld
        qb, kb_, vb, gb = self._rows(q, Lq), self._rows(k, Lk), self._rows(v, Lk), self._rows(d_o, Lq)
        o, dq, dk, dv = self._out(Lq), self._out(Lq), self._out(Lk), self._out(Lk)
        lse = torch.full((B * heads * Lq + 64,), float("nan"), device="cuda")
        desc = ops.attn_desc(self.code, B, heads, Lq, Lk, dh, qb.data_ptr(), kb_.data_ptr(), vb.data_ptr(), ld, ld, ld, o.data_ptr(), ld, lse, self.kp,
                             self.mod, self.flags, dh ** -0.5, drop_p=self.drop, d_o=gb.data_ptr(), lddo=ld, dq=dq.data_ptr(), dk=dk.data_ptr(),
                             dv=dv.data_ptr(), lddq=ld, lddk=ld, lddv=ld, keepbits=self.kb)
        want = getattr(Lb, "ATTN_FAMILY_" + self.fam)
        assert ops.attn_family(desc, False) == want, f"{self.what}: forward family {ops.attn_family(desc, False)}"
        assert ops.attn_family(desc, True) == want | (Lb.ATTN_FAMILY_BWD_SINGLE if self.single else 0), f"{self.what}: backward family {ops.attn_family(desc, True):#x}"
        ops.attn_fwd(desc)
        out = {}
        if self.p > 0:
            ntile = B * heads * ((Lq + 31) // 32) * ((Lk + 31) // 32) * 128
            if self.mult_p is None:                  # the bits are a function of (state, site, position): every launch draws the same
                self.tiles = self.kb[:ntile].clone()
                self.mult_p = DR.unpack_keepbits(self.kb, B, heads, Lq, Lk).cuda().double() / ops.attn_keep_prob(self.p)
            assert torch.equal(self.kb[:ntile], self.tiles), f"{self.what}: the keep bits changed between launches"
            out["mult_p"] = self.mult_p
        ops.attn_bwd(desc)
        torch.cuda.synchronize()
        out.update(o=self._take(o, Lq, "o"), dq=self._take(dq, Lq, "dq"), dk=self._take(dk, Lk, "dk"), dv=self._take(dv, Lk, "dv"))
        AR.assert_written(lse[:B * heads * Lq], f"{self.what} lse")
        assert bool(torch.isnan(lse[B * heads * Lq:]).all()), f"{self.what} lse: guard written"
        out["lse"] = lse[:B * heads * Lq].view(B, heads, Lq).clone()
        return out


def _note(fam, ratios):
    for n, x in ratios.items():
        WORST[(fam, n)] = max(WORST.get((fam, n), 0.0), x)


def _cases():
    for fam, dt, dh, ws, shapes, _ in AR.SHAPES:
        for sh in shapes:
            yield pytest.param(fam, dt, dh, ws, sh, id=f"{fam}-{dt}-dh{dh}-{sh if isinstance(sh, int) else 'x'.join(map(str, sh))}")


def _readout_combos(Lq, Lk, dh):
    """(flags, mod recipe, pad recipe): all 8 flag combinations, every mod_id recipe under SEP, every key-padding recipe (rotating; all of
    them with DIAG alone and with DIAG | SEP, where the padding and the diagonal meet).  Cross shapes: flags 0.  L = 1100: flags 0 and 4."""
    pads = AR.PAD_RECIPES
    if Lq != Lk:
        return [(0, None, p) for p in pads]
    if Lq >= 1000:
        return [(0, None, "last5"), (4, "aligned", "tile_start")]
    out, i = [], 0
    for flags in range(8):
        recs = AR.MOD_RECIPES if flags & 4 else (None,)
        if Lq >= 400:                                            # the long shapes: one recipe per flag combination, rotating
            recs = (AR.MOD_RECIPES[flags % 5],) if flags & 4 else (None,)
        for rec in recs:
            out.append((flags, rec, pads[i % 4] if not flags & 4 else pads[i % 5]))
            i += 1
    out += [(1, None, p) for p in pads[:4]] + [(5, "aligned", p) for p in pads]
    return out


@pytest.mark.parametrize("fam,dt,dh,ws,shape", list(_cases()))
def test_mask_readout(ops, fam, dt, dh, ws, shape):
    """(a): o, lse and dv for every (q, k); dq and dk at L <= 264."""
    B, heads = 3, 3
    Lq, Lk = (shape, shape) if isinstance(shape, int) else shape
    name, single = AR.expected_family(fam, dt, dh, shape)
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    tensors = ("o_dv", "dq", "dk") if max(Lq, Lk) <= 264 else ("o_dv",)
    for flags, rec, pad in _readout_combos(Lq, Lk, dh):
        mod = AR.mod_id(Lq, rec) if rec else None
        kp = AR.keypad(B, Lk, pad)
        al = AR.build_allowed(kp, flags, Lq, mod).cuda()
        run = Launch(ops, name, single, dt, B, heads, Lq, Lk, dh, flags, kp, mod, ws)
        _note(name, AR.readout(run, al, B, heads, Lq, Lk, dh, dtype, AR.group_of(name), f"{run.what} {rec} {pad}", tensors=tensors, device="cuda"))


@pytest.mark.parametrize("fam,dh,L", [(f, dh, L) for f, dh in (("KEEPBIT_DH32", 32), ("KEEPBIT_LONG", 64), ("KEEPBIT_LONG", 128)) for L in (136, 200)])
def test_mask_readout_with_dropout(ops, fam, dh, L):
    """The DROP instantiations of the keep-bit families: the keep bits are read from the workspace, nonzero is exactly allowed & keep."""
    B, heads = 3, 3
    for flags, rec, pad in [(0, None, "last5"), (5, "aligned", "tile_start"), (6, "blocks32", "tile_end"), (7, "inside", "full_tile"), (4, "ragged_last", "headpad")]:
        mod = AR.mod_id(L, rec) if rec else None
        kp = AR.keypad(B, L, pad)
        al = AR.build_allowed(kp, flags, L, mod).cuda()
        run = Launch(ops, fam, False, "bf16", B, heads, L, L, dh, flags, kp, mod, True, drop_p=0.4)
        _note(fam, AR.readout(run, al, B, heads, L, L, dh, torch.bfloat16, "bf16", f"{run.what} {rec} {pad}", tensors=("o_dv",), device="cuda"))


def _random_case(ops, name, single, dt, B, heads, Lq, Lk, dh, ws, flags, rec, pad, pad_ld=False):
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    mod = AR.mod_id(Lq, rec) if rec else None
    kp = AR.keypad(B, Lk, pad)
    al = AR.build_allowed(kp, flags, Lq, mod).cuda()
    q, k, v, d_o = AR.random_inputs(B, heads, Lq, Lk, dh, dtype, "cuda")
    run = Launch(ops, name, single, dt, B, heads, Lq, Lk, dh, flags, kp, mod, ws, pad_ld=pad_ld)
    out = run(q, k, v, d_o)
    _note(name, AR.check_all(out, q, k, v, d_o, al, dh ** -0.5, AR.group_of(name), f"{run.what} {rec} {pad}"))


@pytest.mark.parametrize("fam,dt,dh,ws,shape", list(_cases()))
def test_bounds_random(ops, fam, dt, dh, ws, shape):
    """(b): flags {0, 1, 2, 5, 7}, recipes aligned / blocks32 / inside (cross shapes: flags 0; L = 1100: flags 0 and 4)."""
    Lq, Lk = (shape, shape) if isinstance(shape, int) else shape
    name, single = AR.expected_family(fam, dt, dh, shape)
    for i, (flags, rec) in enumerate(AR.random_combos(Lq, Lk)):
        _random_case(ops, name, single, dt, 3, 3, Lq, Lk, dh, ws, flags, rec, AR.PAD_RECIPES[i % 4])


# one shape per family for the small grid and the padded leading dimension: (SHAPES family, dtype, dh, workspace, L)
REPS = [("KEEPBIT_DH32", "bf16", 32, False, 200), ("KEEPBIT_LONG", "bf16", 64, True, 136), ("KEEPBIT_LONG", "bf16", 128, True, 40),
        ("BF16", "bf16", 64, False, 70), ("BF16", "bf16", 32, False, 250), ("BF16_TILED", "bf16", 128, False, 129), ("F32", "bf16", 8, False, 16),
        ("F32", "f32", 32, False, 70), ("F32", "f32", 64, False, 600)]


@pytest.mark.parametrize("B,heads,pad_ld", [(1, 2, False), (3, 3, True)], ids=["B1h2", "ld+8"])
@pytest.mark.parametrize("fam,dt,dh,ws,L", REPS)
def test_small_grid_and_padded_ld(ops, fam, dt, dh, ws, L, B, heads, pad_ld):
    """B = 1, heads = 2 (two workgroups), and ld = heads * dh + 8 with NaN in the input pads: random inputs and one read-out each."""
    name, single = AR.expected_family(fam, dt, dh, L)
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    for flags, rec, pad in [(0, None, "last5"), (7, "inside", "tile_start")]:
        _random_case(ops, name, single, dt, B, heads, L, L, dh, ws, flags, rec, pad, pad_ld=pad_ld)
    mod, kp = AR.mod_id(L, "blocks32"), AR.keypad(B, L, "tile_end")
    al = AR.build_allowed(kp, 5, L, mod).cuda()
    run = Launch(ops, name, single, dt, B, heads, L, L, dh, 5, kp, mod, ws, pad_ld=pad_ld)
    tensors = ("o_dv", "dq", "dk") if L <= 264 else ("o_dv",)
    _note(name, AR.readout(run, al, B, heads, L, L, dh, dtype, AR.group_of(name), run.what, tensors=tensors, device="cuda"))


def test_zz_worst_ratios():
    """Prints the worst err / bound per family and tensor of everything above (run the file whole)."""
    for (fam, n), x in sorted(WORST.items()):
        print(f"[attn] worst err / bound  {fam:13s} {n:3s} {x:.3f}")
    assert all(x <= 1.0 for x in WORST.values())
