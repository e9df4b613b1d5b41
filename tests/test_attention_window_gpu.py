"""The attention window over time stamps (MMFM_ATTN_WINDOW) on every kernel family that takes it, element by element against fp64
(tests/attn_refs.py at its derived per-element bounds, tests/context_window_refs.py for the rule):

  (a) the mask read-out: single-pair inputs show allowed(q, k) itself - o and dv nonzero EXACTLY where
      (DIAG && q == k) | (keypad[b][k] && lo <= pos[b][k] - pos[b][q] <= hi) holds, dq and dk exactly 0 where it does not;
  (b) attn_refs.random_inputs (x 6 keys) against attn_fwd_ref / attn_bwd_ref, without and with drop_p (the multiplier read off the
      counter hash, as the dropout tests of the general families do);
  (c) the all-covering window against the same bounds as the dense launch of the same descriptor;
  (d) mmfm_attn_pos_prep bit for bit against torch.cat + clamp, uniform and segmented;
  (e) the refusals on the device path: no launch, outputs untouched.

Families: KEEPBIT_DH32 (the WIN instantiations of attention_fast.hip: L = 40 two key tiles, 72 three - the last query tile skips tile 0 -
200 and 224 the NKT = 7 forms; drop_p with the keep mask read out of the workspace), F32, F32_TILED, BF16 (dh 32 at an L the keep-bit
kernels do not take, dh 64 with a keep-bit workspace), BF16_TILED, each asserted through ops.attn_win_family in both directions.  Outputs start as NaN sentinels with guard rows behind them."""
import pytest
import torch

import attn_refs as AR
import context_window_refs as CW
import dropout_refs as DR

pytestmark = pytest.mark.gpu

GUARD = 4
B, HEADS = 2, 2


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pos(ops, ts):
    """int32 pos of the stamps ts [B, L] through mmfm_attn_pos_prep (one slot), checked bit for bit on the way."""
    Bn, L = ts.shape
    pos = torch.full((Bn, L), -12345, dtype=torch.int32, device="cuda")
    ops.attn_pos_prep(Bn, [L], [ts.cuda()], pos)
    torch.cuda.synchronize()
    assert torch.equal(pos.cpu(), CW.clamp_pos(ts))
    return pos


class WinLaunch:
    """One descriptor's forward + backward under a window (win None: the dense entry points) as run(q, k, v, d_o) -> dict over
    [B, heads, L, dh] tensors: NaN-filled outputs with guard rows, the family asserted in both directions."""

    def __init__(self, ops, fam, dt, Bn, heads, L, dh, flags, kp, pos, lo, hi, ws=False, drop_p=0.0, dense=False):
        from multi_modal_foundation_model_amd import _lib as Lb
        self.ops, self.Lb, self.fam = ops, Lb, fam
        self.dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        self.code = Lb.BF16 if dt == "bf16" else Lb.F32
        self.B, self.heads, self.L, self.dh, self.flags = Bn, heads, L, dh, flags
        self.H = heads * dh
        self.kp, self.pos = kp.cuda(), pos
        self.win = None if dense else ops.attn_window(pos, lo, hi)
        self.kb = torch.zeros(ops.attn_keepbits_bytes(Bn, heads, L, L), dtype=torch.uint8, device="cuda") if ws else None
        self.drop, self.mult_p, self.p = None, None, drop_p
        self.keepbit = fam.startswith("KEEPBIT")
        if drop_p > 0:
            assert ws or not self.keepbit
            self.state = torch.zeros(2, dtype=torch.int32, device="cuda")
            ops.rng_seed(self.state, 4321)
            self.drop = ops.dropout(self.state, 7, drop_p)
            if not self.keepbit:             # the general families hash: the multiplier is read off the counter hash, as the dropout tests do
                self.mult_p = DR.general_attn_multiplier(ops, self.state, 7, drop_p, self.dtype, dh, Bn, heads, L, L).double()
        self.what = f"window {fam} {dt} dh {dh} L {L} flags {flags} [{lo}, {hi}]" + (f" drop_p {drop_p}" if drop_p else "") + (" dense" if dense else "")

    def _rows(self, x):
        return x.transpose(1, 2).reshape(self.B * self.L, self.H).contiguous()

    def _out(self):
        return torch.full((self.B * self.L + GUARD, self.H), float("nan"), dtype=self.dtype, device="cuda")

    def _take(self, buf, name):
        n = self.B * self.L
        AR.assert_written(buf[:n], f"{self.what} {name}")
        nanbits = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device="cuda"))[0]
        assert bool((_bits(buf[n:]) == nanbits).all()), f"{self.what} {name}: guard rows written"
        return buf[:n].reshape(self.B, self.L, self.heads, self.dh).transpose(1, 2).contiguous()

    def __call__(self, q, k, v, d_o):
        ops, Lb, Bn, heads, L, dh, H = self.ops, self.Lb, self.B, self.heads, self.L, self.dh, self.H
        qb, kb_, vb, gb = self._rows(q), self._rows(k), self._rows(v), self._rows(d_o)
        o, dq, dk, dv = self._out(), self._out(), self._out(), self._out()
        lse = torch.full((Bn * heads * L + 64,), float("nan"), device="cuda")
        desc = ops.attn_desc(self.code, Bn, heads, L, L, dh, qb.data_ptr(), kb_.data_ptr(), vb.data_ptr(), H, H, H, o.data_ptr(), H, lse, self.kp,
                             None, self.flags, dh ** -0.5, drop_p=self.drop, d_o=gb.data_ptr(), lddo=H, dq=dq.data_ptr(), dk=dk.data_ptr(),
                             dv=dv.data_ptr(), lddq=H, lddk=H, lddv=H, keepbits=self.kb)
        want = getattr(Lb, "ATTN_FAMILY_" + self.fam)
        ff, fb = ops.attn_win_family(desc, self.win, False), ops.attn_win_family(desc, self.win, True)
        assert ff == want and fb & Lb.ATTN_FAMILY_MASK == want, f"{self.what}: families {ff} / {fb:#x}, expected {want}"
        ops.attn_win_fwd(desc, self.win)
        if self.keepbit and self.p > 0:      # the keep-bit family: the keep mask is read out of the workspace the forward wrote
            torch.cuda.synchronize()
            mult = DR.unpack_keepbits(self.kb, Bn, heads, L, L).cuda().double() / ops.attn_keep_prob(self.p)
            ntile = Bn * heads * ((L + 31) // 32) ** 2 * 128
            if self.mult_p is None:
                self.mult_p, self.tiles = mult, self.kb[:ntile].clone()
            assert torch.equal(self.kb[:ntile], self.tiles), f"{self.what}: the keep bits changed between launches"
        ops.attn_win_bwd(desc, self.win)
        torch.cuda.synchronize()
        out = dict(o=self._take(o, "o"), dq=self._take(dq, "dq"), dk=self._take(dk, "dk"), dv=self._take(dv, "dv"))
        AR.assert_written(lse[:Bn * heads * L], f"{self.what} lse")
        assert bool(torch.isnan(lse[Bn * heads * L:]).all()), f"{self.what} lse: guard written"
        out["lse"] = lse[:Bn * heads * L].view(Bn, heads, L).clone()
        if self.mult_p is not None:
            out["mult_p"] = self.mult_p
        return out


# (family, dtype, dh, keep-bit workspace, L).  L = 40: two key tiles, the last with one 8-key group; 72: three tiles; 200 / 224: seven tiles,
# the model's shape; F32_TILED / BF16_TILED reached by shape as in attn_refs.SHAPES (fp32 dh 64 L 600; dh 128 always).
CASES = [("F32", "f32", 32, False, 40), ("F32", "f32", 32, False, 72), ("F32", "f32", 32, False, 200), ("F32_TILED", "f32", 64, False, 600),
         ("KEEPBIT_DH32", "bf16", 32, True, 40), ("KEEPBIT_DH32", "bf16", 32, True, 72), ("KEEPBIT_DH32", "bf16", 32, True, 200),
         ("KEEPBIT_DH32", "bf16", 32, True, 224), ("BF16", "bf16", 32, False, 44),
         ("BF16", "bf16", 64, True, 72), ("BF16_TILED", "bf16", 128, False, 136)]
IDS = [f"{f}-{dt}-dh{dh}-L{L}{'-ws' if ws else ''}" for f, dt, dh, ws, L in CASES]
PADS = ("tile_start", "full_tile", "last5")


def _combos(L):
    """(window name, flags, lo, hi, stamp recipe, pad recipe): every window of context_window_refs.WINDOWS with the stamp and key-padding
    recipes rotating, plus the pinned ones: [-8, 0] on arange stamps (at L = 72 rows 40..63 have no allowed key in key tile 0) and the
    far window on arange.  DIAG is added where a combination would leave a query without a key (decided from the inputs alone)."""
    out = []
    for i, (name, flags, lo, hi) in enumerate(CW.WINDOWS):
        out.append((name, flags, lo, hi, CW.STAMP_RECIPES[i % len(CW.STAMP_RECIPES)], PADS[i % 3]))
    out += [("back8", 0, -8, 0, "arange", "tile_start"), ("far", 1, -40, -33, "arange", "last5"), ("pm3", 0, -3, 3, "two_mod", "full_tile"),
            ("causal_time", 0, -CW.INF, 0, "shuffled", "last5"), ("fwd5", 0, 0, 5, "huge", "tile_start")]
    return out


def _allowed(kp, flags, pos, lo, hi):
    al = DR.allowed_mask(kp, 0, kp.shape[1]) & CW.band(lo, hi, pos)
    if not bool(al.any(-1).all()):
        flags |= 1
    return flags, CW.window_allowed(kp, flags, pos, lo, hi)


@pytest.mark.parametrize("fam,dt,dh,ws,L", CASES, ids=IDS)
def test_window_readout(ops, fam, dt, dh, ws, L):
    """(a): o, lse and dv for every (q, k); dq and dk at L <= 72.  The long shapes read out a rotating third of the combinations."""
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    tensors = ("o_dv", "dq", "dk") if L <= 72 else ("o_dv",)
    combos = _combos(L)
    if L > 224:
        combos = combos[::4]
    for name, flags, lo, hi, rec, pad in combos:
        ts, kp = CW.stamps(rec, B, L), AR.keypad(B, L, pad)
        pos = _pos(ops, ts)
        flags, al = _allowed(kp, flags, pos.cpu(), lo, hi)
        run = WinLaunch(ops, fam, dt, B, HEADS, L, dh, flags, kp, pos, lo, hi, ws=ws)
        AR.readout(run, al.cuda(), B, HEADS, L, L, dh, dtype, AR.group_of(fam), f"{run.what} {name} {rec} {pad}", tensors=tensors, device="cuda")


@pytest.mark.parametrize("drop_p", [0.0, 0.4], ids=["nodrop", "drop"])
@pytest.mark.parametrize("fam,dt,dh,ws,L", CASES, ids=IDS)
def test_window_bounds_random(ops, fam, dt, dh, ws, L, drop_p):
    """(b): every tensor of forward and backward at the derived bounds, drop_p off and on."""
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    q, k, v, d_o = AR.random_inputs(B, HEADS, L, L, dh, dtype, "cuda")
    combos = _combos(L)
    if L > 224:
        combos = combos[1::4]
    for name, flags, lo, hi, rec, pad in combos:
        ts, kp = CW.stamps(rec, B, L), AR.keypad(B, L, pad)
        pos = _pos(ops, ts)
        flags, al = _allowed(kp, flags, pos.cpu(), lo, hi)
        run = WinLaunch(ops, fam, dt, B, HEADS, L, dh, flags, kp, pos, lo, hi, ws=ws, drop_p=drop_p)
        out = run(q, k, v, d_o)
        AR.check_all(out, q, k, v, d_o, al.cuda(), dh ** -0.5, AR.group_of(fam), f"{run.what} {name} {rec} {pad}", mult_p=out.get("mult_p"))


@pytest.mark.parametrize("fam,dt,dh,ws,L", [c for c in CASES if c[4] in (72, 200, 136)], ids=[i for c, i in zip(CASES, IDS) if c[4] in (72, 200, 136)])
def test_all_covering_window_like_dense(ops, fam, dt, dh, ws, L):
    """(c): the all-covering window and the dense launch of the same general family meet the SAME bounds (they are not bit-compared: the
    window launch never takes the mask-free shortcut).  Dense launches of these descriptors run without a workspace, on the same family."""
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    q, k, v, d_o = AR.random_inputs(B, HEADS, L, L, dh, dtype, "cuda")
    kp = AR.keypad(B, L, "last5")
    pos = _pos(ops, CW.stamps("shift7", B, L))
    al = AR.build_allowed(kp, 0, L).cuda()
    assert torch.equal(al.cpu(), CW.window_allowed(kp, 0, pos.cpu(), -CW.INF, CW.INF))
    for lo, hi in ((-CW.INF, CW.INF), (-(1 << 31) + 1, (1 << 31) - 1)):             # the second: clamped to +-2^30 by the call
        run = WinLaunch(ops, fam, dt, B, HEADS, L, dh, 0, kp, pos, lo, hi, ws=ws)
        AR.check_all(run(q, k, v, d_o), q, k, v, d_o, al, dh ** -0.5, AR.group_of(fam), run.what)
    dense = WinLaunch(ops, fam, dt, B, HEADS, L, dh, 0, kp, pos, 0, 0, ws=ws and dh == 32, dense=True)
    AR.check_all(dense(q, k, v, d_o), q, k, v, d_o, al, dh ** -0.5, AR.group_of(fam), dense.what)


@pytest.mark.parametrize("L", [40, 72, 200, 224])
def test_keepbit_window_readout_with_dropout(ops, L):
    """The DROP WIN instantiations of the keep-bit family: the keep bits are read from the workspace, o and dv are nonzero exactly where
    allowed & keep holds.  Among the combinations: [-8, 0] on arange stamps (L = 72: rows 40..63 have no allowed key in key tile 0, the
    reference-exponent case), shuffled stamps through the tile classification, a far window that skips the tiles next to the diagonal."""
    for name, flags, lo, hi, rec, pad in _combos(L)[8:] + _combos(L)[3:6]:
        ts, kp = CW.stamps(rec, B, L), AR.keypad(B, L, pad)
        pos = _pos(ops, ts)
        flags, al = _allowed(kp, flags, pos.cpu(), lo, hi)
        run = WinLaunch(ops, "KEEPBIT_DH32", "bf16", B, HEADS, L, 32, flags, kp, pos, lo, hi, ws=True, drop_p=0.4)
        AR.readout(run, al.cuda(), B, HEADS, L, L, 32, torch.bfloat16, "bf16", f"{run.what} {name} {rec} {pad}", tensors=("o_dv",), device="cuda")


def test_pos_prep_uniform_and_segmented(ops):
    """(d): bit-exact against torch.cat + clamp: the uniform form (one shared stamp tensor passed M times), segments of different length
    with per-sample shifted stamps, stamps beyond +-2^29, more than one block (B * L > 256) and the slot limit."""
    Bn = 3
    shared = CW.stamps("shift7", Bn, 100).cuda()
    pos = torch.full((Bn, 200), -1, dtype=torch.int32, device="cuda")
    ops.attn_pos_prep(Bn, [100, 100], [shared, shared], pos)
    assert torch.equal(pos, torch.cat([shared, shared], 1).to(torch.int32))
    Ts = [8, 5, 37, 23, 1, 64, 3, 200]
    seg = [(CW.stamps("huge" if j % 3 == 0 else "shift7", Bn, T) - (j % 2) * 11).cuda() for j, T in enumerate(Ts)]
    for M in (1, 2, 5, 8):
        Lt = sum(Ts[:M])
        pos = torch.full((Bn * Lt + 8,), -1, dtype=torch.int32, device="cuda")
        ops.attn_pos_prep(Bn, Ts[:M], seg[:M], pos[:Bn * Lt].view(Bn, Lt))
        want = torch.cat(seg[:M], 1).clamp(-CW.POS_CLAMP, CW.POS_CLAMP).to(torch.int32)
        assert torch.equal(pos[:Bn * Lt].view(Bn, Lt), want), M
        assert bool((pos[Bn * Lt:] == -1).all()), "written behind the buffer"


def test_refusals_launch_nothing(ops):
    """(e): Lq != Lk, CAUSAL, SEP and a NULL pos raise with a message, for both directions, and leave the outputs alone."""
    from multi_modal_foundation_model_amd import _lib as Lb
    L, dh = 40, 32
    H = HEADS * dh
    x = torch.zeros(B * L, H, device="cuda")
    o = torch.full((B * L, H), float("nan"), device="cuda")
    lse = torch.full((B * HEADS * L,), float("nan"), device="cuda")
    kp = torch.ones(B, L, dtype=torch.uint8, device="cuda")
    mod = torch.zeros(L, dtype=torch.uint8, device="cuda")
    pos = torch.zeros(B, L, dtype=torch.int32, device="cuda")
    win = ops.attn_window(pos, -1, 1)
    null = Lb.AttnWindow(None, -1, 1)

    def desc(Lq, flags):
        return ops.attn_desc(Lb.F32, B, HEADS, Lq, L, dh, x.data_ptr(), x.data_ptr(), x.data_ptr(), H, H, H, o.data_ptr(), H, lse, kp, mod, flags,
                             dh ** -0.5, d_o=x.data_ptr(), lddo=H, dq=o.data_ptr(), dk=o.data_ptr(), dv=o.data_ptr(), lddq=H, lddk=H, lddv=H)
    for d, w, word in ((desc(32, 0), win, "Lq == Lk"), (desc(L, 2), win, "CAUSAL"), (desc(L, 4), win, "CAUSAL / SEP"), (desc(L, 0), null, "pos")):
        for fn in (ops.attn_win_fwd, ops.attn_win_bwd):
            with pytest.raises(Lb.MmfmError, match=word):
                fn(d, w)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(lse).all())
