"""The step-plan builder: MultiModal forward / backward of one batch shape as lists of pre-bound HIP kernel launches.

`PlanBuilder(engine, B, T, training, grad).build()` returns the plan dict `Engine._plan` caches.  What is mutable while a plan is laid
out (the launch lists, the parked weight gradient, the pending slab reductions) lives in the builder; parameters, buffer pools, dropout
sites and the regime decisions (`_fused_mask`, `_dw_split`, `_w_transposed`) stay with the engine.  DESIGN.md §7b: layout, plan signature."""
from __future__ import annotations

import functools
import math
import os
from collections import namedtuple

import torch

from . import _lib as L
from . import ops as K


def _align(n, a=8):
    return (n + a - 1) // a * a


# The plan-time MMFM_* environment switches, read once when a plan is built.  fused: MMFM_FUSED as an int, None when it is
# not set (the shape decides: Engine._fused_mask); the others: False where the variable turns the path off
Switches = namedtuple("Switches", "fused gemm_big gemm_dw batch_reduce dw_pair attn_keepbits mlp_bwd_split")


def read_switches() -> Switches:
    env, on = os.environ, lambda k: os.environ.get(k, "1") != "0"
    return Switches(fused=int(env["MMFM_FUSED"]) if "MMFM_FUSED" in env else None, gemm_big=on("MMFM_GEMM_BIG"), gemm_dw=on("MMFM_GEMM_DW"),
                    batch_reduce=on("MMFM_BATCH_REDUCE"), dw_pair=on("MMFM_DW_PAIR"), attn_keepbits=on("MMFM_ATTN_KEEPBITS"),
                    mlp_bwd_split=env.get("MMFM_MLP_BWD_SPLIT", "1") == "1")


# Live rows: tokeniser rows (B * T per modality) from which a bf16 plan runs the tokeniser chains on the compact row space
# of the time bins sample 0 leaves unmasked.  Below it the chains are launch-bound and the plan stays what it was.  MMFM_LIVE_ROWS = 0
# turns the path off, 1 turns it on at any size
LIVE_ROWS_MIN = 16384


def live_rows_on(BT):
    v = os.environ.get("MMFM_LIVE_ROWS")
    return v == "1" if v in ("0", "1") else BT >= max(8192, LIVE_ROWS_MIN)


# Grouped context side: rows from which a bf16 plan on the fused norm + linear path projects the context to the keys / values
# of ALL decoder layers in one launch (mmfm_rowgemm_groups) and sums their dX products behind one norm backward at the head of the bridge
# segment.  Below it the per-layer launches stay, call for call.  MMFM_CTX_GROUP = 0 turns the path off, 1 turns it on at any size
CTX_GROUP_MIN = 16384
CTX_GROUP_BIAS = 2560       # floats of bias the grouped forward keeps in LDS: groups * N of one launch (csrc/rowgemm.hip, GBIAS_MAX)


# The du-only front half of the fused MLP backward (mmfm_mlp_bwd with t1 = g = NULL): what a pruned plan launches for
# an MLP block neither projection of which takes a gradient.  False: such a block passes real t1 / g buffers, as the full plan does
MLP_DX_ONLY = True


def ctx_group_on(R):
    v = os.environ.get("MMFM_CTX_GROUP")
    return v == "1" if v in ("0", "1") else R >= CTX_GROUP_MIN


# What a side of the model lays its blocks out with (EngineConfig.side, in this plan's mode): heads, I = inter_size, dp / dpe = the
# transformer's / the embedder's dropout (0 outside training), act = (MMFM_MLP_* kind, beta) with act_fwd / act_grad the un-fused MLP's
# mmfm_gemm act codes, the embedder's scale, mult, max_F, activation codes (emb_fwd / emb_grad) and pos, and - set by `workspaces` - use_keep (attention dropout of this side runs
# on keep-bit workspaces) and F_MLP (its MLP blocks run the row-owner MLP kernels)
class Side:
    def __init__(self, sc, training):
        self.heads, self.I, self.act, self.scale, self.mult, self.max_F = sc.heads, sc.inter, sc.act, sc.embed_scale, sc.mult, sc.max_F
        self.dp, self.dpe = (sc.dropout, sc.embed_dropout) if training else (0.0, 0.0)
        self.act_fwd, self.act_grad = K.GEMM_ACTS[sc.act[0]]
        # the embedder's options: its activation's mmfm_gemm codes (ops.EMBED_ACTS), pos (False: no position table) and whether
        # token_embed has a bias (the layout decides what the launches get: Engine.Pb / Gb)
        self.emb_act, self.pos = sc.embed_act, sc.embed_pos
        self.emb_fwd, self.emb_grad = K.embed_act(sc.embed_act)
        self.use_keep = self.F_MLP = False


def elem_buf(which, m, shape):
    """The pool key of modality m's static element-mask buffer ("cm" / "tm") of compact shape `shape`: one buffer per broadcast pattern."""
    return f"{which}/{m}/{'x'.join(str(int(s)) for s in shape)}"


def chan_buf(m, shape):
    """The pool key of modality m's static channel-mask buffer (u8 [B or 1, N]; 1 = a real channel): one buffer per shape, as `elem_buf`."""
    return f"chan/{m}/{'x'.join(str(int(s)) for s in shape)}"


def combine_chan(entry, v, B, T, N):
    """A modality's element masks under its channel mask v (u8 [B or 1, N], 1 = a real channel; neuron padding), on
    whatever device the tensors live: pure tensor arithmetic on compact shapes, nothing is expanded beyond what the result needs.
    entry: None or (cm, tm, corrupted or None), the masks u8 [B or 1, T or 1, N or 1] (Masker.element_masks).  Returns (entry', chan):
      cm'   - what mmfm_stage_masked zeroes.  Where the engine does the masker's zeroing (corrupted is None): cm | (1 - v)[:, None, :],
              the masker's elements and every padded channel; its shape is the broadcast of the two, so a [B,T,1] / [1,T,1]
              corruption mask becomes [B,T,N] (for staging only).  Where the masker corrupted the inputs itself (`corrupted`: noise
              and kept values under cm, zero_ratio < 1): (1 - v)[:, None, :] alone - only the padded channels of `corrupted` go;
      tm'   - no entry: None, the row mask is the plan's token mask and the loss runs the chan form (chan = v);
            - tm [B,T,1] / [1,T,1]: tm itself, the row mask of the chan form (chan = v);
            - any other tm (it carries the channel axis, or is one value per sample): tm & v[:, None, :] in compact form, the loss runs
              the element form under the resulting shape (chan = None)."""
    if v.dtype != torch.uint8 or v.dim() != 2 or v.shape[1] != N or v.shape[0] not in (1, B):
        raise ValueError(f"channel mask: a uint8 tensor of shape [{B} or 1, {N}], got {v.dtype} {tuple(v.shape)}")
    v = v.contiguous()
    pad = (1 - v)[:, None, :]
    if entry is None:
        return (pad.contiguous(), None, None), v
    cm, tm, corrupted = entry
    cm2 = (cm | pad).contiguous() if corrupted is None else pad.contiguous()
    if tm.shape[1] == T and tm.shape[2] == 1:
        return (cm2, tm, corrupted), v
    return (cm2, (tm & v[:, None, :]).contiguous(), corrupted), None


def mask_key(elem, chan):
    """What a plan is keyed by for its masks: `elem` (Engine.elem_key) alone - today's key, None included - while no modality carries a
    channel mask, else both keys behind a tag that no elem key starts with."""
    return elem if chan is None else ("chan", elem, chan)


class PlanBuilder:
    def __init__(self, engine, B, T, training, grad=True, frozen=None, elem=None, chan=None):
        """frozen: the names (layout entries) of the parameters with requires_grad = False, or None / empty: everything is trainable and
        the plan is the one it always was.  With frozen parameters the backward is pruned to what the others need.
        elem (Engine.elem_key; None: the plan it always was): per modality None or the compact shapes of its (corruption, target)
        element masks.  Such a decoder modality's loss launches are mmfm_masked_loss_elem_* on its static target-mask buffer; they write
        the modality's count behind mmfm_mask_prep.  Everything upstream of the heads is unchanged.
        chan (Engine.chan_key; None: the plan it always was): per modality None or the shape of its channel mask.  Such a decoder
        modality's loss launches are mmfm_masked_loss_chan_* on its static channel-mask buffer and its row mask - the token mask, or
        the [B,T,1] / [1,T,1] target mask where `elem` gives it one (its elem entry then has a corruption mask for staging and, in
        the first case, no target mask: `combine_chan`).  DESIGN.md §3x."""
        e, c = self.e, self.c = engine, engine.cfg
        self.elem, self.chan = elem, chan
        self.B, self.T, self.training, self.grad = B, T, bool(training), bool(grad)
        self.frozen = frozenset(frozen) if frozen else None
        self.groups = {}             # gradient group -> (its launches are emitted, the parameters whose gradients they write) (`keep`)
        self.parts = {l.name: l.parts for l in e.linears if l.parts}
        self.sw = read_switches()
        # each side's modalities (EngineConfig.side_mods: index in cfg.mods, name, channels).  A modality's place in its side's list is
        # its slot in that side's stitched sequence; its index in cfg.mods names its buffers and is its mod_emb row.  M counts a side's
        # modalities: both sides have as many (cross-attention pairs the two sequences position for position, mm.py:152-158, 210)
        self.mods_of = {side: c.side_mods(side) for side in ("encoder", "decoder")}
        self.H, self.M = c.hidden, len(self.mods_of["encoder"])
        # T: one length for every modality, or a tuple of per-modality lengths in cfg.mods order - a segmented plan:
        # slot j of a side's stitched sequence starts at off[side][j], each modality has its own stamps and attention mask
        # (ts/{m}, attn/{m}) and the edges run the mmfm_*_seg entry points.  Tm[m] / BTm[m]: bins / tokeniser rows of modality m
        self.seg = isinstance(T, tuple)
        if self.seg and (len(T) != len(c.mods) or any(int(t) < 1 for t in T)):
            raise ValueError(f"engine: per-modality lengths {T}: one positive length per modality of {[m for m, _ in c.mods]}")
        self.Tm = {m: int(T[m]) if self.seg else T for m in range(len(c.mods))}
        self.BTm = {m: B * t for m, t in self.Tm.items()}
        self.off = {}
        for side, mods in self.mods_of.items():
            self.off[side] = [0]
            for m, _, _ in mods:
                self.off[side].append(self.off[side][-1] + self.Tm[m])
        if self.seg:
            if len(self.mods_of["decoder"]) > L.MAX_SEGMENTS or self.M > L.MAX_SEGMENTS:
                raise NotImplementedError(f"engine: a segmented plan holds at most {L.MAX_SEGMENTS} modalities per side")
            if self.off["encoder"][-1] != self.off["decoder"][-1]:
                raise RuntimeError(f"engine: the encoder's sequence has {self.off['encoder'][-1]} tokens, the decoder's "
                                   f"{self.off['decoder'][-1]}: cross-attention needs the two lengths equal")
        elif len(self.mods_of["decoder"]) != self.M:
            raise RuntimeError(f"engine: the encoder's sequence has {self.M * T} tokens ({self.M} modalities x {T}), the decoder's "
                               f"{len(self.mods_of['decoder']) * T}: cross-attention needs the two lengths equal")
        self.Lq = self.off["encoder"][-1]
        self.R = B * self.Lq
        # BT: the rows of a tokeniser (uniform) / of the longest one (segmented: what sizes a workspace every modality uses)
        self.BT = max(self.BTm[m] for mods in self.mods_of.values() for m, _, _ in mods) if self.seg else B * T
        self.Md = len(self.mods_of["decoder"])         # the decoder's modalities: M, unless a segmented plan's sides split their bins differently
        # the mask products (tokmask / keypad / keep0 / mod_id / count) come from the side's own modalities' masks: one buffer set while
        # the two sides have the same modalities, else the decoder's own under "dec/"
        self.split_masks = [m for m, _, _ in self.mods_of["encoder"]] != [m for m, _, _ in self.mods_of["decoder"]]
        # EngineConfig.per_sample_mask: per side, keep [B, Lq] - every sample's own row - and keep_any [Lq], their OR, stand
        # where keep0 [Lq] stands; the mask launch is mmfm_mask_prep_rows, the stitch launches the _rows pair, and the live-bin records
        # come from keep_any.  False: no buffer, launch or argument of the plan differs from what it always was
        self.per_sample = bool(getattr(c, "per_sample_mask", False))
        self.staged = sorted({m for side in self.mods_of.values() for m, _, _ in side})      # modalities some side uses
        self.sides = {side: Side(c.side(side), training) for side in ("encoder", "decoder")}
        # stitched modalities (EngineConfig.sessions): st[m] = the neuron counts of m's sessions.  Such a modality's inputs,
        # targets and predictions are nd[m] = max(st[m]) wide, its tokenisers and its head run at the shared width c.mods[m][1]
        self.st = {m: c.stitched(m) for m in self.staged if c.stitched(m)}
        self.nd = {m: c.data_width(m) for m in range(len(c.mods))}
        for m in self.st:
            if c.loss_kind.get(c.mods[m][0]) == L.LOSS_SOFTMAX_CE:
                raise NotImplementedError(f"modality {c.mods[m][0]!r}: per-session layers (use_session) on a softmax cross-entropy modality are "
                                          "not built - the read-out's zeros beyond n_k would enter every row's normaliser")
        self.Imax, self.mult_max = max(sd.I for sd in self.sides.values()), max(sd.mult for sd in self.sides.values())
        self.code, self.es, self.buf, self.b = e.code, 4 if e.dtype == "fp32" else 2, e._buf, e.b
        # the tokeniser chains on the live rows only (bf16; the fp32 parity path keeps the full row space).  lv: (side, slot) -> the
        # slot's mmfm_live_rows, filled by forward()
        # (a segmented plan runs without live-row compaction: the live-bin entry points have no segment forms)
        # (so does a plan with a stitched modality: the read-in runs on the full row space)
        self.live = not self.seg and not self.st and self.code == L.BF16 and live_rows_on(self.BT) and self.live_bias_ok()
        self.lv = {}
        self.enc_flags = L.ATTN_DIAG                                                # mm.py:152-158
        # EngineConfig.context: the encoder's self-attention and the cross-attention (whose mask IS the encoder's, mm.py:210) see a key
        # only inside [lo, hi] over the time stamps.  forward() writes the encoder side's `pos` once per step (mmfm_attn_pos_prep, from
        # the stamp buffers the stitch launches read) and those sites launch mmfm_attn_win_*; the decoder's self-attention does not
        # (adapt_decoder_attention_mask has no context term).  None: no window call anywhere in the plan
        self.win_lohi = None if c.context is None else K.context_window(*c.context)
        self.win = None              # the mmfm_attn_window of the windowed sites, set by forward()
        # mm.py:178-194.  The decoder self-attention sites pass these flags, mod_id and their keep-bit buffer like every other site: at
        # dh = 32 the fast kernels take CAUSAL / SEP (csrc/attention_fast.hip, "mask tiles"), at dh = 64 the general kernels do
        self.dec_flags = (L.ATTN_CAUSAL if c.causal_mask else 0) | (L.ATTN_SEP if c.sep_mask else 0)
        self.fwd, self.bwd, self.cur = [], [], []      # the forward, the closed backward segments, the open one
        self.pend: list = []         # batched reduction: the open segment's slab regions, summed by ONE launch in close_segment
        self.late_lng: list = []     # ... and the norm-fed linears whose mmfm_ln_linear_grad runs behind that launch
        self.lng_sites = 0           # ... counted with the pruned ones: a site keeps the reduced buffer it has in the full plan
        self.slabm_off = 0           # ... and the floats of ws/slabm the open segment has handed out
        self.deferred: list = []     # a parked weight gradient, waiting for a partner (mmfm_gemm_pair)
        self.used_wt: list = []      # weights whose bf16 transpose a dX product reads
        self.stream_in = {}          # layer tag -> the residual stream that entered it

    def embed_saved(self, sd):
        """What the backward of a tokeniser's activation reads: "z", the token_embed pre-activation, stored by the forward;
        "a", the activation itself (softsign in bf16 mode, act 5: nothing extra is stored); None for the identity."""
        if sd.emb_fwd == L.ACT_EMB_IDENTITY:
            return None
        if sd.emb_fwd == L.ACT_SOFTSIGN and self.code == L.BF16:
            return "a"
        return "z"

    def live_bias_ok(self):
        """The live path lets the bias gradient ride on the weight-gradient launch (mmfm_gemm_desc.colsum): a tokeniser linear whose bias
        gradient does not sit right behind its weight gradient would need the stand-alone column sum, which knows no live rows."""
        if not self.grad:
            return True
        e = self.e
        for side, mods in self.mods_of.items():
            for _, mod, _ in mods:
                for lin in ("token_embed", "projection"):
                    w = f"{side}_embeddings.{mod}.embedder.{lin}"
                    gw, gb = e.Gv(w + ".weight"), e.Gb(w)
                    if gb is not None and gb.data_ptr() != gw.data_ptr() + 4 * gw.numel():
                        return False
        return True

    def mk(self, side, name):
        """The key of mask product `name` of `side` ("encoder" / "decoder")."""
        return "dec/" + name if self.split_masks and side == "decoder" else name

    def side(self, name):
        """The Side a block belongs to, from its parameter prefix (`encoder.3`), its tag (`enc3`, `dec0/xa`) or the side's own name."""
        return self.sides["encoder" if name.startswith("enc") else "decoder"]

    @staticmethod
    def rows(t, R, N):
        """The first R x N elements of workspace `t` as [R, N]: a workspace both sides use is sized by the larger side."""
        return t if tuple(t.shape) == (R, N) else t.view(-1)[:R * N].view(R, N)

    def build(self):
        self.workspaces()
        self.forward()
        plan = dict(fwd=self.fwd, bwd=None, B=self.B, T=self.T, training=self.training, M=self.M, R=self.R, BT=self.BT,
                    runs=dict(fwd=0, bwd=0), graphs={}, b=self.b, count=self.mk("decoder", "count"))
        if self.grad:
            full = None
            if self.frozen is not None:
                # the all-trainable backward first, for its launch counts (Engine.backward_report) and for what it leaves behind outside
                # the backward: every buffer of the pool and every transposed weight the forward refreshes, so that the forward of a
                # pruned plan is launch for launch the all-trainable one.  Its launches are dropped
                frozen, self.frozen = self.frozen, None
                self.backward(refresh=False)
                full = [(name, len(seg)) for name, seg in self.bwd]
                self.frozen, self.bwd, self.groups = frozen, [], {}
            self.backward()
            plan.update(bwd=self.bwd, fused=self.fm, use_keep=any(sd.use_keep for sd in self.sides.values()),
                        report=dict(segments=[(name, len(seg), n) for (name, seg), (_, n) in zip(self.bwd, full or [(n_, len(s_)) for n_, s_ in self.bwd])],
                                    pruned=[g for g, (kept, _) in self.groups.items() if not kept],
                                    pruned_params=sorted({k for kept, names in self.groups.values() if not kept for k in names}
                                                         - {k for kept, names in self.groups.values() if kept for k in names})))
        return plan

    # ------------------------------------------------------------------ which gradients are needed
    def trainable(self, names):
        """True where one of the parameters `names` (layout entries) takes a gradient."""
        return self.frozen is None or any(n not in self.frozen for n in names)

    def lin_names(self, wname):
        """The layout entries linear `wname` writes the gradients of: weight and bias, or those of the nn.Linear's a fused projection aliases."""
        has, parts = self.e.layout.has, self.parts.get(wname)
        if parts:
            pre = wname.rsplit(".", 1)[0]
            return [f"{pre}.{nm}{kind}" for nm in parts for kind in (".weight", ".bias") if has(f"{pre}.{nm}{kind}")]
        return [wname + kind for kind in (".weight", ".bias") if has(wname + kind)]

    def norm_names(self, lnname):
        return [lnname + ".scale"] if self.e.is_sn(lnname) else [lnname + ".weight", lnname + ".bias"]

    def tl(self, wname, lnname=None):
        """True where linear `wname`, or the norm that feeds it, takes a gradient."""
        return self.trainable(self.lin_names(wname) + (self.norm_names(lnname) if lnname else []))

    def keep(self, group, kept, names):
        """Records whether the launches of gradient group `group` - they write the gradients of the parameters `names` - are emitted
        (Engine.backward_report names the others) and returns it."""
        self.groups[group] = (bool(kept), tuple(names))
        return bool(kept)

    def skip_slabs(self, S, N, Kd, nb):
        """A pruned weight gradient of the batched-reduction regime still takes its slab region, so that every surviving product keeps
        the region it has in the all-trainable plan."""
        if self.batch_red and S > 1:
            self.slab_region(S, _align(N * Kd + nb) if nb else N * Kd)

    # ------------------------------------------------------------------ static inputs, workspaces, the regime of this shape
    def workspaces(self):
        e, c, buf, sw = self.e, self.c, self.buf, self.sw
        B, T, H, R, BT, Lq, M = self.B, self.T, self.H, self.R, self.BT, self.Lq, self.M
        f32, i64, u8 = torch.float32, torch.int64, torch.uint8
        dec = {m for m, _, _ in self.mods_of["decoder"]}
        chans = [c.mods[m][1] for m in self.staged]
        for m in self.staged:
            n = c.mods[m][1]
            # input rows padded to 16 B (zeros): the tokeniser's weight-gradient GEMM streams them by LDS-DMA (csrc/gemm_dw.hip)
            buf(f"in/{m}", (self.BTm[m], _align(n, 8)), zero=True); buf(f"mask/{m}", (B, self.Tm[m]), i64)
            if m in self.st:        # the padded batch as it came (the read-in writes in/{m}), the session of every sample and the run table
                buf(f"sin/{m}", (self.BTm[m], _align(self.nd[m], 8)), zero=True)
                buf(f"sess/sid/{m}", (B,), torch.int32, zero=True)
                buf(f"sess/runs/{m}", (K.session_runs_ints(B, len(self.st[m]), K.session_dw_chunk(B)),), torch.int32, zero=True)
            if m in dec:            # targets: decoder modalities only
                buf(f"tgt/{m}", (self.BTm[m], self.nd[m]), f32, zero=m in self.st)
            if self.seg:            # the modality's own time stamps and attention mask
                buf(f"ts/{m}", (B, self.Tm[m]), i64); buf(f"attn/{m}", (B, self.Tm[m]), i64)
        if not self.seg:
            buf("ts", (B, T), i64); buf("attn", (B, T), i64)
        Mmax = max(M, self.Md)
        buf("loss_sum", (Mmax,), f32)
        for pre in ("", "dec/") if self.split_masks else ("",):
            buf(pre + "tokmask", (B, Lq), u8); buf(pre + "keypad", (B, Lq), u8)
            if self.per_sample:
                buf(pre + "keep", (B, Lq), u8); buf(pre + "keep_any", (Lq,), u8)
            else:
                buf(pre + "keep0", (Lq,), u8)
            buf(pre + "mod_id", (Lq,), u8); buf(pre + "count", (Mmax,), i64)
        max_slab = 1
        for m, n in zip(self.staged, chans):
            # the same arguments the launches below pass (the token embedding reads its input rows padded to 16 B: ldn selects the
            # streaming kernel and with it another split count)
            for mult in sorted({sd.mult for sd in self.sides.values()}):
                for (mm, nn, ldn) in ((n * mult, n, _align(n, 8)), (H, n * mult, None), (n, H, None)):
                    max_slab = max(max_slab, e._dw_split(mm, nn, self.BTm[m], ldn=ldn, sw=sw)[0] * _align(mm * nn + mm))
        for l in e.linears:
            max_slab = max(max_slab, e._dw_split(l.N, l.K, R, sw=sw)[0] * _align(l.N * l.K + l.N))
        self.slab = buf("ws/slab", (max_slab,), f32)
        self.slab2 = buf("ws/slab2", (max_slab,), f32)          # a deferred weight-gradient GEMM's slabs, paired with the next one (mmfm_gemm_pair)
        # launch-bound regime (R <= 8192, the reference's batch of 16): every dW GEMM keeps its own slab region and ONE
        # mmfm_reduce_slabs_multi per backward segment sums them all (66 reductions of ~7 us each otherwise)
        self.batch_red = R <= 8192 and sw.batch_reduce
        if self.batch_red:
            # regions are handed out per backward segment and reused by the next one (close_segment resets the offset behind the segment's
            # reduction): the largest segment's parameters bound the need, not the whole model's
            seg_max = max(end - s0 for _, s0, end in e.layout.segments)
            self.slabm = buf("ws/slabm", (max(1, min(R // 256, 15)) * (seg_max + 128 * 64),), f32)
        maxN = max([3 * H, self.Imax] + [n * self.mult_max for n in chans])
        buf("ws/col", (max(1, L.lib().mmfm_colsum_workspace(R, maxN) // 4),), f32)
        buf("ws/ln", (max(1, L.lib().mmfm_layernorm_bwd_workspace(R, H) // 4),), f32)
        if self.seg:
            need = max(L.lib().mmfm_stitch_bwd_seg_workspace(self.code, B, self.Tm[m], Lq, self.off[side][slot], H, self.sides[side].max_F)
                       for side, mods in self.mods_of.items() for slot, (m, _, _) in enumerate(mods))
        else:
            need = max(L.lib().mmfm_stitch_bwd_workspace(self.code, B, T, Lq, H, sd.max_F) for sd in self.sides.values())
        buf("ws/stitch", (max(1, need // 4),), f32)
        need = L.lib().mmfm_masked_loss_workspace(BT, 1)
        for m, mod, n in self.mods_of["decoder"]:          # (a model without a softmax cross-entropy modality sizes it as it always did)
            if c.loss_kind[mod] == L.LOSS_SOFTMAX_CE:
                need = max(need, L.lib().mmfm_softmax_ce_workspace(self.BTm[m], n))
        buf("ws/loss", (max(1, need // 4),), f32)
        if self.st:
            if self.grad:
                buf("ws/sess", (max(L.lib().mmfm_session_dw_workspace(B, c.mods[m][1], self.nd[m], len(sz), K.session_dw_chunk(B)) for m, sz in self.st.items()) // 4,), f32)
            for m in self.st:
                # (an element target mask with a channel axis comes out of combine_chan with v folded in: the element form, no channel mask)
                if (self.chan is None or self.chan[m] is None) and (self.elem is None or self.elem[m] is None or self.elem[m][1] is None):
                    raise ValueError(f"modality {c.mods[m][0]!r}: a stitched modality's loss runs under the channel mask of its sessions (Engine.forward(sess=...))")
        if self.chan is not None:
            for m, shape in enumerate(self.chan):
                if shape is None or m not in self.staged:
                    continue
                mod, n = c.mods[m][0], self.nd[m]
                if c.loss_kind.get(mod) == L.LOSS_SOFTMAX_CE:
                    raise ValueError(f"modality {mod!r}: softmax cross-entropy couples its classes - it takes no channel mask (space_attn_mask)")
                if tuple(shape) not in ((B, n), (1, n)):
                    raise ValueError(f"modality {mod!r}: channel mask of shape {tuple(shape)} for [{B} or 1, {n}]")
                if self.elem is None or self.elem[m] is None:
                    raise ValueError(f"modality {mod!r}: a channel mask comes with the staging mask of `combine_chan`")
                buf(chan_buf(m, shape), tuple(shape), u8, zero=True)
        if self.elem is not None:
            for m, shapes in enumerate(self.elem):
                if shapes is None or m not in self.staged:
                    continue
                if shapes[1] is not None and c.loss_kind.get(c.mods[m][0]) == L.LOSS_SOFTMAX_CE and tuple(shapes[1]) != (B, self.Tm[m], 1):
                    raise NotImplementedError(f"modality {c.mods[m][0]!r}: softmax cross-entropy couples its classes - it takes a target "
                                              f"mask of shape [{B}, {self.Tm[m]}, 1] (one value per row), not {tuple(shapes[1])}")
                for which, shape in zip(("cm", "tm"), shapes):
                    if shape is None:           # (a channel-masked modality whose row mask is the token mask has no target mask)
                        continue
                    if len(shape) != 3 or any(s not in (1, full) for s, full in zip(shape, (B, self.Tm[m], self.nd[m]))):
                        raise ValueError(f"modality {c.mods[m][0]!r}: element mask of shape {tuple(shape)} for [{B}, {self.Tm[m]}, {self.nd[m]}]")
                    buf(elem_buf(which, m, shape), tuple(shape), u8, zero=True)
            # sized for the decoder's longest modality, whichever of them carry element masks: one size per pool
            need = max(K.masked_loss_elem_workspace(B, self.Tm[m], self.nd[m]) for m, _, _ in self.mods_of["decoder"])
            buf("ws/loss_elem", (need // 4 + 2,), f32)
        # Two weight gradients whose operands are both at hand (MLP down / up, attention out_proj / qkv) leave in ONE launch
        # (mmfm_gemm_pair): `dlin(..., defer=True)` parks the first, the next `dlin_ln` takes it along; `flush_deferred` issues a
        # parked one alone.  Each product then makes half as many K-slabs (csrc/gemm_dw.hip).
        self.pair_ok = self.code == L.BF16 and not self.batch_red and sw.dw_pair and sw.gemm_dw
        # keep decisions of the attention-probability dropout: one bit tile set per attention site, written by the forward (generator
        # kernel in front of it), read by the backward (csrc/attention_fast.hip; 51 MB per site at B = 1024).  MMFM_ATTN_KEEPBITS=0: hash.
        # Per side: a side without dropout has no workspace, so its sites launch no generator
        fm = self.fm = e._fused_mask(R, sw)
        self.F_QKV, self.F_LNL, self.F_OUT = bool(fm & 1), bool(fm & 2), bool(fm & 8)
        for name, sd in self.sides.items():
            sd.use_keep = self.code == L.BF16 and sd.dp > 0 and self.grad and sw.attn_keepbits
            sd.F_MLP = e.fused_mlp(name, fm)
        self.prep = e._build_prep() if fm else None
        # the context side of all decoder layers in one launch per direction
        self.ctx_group = self.F_LNL and self.code == L.BF16 and c.n_dec > 0 and ctx_group_on(R)
        if fm:
            K.prep_weights(self.prep["table"], self.prep["n"], self.prep["tiles"], plan=self.fwd)
            self.gdb = buf("ws/gdb", (max(_align(l.N * l.K + l.N) for l in e.linears if l.norm),), f32)
            if "ws/lng" not in self.b:
                self.b["ws/lng"] = K.ln_linear_grad_workspace(H, e.device)          # zeroed once; the kernel re-arms its tickets

    def slab_region(self, S, stride):
        o = self.slabm_off
        self.slabm_off = o + S * stride
        if self.slabm_off > self.slabm.numel():
            raise RuntimeError(f"engine: ws/slabm holds {self.slabm.numel()} floats, the plan's slab regions need {self.slabm_off}")
        return self.slabm[o:o + S * stride]

    # ------------------------------------------------------------------ linears and their gradients
    def lin(self, plan, X, wname, Y, Mr, N, Kd, ldx=None, live=None, **kw):
        """live: the mmfm_live_rows of the row space Mr (a tokeniser linear of the live path), else None."""
        gemm = K.gemm if live is None else functools.partial(K.gemm_live, live=live)
        gemm(X, self.e.W(wname + ".weight"), Y, Mr, N, Kd, lda=ldx or Kd, ldb=Kd, ldc=N, bias=self.e.Pb(wname), dtype=self.code, plan=plan, **kw)

    def wgrad(self, plan, dY, X, dst, N, Kd, Mr, nb, S, kchunk, what, ldx=None, colsum=None, slab=None, paired=False, live=None):
        """THE weight-gradient product: dst[N, Kd], with nb (N or 0) column sums of dY right behind it, = dY[Mr, N]^T X[Mr, Kd].
        S == 1: one launch straight into dst (`colsum`: where its column sums go when not behind dst).  S > 1: S K-slabs of `stride`
        floats - in a region of ws/slabm whose reduction joins the segment's ONE launch (batched reduction), else in `slab`, reduced
        into dst at once.  paired: nothing is launched; returns the descriptor for mmfm_gemm_pair and the reduction for `reduce`."""
        n = N * Kd + nb
        if S == 1 and not paired:
            out, cs, split, red = dst, colsum if colsum is not None else (dst.data_ptr() + 4 * N * Kd if nb else None), {}, None
        else:
            stride = _align(n) if nb else n
            out = self.slab_region(S, stride) if self.batch_red else slab
            if S * stride > out.numel():
                raise RuntimeError(f"engine: {what}: {S} slabs x {stride} floats exceed the {out.numel()}-float slab workspace")
            cs = out.data_ptr() + 4 * N * Kd if nb else None
            split, red = dict(splits=S, kchunk=kchunk, slab_stride=stride), (dst, out, n, S, stride)
        emit = K.gemm_desc if paired else functools.partial(K.gemm, plan=plan) if live is None else functools.partial(K.gemm_live, live=live, plan=plan)
        d = emit(dY, X, out, N, Kd, Mr, lda=N, ldb=ldx or Kd, ldc=Kd, a_kcontig=0, b_kcontig=0, dtype=self.code, c_f32=1, colsum=cs, **split)
        if paired:
            return d, red
        if red is not None:
            self.reduce(plan, red)

    def reduce(self, plan, red):
        if self.batch_red:
            self.pend.append(red + (False,))
        else:
            K.reduce_slabs(*red, plan=plan)

    def pair_splits(self, Na, Ka, Nb, Kb, Mr):
        ta, tb = L.lib().mmfm_gemm_dw_tiles(Na, Ka, Mr), L.lib().mmfm_gemm_dw_tiles(Nb, Kb, Mr)
        ia = 256 * (Na + Ka) / (Na + Ka + Nb + Kb)
        Sa = max(1, int(ia) // ta)
        while Sa > 1 and (ta * Sa) % 8:
            Sa -= 1
        Sb = max(1, (256 - ta * Sa) // tb)
        out = []
        for S in (Sa, Sb):
            kchunk = _align(-(-Mr // max(1, min(S, Mr // 512))), 64)
            out += [-(-Mr // kchunk), kchunk]
        return out

    def flush_deferred(self, plan):
        if self.deferred:
            a = self.deferred.pop()
            self.dlin(plan, a["dY"], a["X"], a["wname"], a["Mr"], a["N"], a["Kd"])

    def dlin(self, plan, dY, X, wname, Mr, N, Kd, dX=None, ldx=None, defer=False, live=None, need_dx=True, **kw):
        """Backward of Y[Mr,N] = X[Mr,Kd] @ W[N,Kd]^T + b:  dW, db into G;  dX = dY @ W (optional, fused epilogue).
        ldx = row stride of X when its rows are padded.  live: the mmfm_live_rows of the row space Mr when dY, X and dX hold the live rows
        only (the split count and the kernels are those of all Mr rows; the kernels read the live count off the record).
        Pruned plan: the dW / db launches leave only where the linear takes a gradient, the dX product only where `need_dx`."""
        e, code = self.e, self.code
        want_w = self.keep(wname, self.tl(wname), self.lin_names(wname))
        S, kchunk = e._dw_split(N, Kd, Mr, ldn=ldx, sw=self.sw)
        gw, gb = e.Gv(wname + ".weight"), e.Gb(wname)
        # bf16: the bias gradient (column sums of dY) rides on the dW GEMM (mmfm_gemm_desc.colsum); when the bias
        # gradient sits right behind the weight gradient in the flat buffer one slab reduction finishes both.
        # A bias-free linear (gb None) has no column sum anywhere: the GEMM runs without colsum, its slabs hold the weight gradient only
        fused = code == L.BF16 and gb is not None
        adjacent = fused and gb.data_ptr() == gw.data_ptr() + 4 * N * Kd
        if not want_w:
            self.skip_slabs(S, N, Kd, N if adjacent and S > 1 else 0)
        elif defer and self.pair_ok and S > 1 and (adjacent or gb is None) and dX is None and ldx in (None, Kd):
            self.flush_deferred(plan)
            self.deferred.append(dict(dY=dY, X=X, wname=wname, Mr=Mr, N=N, Kd=Kd, nb=N if gb is not None else 0))
            return
        if want_w:
            self.wgrad(plan, dY, X, gw, N, Kd, Mr, N if adjacent and S > 1 else 0, S, kchunk, wname, ldx=ldx, colsum=gb if fused else None, slab=self.slab,
                       live=live)
            if gb is not None and (not fused or (S > 1 and not adjacent)):
                assert live is None, wname          # live_bias_ok
                K.colsum(dY, Mr, N, N, gb, self.b["ws/col"], plan=plan)
        if dX is not None:
            gemm = K.gemm if live is None else functools.partial(K.gemm_live, live=live)
            wT = e._w_transposed(wname, N, Kd, Mr, sw=self.sw) if code == L.BF16 else None
            if not need_dx:
                return
            if wT is not None:      # reduction >= 512: the 256-tile kernel (csrc/gemm_big.hip) against the K-contiguous transpose W^T [Kd, N]
                self.used_wt.append(wname)
                gemm(dY, wT, dX, Mr, Kd, N, lda=N, ldb=N, ldc=Kd, b_kcontig=1, dtype=code, plan=plan, **kw)
            else:
                gemm(dY, e.W(wname + ".weight"), dX, Mr, Kd, N, lda=N, ldb=Kd, ldc=Kd, b_kcontig=0, dtype=code, plan=plan, **kw)

    def lin_norm_grad(self, plan, Gdb, wname, lnname, N):
        """Weight, bias and norm-parameter gradients of a norm-fed linear from Gdb = [dY^T x_hat | colsum dY]
        (bias-free: dbias None; behind a ScaleNorm Gdb then has no colsum block, dlin_ln)."""
        e, H, ws = self.e, self.H, self.b["ws/lng"]
        if e.is_sn(lnname):
            K.sn_linear_grad(Gdb, e.Pf(wname + ".weight"), e.Pf(lnname + ".scale"), N, H, e.Gv(wname + ".weight"),
                             e.Gb(wname), e.Gv(lnname + ".scale"), ws, plan=plan)
            return
        K.ln_linear_grad(Gdb, e.Pf(wname + ".weight"), e.Pf(lnname + ".weight"), e.Pf(lnname + ".bias"), N, H,
                         e.Gv(wname + ".weight"), e.Gb(wname), e.Gv(lnname + ".weight"), e.Gv(lnname + ".bias"), ws, plan=plan)

    def dlin_ln(self, plan, dYt, tag, wname, lnname, N):
        """Gradients of a LayerNorm-fed linear and of that LayerNorm's affine from G = dY^T x_hat (mmfm_ln_linear_grad)."""
        H, R, deferred = self.H, self.R, self.deferred
        S, kchunk = self.e._dw_split(N, H, R, sw=self.sw)
        xh = self.b[tag + "/xh"]
        # the colsum block behind G: N, or 0 for a bias-free linear behind a ScaleNorm (nobody reads db).  Behind a LayerNorm db = colsum dY
        # stays even without a bias: dW and dbeta need it (beta is folded into the linear)
        nb = N if (self.e.Gb(wname) is not None or not self.e.is_sn(lnname)) else 0
        if not self.keep(wname, self.tl(wname, lnname), self.lin_names(wname) + self.norm_names(lnname)):
            # nothing of the group (the linear, the norm that feeds it) takes a gradient: no product, no reduction, no
            # mmfm_ln_linear_grad.  A parked partner stays parked: the caller's flush_deferred issues it alone
            self.skip_slabs(S, N, H, nb)
            self.lng_sites += self.batch_red and S > 1
            return
        if deferred and S > 1 and deferred[-1]["Mr"] == R:
            a = deferred.pop()
            Sa, kca, Sb, kcb = self.pair_splits(a["N"], a["Kd"], N, H, R)
            da, ra = self.wgrad(plan, a["dY"], a["X"], self.e.Gv(a["wname"] + ".weight"), a["N"], a["Kd"], R, a["nb"], Sa, kca, a["wname"],
                                slab=self.slab2, paired=True)
            db_, rb = self.wgrad(plan, dYt, xh, self.gdb, N, H, R, nb, Sb, kcb, wname, slab=self.slab, paired=True)
            K.gemm_pair(da, db_, plan=plan)
            self.reduce(plan, ra)
            self.reduce(plan, rb)
        elif self.batch_red and S > 1:
            # launch-bound regime: the slabs join the segment's ONE reduction launch (own region, own reduced buffer per site) and
            # mmfm_ln_linear_grad runs behind it at the end of the segment (close_segment) - one reduction launch per site less
            g_site = self.buf(f"ws/gdb/{self.lng_sites}", (self.gdb.numel(),), torch.float32)
            self.wgrad(plan, dYt, xh, g_site, N, H, R, nb, S, kchunk, wname)
            self.late_lng.append((g_site, wname, lnname, N))
            self.lng_sites += 1
            return
        else:
            self.wgrad(plan, dYt, xh, self.gdb, N, H, R, nb, S, kchunk, wname, slab=self.slab)
        self.lin_norm_grad(plan, self.gdb, wname, lnname, N)

    # ------------------------------------------------------------------ norms, norm-fed linears, attention descriptors
    def ln_f(self, plan, X, name, Y, tag, **kw):
        e, R, H, f32 = self.e, self.R, self.H, torch.float32
        if e.is_sn(name):
            K.scalenorm_fwd(X, e.Pf(name + ".scale"), Y, self.buf(tag + "/rstd", (R,), f32), R, H, plan=plan)
            return
        seg_T = kw.pop("seg_T", None)
        if seg_T is not None:
            K.layernorm_fwd_seg(X, e.Pf(name + ".weight"), e.Pf(name + ".bias"), Y, self.buf(tag + "/mean", (R,), f32),
                                self.buf(tag + "/rstd", (R,), f32), R, H, seg_T, plan=plan)
            return
        K.layernorm_fwd(X, e.Pf(name + ".weight"), e.Pf(name + ".bias"), Y, self.buf(tag + "/mean", (R,), f32),
                        self.buf(tag + "/rstd", (R,), f32), R, H, plan=plan, **kw)

    def ln_b(self, plan, dY, X, name, tag, dres, dX, **kw):
        e, b, R, H = self.e, self.b, self.R, self.H
        if e.is_sn(name):       # (ws/ln, sized for the LayerNorm backward, covers the ScaleNorm's per-block partials)
            K.scalenorm_bwd(dY, X, b[tag + "/rstd"], e.Pf(name + ".scale"), dres, dX, e.Gv(name + ".scale"), R, H, b["ws/ln"], plan=plan)
            return
        seg_T = kw.pop("seg_T", None)
        if seg_T is not None:
            K.layernorm_bwd_seg(dY, X, b[tag + "/mean"], b[tag + "/rstd"], e.Pf(name + ".weight"), dres, dX,
                                e.Gv(name + ".weight"), e.Gv(name + ".bias"), R, H, b["ws/ln"], seg_T, plan=plan)
            return
        K.layernorm_bwd(dY, X, b[tag + "/mean"], b[tag + "/rstd"], e.Pf(name + ".weight"), dres, dX,
                        e.Gv(name + ".weight"), e.Gv(name + ".bias"), R, H, b["ws/ln"], plan=plan, **kw)

    def stitch_mode(self, side, slot):
        """The stitch entry points of slot `slot` of `side` - segment, live-row or uniform - as the suffix of their names, and the
        operands the three differ in: the slot's own stamps and offset, or the shared stamps and the slot index (and the live-bin record).
        Under per-sample masks the one _rows pair serves all three: the slot's stamps and offset, the side's keep [B, Lq] with its row
        stride, and the live-bin record or None."""
        lv = self.lv.get((side, slot))
        if self.per_sample:
            ts = self.b[f"ts/{self.mods_of[side][slot][0]}"] if self.seg else self.b["ts"]
            return "_rows", dict(ts=ts, off=self.off[side][slot], keep=self.b[self.mk(side, "keep")], keep_ld=self.Lq,
                                 rec=None if lv is None else lv._keep)
        keep0 = self.b[self.mk(side, "keep0")]
        if self.seg:
            return "_seg", dict(ts=self.b[f"ts/{self.mods_of[side][slot][0]}"], off=self.off[side][slot], keep0=keep0)
        return ("", dict(ts=self.b["ts"], m=slot, keep0=keep0)) if lv is None else ("_live", dict(ts=self.b["ts"], m=slot, rec=lv._keep, keep0=keep0))

    def stitch_f(self, plan, side, slot, tok, mod_row, pos, x, emb):
        sfx, kw = self.stitch_mode(side, slot)
        getattr(K, "stitch_fwd" + sfx)(tok=tok, mod_row=mod_row, pos=pos, x=x, emb=emb, B=self.B,
                                       T=self.Tm[self.mods_of[side][slot][0]], Lseq=self.Lq, H=self.H, max_F=self.sides[side].max_F,
                                       plan=plan, **kw)

    def stitch_b(self, plan, side, slot, dS, dextra, acc_mod):
        """acc_mod: the modality's mod_emb gradient row is added to (the encoder side of a shared table), else overwritten."""
        e, sd = self.e, self.sides[side]
        m, mod, _ = self.mods_of[side][slot]
        pS = f"{side}_embeddings.{mod}.embedder"
        sfx, kw = self.stitch_mode(side, slot)
        getattr(K, "stitch_bwd" + sfx)(dx=dS, dextra=dextra, drop=e._drop(f"{side}/embdrop/{m}", sd.dpe),
                                       d_tok=self.buf(f"d/tok/{side}/{m}", (self.BTm[m], self.H)),
                                       d_mod_row=e.Gv(f"{self.c.mod_emb_owner(side, mod)}_embeddings.{mod}.embedder.mod_emb.weight")[m],
                                       d_pos=e.Gv(pS + ".pos_embed.weight") if sd.pos else None, acc_mod=acc_mod, acc_pos=False, B=self.B,
                                       T=self.Tm[m], Lseq=self.Lq, H=self.H, max_F=sd.max_F, ws=self.b["ws/stitch"], plan=plan, **kw)

    def ln_lin(self, plan, Xin, lnname, wname, Yout, N, tag, residual=None, alias=None):
        """LayerNorm (or ScaleNorm) + the linear it feeds in one launch; x_hat / rstd saved for the backward when training.
        alias = tag of an earlier call on the SAME input: x_hat / rstd do not depend on the norm's affine / gain (it is folded
        into the prepared weights), so the earlier call's saved tensors serve this site's backward too and nothing is stored."""
        b, R, H = self.b, self.R, self.H
        pw = self.prep["v"][wname]
        xh = rs = None
        if alias is not None and self.grad:
            b[tag + "/xh"], b[tag + "/rs"] = b[alias + "/xh"], b[alias + "/rs"]
        elif self.grad:
            xh, rs = self.buf(tag + "/xh", (R, H)), self.buf(tag + "/rs", (R,), torch.float32)
        K.rowgemm(Xin, pw["Wp"], Yout, R, N, H, bias=pw["bp"], ln=2 if self.e.is_sn(lnname) else 1, xhat=xh, rstd=rs, residual=residual,
                  ldr=H if residual is not None else 0, stream_out=True, plan=plan)

    def dx_ln(self, plan, dYt, Kd, tag, wname, lnname, dres, dXout):
        """dX of a norm-fed linear with the norm's backward (and the residual gradient) in its epilogue."""
        H = self.H
        K.rowgemm(dYt, self.prep["v"][wname]["WpT"], dXout, self.R, H, Kd, ldw=Kd, residual=dres, ldr=H if dres is not None else 0,
                  ln_bwd=2 if self.e.is_sn(lnname) else 1, bwd_xhat=self.b[tag + "/xh"], bwd_rstd=self.b[tag + "/rs"], plan=plan)

    def attn_desc(self, tag, q, ldq, kv, ldkv, koff, voff, o, flags, d_o=None, dq=None, dkv=None, lddq=0, lddkv=0, dkoff=0, dvoff=0):
        """The descriptor of attention site `tag` (`enc{i}/sa`, `dec{i}/sa`, `dec{i}/xa`): head count, head dim, dropout, the keep-bit
        workspace and the LSE buffer are the site's side's - cross-attention splits the context's keys / values by the decoder's heads."""
        e, b, buf, B, Lq, H, es, sd = self.e, self.b, self.buf, self.B, self.Lq, self.H, self.es, self.side(tag)
        heads, dp = sd.heads, sd.dp
        # whose mask products: the encoder's for its self-attention and for cross-attention (xa_mask IS the encoder's mask, mm.py:210),
        # the decoder's (its mod_id under CAUSAL / SEP) for the decoder's self-attention
        ms = "decoder" if tag.startswith("dec") and tag.endswith("/sa") else "encoder"
        dh = H // heads
        # (a windowed site at dh 64 / 128 runs the general kernels, which hash their drop_p decisions: no keep-bit workspace.  At dh 32 the
        # keep-bit kernels have window forms and the site keeps the workspace it always had)
        keep = buf(tag + "/keep", (K.attn_keepbits_bytes(B, heads, Lq, Lq),), torch.uint8) if sd.use_keep and (dh == 32 or not self.windowed(tag)) else None
        return K.attn_desc(self.code, B, heads, Lq, Lq, dh, q.data_ptr(), kv.data_ptr() + koff * es, kv.data_ptr() + voff * es, ldq, ldkv, ldkv,
                           o.data_ptr(), H, buf(tag + "/lse", (B, heads, Lq), torch.float32), b[self.mk(ms, "keypad")], b[self.mk(ms, "mod_id")], flags,
                           1.0 / math.sqrt(dh), drop_p=e._drop(tag + "/p", dp), drop_o=e._drop(tag + "/o", dp),
                           d_o=K.P(d_o), lddo=H, dq=K.P(dq), dk=None if dkv is None else dkv.data_ptr() + dkoff * es,
                           dv=None if dkv is None else dkv.data_ptr() + dvoff * es, lddq=lddq, lddk=lddkv, lddv=lddkv, keepbits=keep)

    def windowed(self, tag):
        """Whether attention site `tag` runs under the context window: every site but the decoder's self-attention, when there is one."""
        return self.win_lohi is not None and not (tag.startswith("dec") and tag.endswith("/sa"))

    def attn(self, plan, tag, desc, backward=False):
        """Emits attention site `tag`: mmfm_attn_win_fwd / _bwd with the plan's window where `windowed`, else mmfm_attn_fwd / _bwd."""
        if self.windowed(tag):
            (K.attn_win_bwd if backward else K.attn_win_fwd)(desc, self.win, plan=plan)
        else:
            (K.attn_bwd if backward else K.attn_fwd)(desc, plan=plan)

    def elem_tm(self, m):
        """Modality m's static target-mask buffer where its loss runs under a per-element mask, else None."""
        shapes = self.elem[m] if self.elem is not None else None
        return None if shapes is None or shapes[1] is None else self.b[elem_buf("tm", m, shapes[1])]

    def chan_rows(self, m, tokmask, off):
        """Where modality m's loss runs under a channel mask: (row mask, its leading dimension, the static channel-mask buffer) - the
        row mask is the [B,T,1] / [1,T,1] target mask where the modality has one (mask_ld T / 0), else the token mask - else None."""
        if self.chan is None or self.chan[m] is None:
            return None
        tm = self.elem_tm(m)
        if tm is None:
            return tokmask[:, off:], self.Lq, self.b[chan_buf(m, self.chan[m])]
        return tm, (0 if tm.shape[0] == 1 else self.Tm[m]), self.b[chan_buf(m, self.chan[m])]

    def sess_desc(self, m, which, bias=True, grads=False, ld_p=None):
        """The mmfm_session_desc of stitched modality m: which = "in" (read-in: the padded side is sin/{m}, the P side in/{m}'s rows) or
        "out" (read-out: pred/{m} and the head's output).  grads: the gradient launch's form (no weights; dW / db are bounded by G)."""
        e, c = self.e, self.c
        t = e.session_tables(m)
        width, N = c.mods[m][1], self.nd[m]
        ld_pad, ld_p = (_align(N, 8), ld_p or _align(width, 8)) if which == "in" else (N, width)
        return K.session_desc(self.code, self.B, self.Tm[m], width, N, len(self.st[m]), self.b[f"sess/sid/{m}"], t["n"], t["w_" + which],
                              ld_pad=ld_pad, ld_p=ld_p, b_off=t["b_" + which] if c.stitch_bias else None, w=None if grads else e.Pw,
                              w_elems=e.layout.n, bias=e.P if bias and c.stitch_bias and not grads else None, b_elems=e.layout.n)

    def sess_names(self, m, which):
        """The layout entries of modality m's read-in ("in") / read-out ("out") layers."""
        mod = self.c.mods[m][0]
        return [f"session_{which}.{mod}.{k}.{kind}" for k in range(len(self.st[m])) for kind in (("weight", "bias") if self.c.stitch_bias else ("weight",))]

    def sess_dw(self, plan, m, which, a_pad, q):
        """The weight (and bias) gradients of modality m's session layers in one call: absent sessions keep their spans of G."""
        e = self.e
        K.session_dw(self.sess_desc(m, which, grads=True, ld_p=self.c.mods[m][1]), a_pad, q, self.b[f"sess/runs/{m}"], K.session_dw_chunk(self.B), e.G,
                     e.G if self.c.stitch_bias else None, which == "out", self.b["ws/sess"], plan=plan)

    def loss_spec(self, mod):
        c = self.c
        return c.loss_kind[mod], float(c.loss_param.get(mod, 0.0)), int(c.loss_flags.get(mod, 0))

    def loss(self, plan, mod, two_kind, kind_fn, *args):
        """A modality's masked loss, forward or backward.  PoissonNLL(log_input) / MSE without a flag go through the two-kind entry
        points (`two_kind`), call for call the plan it always was; every other elementwise kind through `kind_fn` with its float and
        flags.  Softmax cross-entropy has calls of its own: `softmax_ce`."""
        c = self.c
        kind, param, flags = c.loss_kind[mod], float(c.loss_param.get(mod, 0.0)), int(c.loss_flags.get(mod, 0))
        if kind in (L.LOSS_POISSON_LOG, L.LOSS_MSE) and flags == 0:
            two_kind(kind, *args, plan=plan)
        else:
            kind_fn(kind, param, flags, *args, plan=plan)

    def softmax_ce(self, plan, m, mod, pred, target, rowmask, mask_ld, T, R, N, loss_sum=None, ws=None, dpred=None):
        """The softmax cross-entropy of modality `m` (loss_kind 7): the forward (`loss_sum`, `ws`) or, with `dpred`, the backward.  The
        training plan saves (lse, sum w t') per row in `rowstat/{m}` for a one-pass backward; the forward-only plan passes NULL."""
        w, eps, b = self.e.loss_w.get(mod), float(self.c.loss_param.get(mod, 0.0)), self.b
        if dpred is None:
            stat = self.buf(f"rowstat/{m}", (R, 2), torch.float32) if self.grad else None
            K.softmax_ce_fwd(pred, target, w, eps, rowmask, mask_ld, T, R, N, loss_sum, stat, ws, plan=plan)
        else:
            K.softmax_ce_bwd(pred, target, w, eps, rowmask, mask_ld, T, R, N, b[f"rowstat/{m}"], b["gout"], b["inv_n"], dpred, plan=plan)

    # ------------------------------------------------------------------ forward blocks
    def out_proj(self, plan, a, wname, Xres, Xout):
        R, H = self.R, self.H
        if self.F_OUT:
            K.rowgemm(a, self.e.W(wname + ".weight"), Xout, R, H, H, bias=self.e.Pb(wname), residual=Xres, ldr=H, plan=plan)
        else:
            self.lin(plan, a, wname, Xout, R, H, H, residual=Xres, ldr=H)

    def self_block(self, plan, X, p, tag, flags):
        """x + attn(ln1(x))  (encoder_embeddings.py:112, decoder_embeddings.py:141)."""
        buf, R, H = self.buf, self.R, self.H
        qkv, a, Xa = buf(tag + "/qkv", (R, 3 * H)), buf(tag + "/a", (R, H)), buf(tag + "/xa", (R, H))
        if self.F_QKV:
            self.ln_lin(plan, X, p + ".ln1", p + ".attn.qkv", qkv, 3 * H, tag + "/ln1")
        else:
            self.ln_f(plan, X, p + ".ln1", buf(tag + "/h1", (R, H)), tag + "/ln1")
            self.lin(plan, self.b[tag + "/h1"], p + ".attn.qkv", qkv, R, 3 * H, H)
        self.attn(plan, tag + "/sa", self.attn_desc(tag + "/sa", qkv, 3 * H, qkv, 3 * H, H, 2 * H, a, flags))
        self.out_proj(plan, a, p + ".attn.out_proj", X, Xa)
        return Xa

    def mlp_block(self, plan, X, p, tag):
        """x + mlp(ln2(x))  (encoder_embeddings.py:114; mm_utils.py:50-52)."""
        e, buf, R, H, f32, sd = self.e, self.buf, self.R, self.H, torch.float32, self.side(p)
        I, dp = sd.I, sd.dp
        Xb = buf(tag + "/xb", (R, H))
        if sd.F_MLP:
            pu = self.prep["v"][p + ".mlp.up_proj"]
            d_ = K.mlp_desc(R, x=X, w_up=pu["Wp"], b_up=pu["bp"], w_down=self.prep["v"][p + ".mlp.down_proj"]["WpP"],
                            b_down=e.Pb(p + ".mlp.down_proj"), drop=e._drop(tag + "/mlpdrop", dp), y=Xb,
                            xhat=buf(tag + "/ln2/xh", (R, H)) if self.grad else None,
                            rstd=buf(tag + "/ln2/rs", (R,), f32) if self.grad else None, scalenorm=e.is_sn(p + ".ln2"),
                            act=sd.act[0], act_beta=sd.act[1])
            K.mlp_fwd(d_, plan=plan)
            return Xb
        h, u, g = buf(tag + "/h2", (R, H)), buf(tag + "/u", (R, I)), buf(tag + "/g", (R, I))
        self.ln_f(plan, X, p + ".ln2", h, tag + "/ln2")
        self.lin(plan, h, p + ".mlp.up_proj", g, R, I, H, pre_out=u, act=sd.act_fwd, act_scale=sd.act[1])
        self.lin(plan, g, p + ".mlp.down_proj", Xb, R, H, I, drop=e._drop(tag + "/mlpdrop", dp), residual=X, ldr=H)
        return Xb

    # ------------------------------------------------------------------ forward
    def forward(self):
        e, c, b, buf, fwd = self.e, self.c, self.b, self.buf, self.fwd
        B, T, H, R, BT, Lq, M = self.B, self.T, self.H, self.R, self.BT, self.Lq, self.M
        mk = self.mk
        for side in ("encoder", "decoder") if self.split_masks else ("encoder",):       # mm.py:147-149 / 169-171: each side's own masks
            mods = self.mods_of[side]
            if self.per_sample:
                outs = [b[mk(side, k)] for k in ("tokmask", "keypad", "keep", "keep_any", "mod_id", "count")]
                K.mask_prep_rows(B, [self.Tm[m] for m, _, _ in mods], [b[f"mask/{m}"] for m, _, _ in mods], [1] * len(mods),
                                 [b[f"attn/{m}"] if self.seg else b["attn"] for m, _, _ in mods], [n for _, _, n in mods], *outs, plan=fwd)
                if self.live:       # a bin is dead only where every sample masks it
                    K.live_bins(b[mk(side, "keep_any")], T, M, buf(mk(side, "live"), (M, L.live_rec_ints(T)), torch.int32), plan=fwd)
                continue
            outs = [b[mk(side, k)] for k in ("tokmask", "keypad", "keep0", "mod_id", "count")]
            if self.seg:
                K.mask_prep_seg(B, [self.Tm[m] for m, _, _ in mods], [b[f"mask/{m}"] for m, _, _ in mods], [1] * len(mods),
                                [b[f"attn/{m}"] for m, _, _ in mods], [n for _, _, n in mods], *outs, plan=fwd)
            else:
                K.mask_prep(B, T, [b[f"mask/{m}"] for m, _, _ in mods], [1] * M, b["attn"], [n for _, _, n in mods], *outs, plan=fwd)
            if self.live:
                # the live-bin records of the side's modality slots, from its keep0 (device side: nothing is read back)
                rec = buf(mk(side, "live"), (M, L.live_rec_ints(T)), torch.int32)
                K.live_bins(b[mk(side, "keep0")], T, M, rec, plan=fwd)
        if self.win_lohi is not None:
            # the encoder side's time stamps as int32 [B, Lq], slot by slot: the shared stamp tensor once per slot, or each slot's own
            enc = self.mods_of["encoder"]
            pos = buf("attn/pos", (B, Lq), torch.int32)
            K.attn_pos_prep(B, [self.Tm[m] for m, _, _ in enc], [b[f"ts/{m}"] if self.seg else b["ts"] for m, _, _ in enc], pos, plan=fwd)
            self.win = K.attn_window(pos, *self.win_lohi)
        gathered = set()
        for m in self.st:           # the read-in, once per stitched modality: both sides' tokenisers read in/{m}
            K.session_reduce(self.sess_desc(m, "in"), b[f"sin/{m}"], b[f"in/{m}"], plan=fwd)
        tok_tmp = buf("tok_tmp", (BT, H))
        x_enc, emb_enc, x_dec = buf("x_enc", (R, H)), buf("emb_enc", (R, H)), buf("x_dec", (R, H))
        for side, xs, es_ in (("encoder", x_enc, emb_enc), ("decoder", x_dec, None)):
            sd = self.sides[side]
            for slot, (m, mod, n) in enumerate(self.mods_of[side]):
                p = f"{side}_embeddings.{mod}.embedder"
                n2 = n * sd.mult
                BT = self.BTm[m]
                a = buf(f"{side}/a/{m}", (BT, n2))
                # bf16 mode: the backward takes softsign' from the activation itself (act 5), no saved pre-activation (274 MB per
                # tokeniser at B = 1024, written here and read back there); the fp32 parity path keeps the exact form
                # every other activation but the identity stores z in both modes (2 bytes x B T x mult N in bf16)
                z = buf(f"{side}/z/{m}", (BT, n2)) if self.embed_saved(sd) == "z" else None
                xin, lv = b[f"in/{m}"], None
                if self.live:
                    # a, z and tok_tmp hold the live rows only (b * T_live + rank[t]); the input's live rows are gathered once per
                    # modality and mask set (the two sides share them unless their modalities differ)
                    rec = b[mk(side, "live")][slot]
                    lv = self.lv[side, slot] = K.live_rows(rec, B, T)
                    xin = buf(mk(side, f"in_live/{m}"), (BT, _align(n, 8)))
                    if mk(side, f"in_live/{m}") not in gathered:
                        gathered.add(mk(side, f"in_live/{m}"))
                        K.gather_live_rows(b[f"in/{m}"], xin, B, T, _align(n, 8) * self.es, rec, plan=fwd)
                self.lin(fwd, xin, p + ".token_embed", a, BT, n2, n, ldx=_align(n, 8), pre_out=z, act=sd.emb_fwd, act_scale=sd.scale, live=lv)
                tok = self.rows(tok_tmp, BT, H)
                self.lin(fwd, a, p + ".projection", tok, BT, H, n2, drop=e._drop(f"{side}/embdrop/{m}", sd.dpe), live=lv)
                # row mod_to_indx[mod] of the table this tokeniser reads: its own, or the encoder's where the two share it
                mod_row = e.Pf(f"{c.mod_emb_owner(side, mod)}_embeddings.{mod}.embedder.mod_emb.weight")[m]
                pos = e.Pf(p + ".pos_embed.weight") if sd.pos else None            # embedder.pos: false -> emb = the modality row
                self.stitch_f(fwd, side, slot, tok, mod_row, pos, xs, es_)
        X = x_enc
        for i in range(c.n_enc):
            p, tag = f"encoder.{i}", f"enc{i}"
            self.stream_in[tag] = X
            X = self.mlp_block(fwd, self.self_block(fwd, X, p, tag, self.enc_flags), p, tag)
        self.enc_last = X
        enc_out, context = buf("enc_out", (R, H)), buf("context", (R, H))
        if self.F_LNL:
            self.ln_lin(fwd, X, "encoder_norm", "decoder_proj_context", context, H, "encnorm", residual=emb_enc)
        else:
            self.ln_f(fwd, X, "encoder_norm", enc_out, "encnorm")
            self.lin(fwd, enc_out, "decoder_proj_context", context, R, H, H, residual=emb_enc, ldr=H)       # mm.py:292
        if self.ctx_group:
            self.context_kv(fwd, context)
        Y = x_dec
        for i in range(c.n_dec):
            p, tag = f"decoder.{i}", f"dec{i}"
            self.stream_in[tag] = Y
            Ya = self.self_block(fwd, Y, p, tag, self.dec_flags)
            qc, kvc, a2, Yb = buf(tag + "/qc", (R, H)), buf(tag + "/kvc", (R, 2 * H)), buf(tag + "/a2", (R, H)), buf(tag + "/yb", (R, H))
            if self.F_LNL:
                self.ln_lin(fwd, Ya, p + ".query_norm", p + ".cross_attn.query", qc, H, tag + "/qn")
                # every decoder layer normalises the same context rows: the statistics are saved by the first layer only
                if not self.ctx_group:
                    self.ln_lin(fwd, context, p + ".context_norm", p + ".cross_attn.kv", kvc, 2 * H, tag + "/cn", alias=None if i == 0 else "dec0/cn")
            else:
                hq, hc = buf(tag + "/hq", (R, H)), buf(tag + "/hc", (R, H))
                self.ln_f(fwd, Ya, p + ".query_norm", hq, tag + "/qn")
                self.ln_f(fwd, context, p + ".context_norm", hc, tag + "/cn")
                self.lin(fwd, hq, p + ".cross_attn.query", qc, R, H, H)
                self.lin(fwd, hc, p + ".cross_attn.kv", kvc, R, 2 * H, H)
            self.attn(fwd, tag + "/xa", self.attn_desc(tag + "/xa", qc, H, kvc, 2 * H, 0, H, a2, self.enc_flags))   # xa_mask = encoder mask
            self.out_proj(fwd, a2, p + ".cross_attn.out_proj", Ya, Yb)
            Y = self.mlp_block(fwd, Yb, p, tag)
        self.dec_last = Y
        ydec = buf("ydec", (R, H))                         # de-stitched: [M][B*T][H]
        self.ln_f(fwd, Y, "decoder_norm", ydec, "decnorm", **self.destitch())
        tokmask = b[mk("decoder", "tokmask")]
        for j, (m, mod, n) in enumerate(self.mods_of["decoder"]):
            BT, (r0, r1), off = self.BTm[m], self.ydec_rows(j), self.off["decoder"][j]
            pred = buf(f"pred/{m}", (BT, self.nd[m]))
            if m in self.st:        # the head writes f [BT, P]; the read-out expands it to the padded width, zeros beyond n_s
                fP = buf(f"sess/f/{m}", (BT, n))
                self.lin(fwd, ydec[r0:r1], f"decoder_embeddings.{mod}.out", fP, BT, n, H)
                K.session_expand(self.sess_desc(m, "out"), fP, pred, plan=fwd)
                n = self.nd[m]
            else:
                self.lin(fwd, ydec[r0:r1], f"decoder_embeddings.{mod}.out", pred, BT, n, H)
            ch = self.chan_rows(m, tokmask, off)
            if ch is not None:       # row mask x channel mask: the sum and (behind mmfm_mask_prep) the modality's count
                K.masked_loss_chan_fwd(*self.loss_spec(mod), pred, b[f"tgt/{m}"], ch[0], ch[1], self.Tm[m], BT, n, ch[2], b["loss_sum"][j:j + 1],
                                       b[mk("decoder", "count")][j:j + 1], b["ws/loss_elem"], plan=fwd)
                continue
            if self.elem_tm(m) is not None and c.loss_kind[mod] == L.LOSS_SOFTMAX_CE:
                # coupled classes: the [B,T,1] target mask IS a row mask of pitch T for the softmax cross-entropy kernels; the count -
                # N per set row, as mmfm_mask_prep counts a token mask - comes from one element-mask launch whose sum is discarded
                K.masked_loss_elem_fwd(L.LOSS_MSE, 0.0, 0, pred, b[f"tgt/{m}"], self.elem_tm(m), B, self.Tm[m], n, buf("loss_sum/unused", (1,), torch.float32),
                                       b[mk("decoder", "count")][j:j + 1], b["ws/loss_elem"], plan=fwd)
                self.softmax_ce(fwd, m, mod, pred, b[f"tgt/{m}"], self.elem_tm(m), self.Tm[m], self.Tm[m], BT, n, loss_sum=b["loss_sum"][j:j + 1], ws=b["ws/loss"])
                continue
            if self.elem_tm(m) is not None:       # per-element target mask: the sum and (behind mmfm_mask_prep) the modality's count
                K.masked_loss_elem_fwd(*self.loss_spec(mod), pred, b[f"tgt/{m}"], self.elem_tm(m), B, self.Tm[m], n, b["loss_sum"][j:j + 1],
                                       b[mk("decoder", "count")][j:j + 1], b["ws/loss_elem"], plan=fwd)
                continue
            if c.loss_kind[mod] == L.LOSS_SOFTMAX_CE:
                self.softmax_ce(fwd, m, mod, pred, b[f"tgt/{m}"], tokmask[:, off:], Lq, self.Tm[m], BT, n, loss_sum=b["loss_sum"][j:j + 1], ws=b["ws/loss"])
                continue
            self.loss(fwd, mod, K.masked_loss_fwd, K.masked_loss_kind_fwd, pred, b[f"tgt/{m}"], tokmask[:, off:], Lq, self.Tm[m], BT, n,
                      b["loss_sum"][j:j + 1], b["ws/loss"])
        K.loss_finalize(b["loss_sum"], b[mk("decoder", "count")], self.Md, b["loss"], b["inv_n"], plan=fwd)

    def destitch(self):
        """What tells decoder_norm's launches to write / read the per-modality blocks of ydec: ds_L / ds_T, or the decoder's segments."""
        if self.seg:
            return dict(seg_T=[self.Tm[m] for m, _, _ in self.mods_of["decoder"]])
        return dict(ds_L=self.Lq, ds_T=self.T)

    def ydec_rows(self, j):
        """The rows of the de-stitched ydec / d/ydec that hold decoder slot j: [B * off_j, B * off_{j+1})."""
        off = self.off["decoder"]
        return self.B * off[j], self.B * off[j + 1]

    def ctx_norm_kind(self):
        """1 / 2: every decoder layer's context_norm is a LayerNorm / a ScaleNorm (the grouped launches norm once for all of them)."""
        kinds = {self.e.is_sn(f"decoder.{i}.context_norm") for i in range(self.c.n_dec)}
        assert len(kinds) == 1, "decoder layers with different context_norm kinds"
        return 2 if kinds.pop() else 1

    def context_kv(self, plan, context):
        """dec{i}/kvc of every decoder layer from ONE pass over `context`: norm once (x_hat / rstd saved under dec0/cn, which every layer's
        backward reads), then each layer's prepared cross_attn.kv.  Launches of as many layers as the biases fit in LDS, at most 8."""
        b, R, H, n_dec = self.b, self.R, self.H, self.c.n_dec
        per = max(1, min(L.ROWGEMM_MAX_GROUPS, CTX_GROUP_BIAS // (2 * H)))
        xh = rs = None
        if self.grad:
            xh, rs = self.buf("dec0/cn/xh", (R, H)), self.buf("dec0/cn/rs", (R,), torch.float32)
        for i0 in range(0, n_dec, per):
            ids = range(i0, min(n_dec, i0 + per))
            pws = [self.prep["v"][f"decoder.{i}.cross_attn.kv"] for i in ids]
            K.rowgemm_groups([context], [pw["Wp"] for pw in pws], [self.buf(f"dec{i}/kvc", (R, 2 * H)) for i in ids], R, 2 * H, H,
                             biases=[pw["bp"] for pw in pws], ln=self.ctx_norm_kind(), xhat=xh if i0 == 0 else None,
                             rstd=rs if i0 == 0 else None, stream_out=True, plan=plan)
        if self.grad:
            for i in range(1, n_dec):
                b[f"dec{i}/cn/xh"], b[f"dec{i}/cn/rs"] = xh, rs

    def context_back(self, plan, dctx):
        """d/ctx = norm'( sum_i d/kvc/{i} . W'_i ) in one launch (more than 8 layers: launches of 8 chained through the residual input)."""
        b, R, H, n_dec = self.b, self.R, self.H, self.c.n_dec
        order = list(reversed(range(n_dec)))
        for j0 in range(0, n_dec, L.ROWGEMM_MAX_GROUPS):
            ids = order[j0:j0 + L.ROWGEMM_MAX_GROUPS]
            K.rowgemm_groups([b[f"d/kvc/{i}"] for i in ids], [self.prep["v"][f"decoder.{i}.cross_attn.kv"]["WpT"] for i in ids], [dctx], R, H, 2 * H,
                             ldw=2 * H, residual=dctx if j0 else None, ldr=H if j0 else 0, ln_bwd=self.ctx_norm_kind(),
                             bwd_xhat=b["dec0/cn/xh"], bwd_rstd=b["dec0/cn/rs"], plan=plan)

    # ------------------------------------------------------------------ backward blocks
    def close_segment(self, name):
        if self.pend:                          # the segment's weight-gradient slabs, all in one launch, before its DDP hook fires
            K.reduce_slabs_multi(list(self.pend), self.e.device, plan=self.cur)
            self.pend.clear()
        for g_site, wname, lnname, N in self.late_lng:
            self.lin_norm_grad(self.cur, g_site, wname, lnname, N)
        self.late_lng.clear()
        self.lng_sites = 0
        self.slabm_off = 0                     # the reduction has consumed the regions (stream order): the next segment reuses them
        self.bwd.append((name, self.cur))
        self.cur = []

    def mlp_back(self, plan, dS, p, tag, X_in, below=True):
        """dS: running gradient of the residual stream (in place).  X_in = the stream value that fed ln2.
        below: a launch behind this block reads dS (pruned plan: False where the stream ends above)."""
        e, b, buf, R, H, sd = self.e, self.b, self.buf, self.R, self.H, self.side(p)
        I, dp = sd.I, sd.dp
        up, down = self.tl(p + ".mlp.up_proj", p + ".ln2"), self.tl(p + ".mlp.down_proj")
        need_du = up or below                        # du feeds the up-projection's group and the dX of ln2
        if sd.F_MLP:
            pu, pdn = self.prep["v"][p + ".mlp.up_proj"], self.prep["v"][p + ".mlp.down_proj"]
            t1b, gb, dub = buf("d/t1m", (R, H)), buf("d/g", (R, I)), buf("d/du", (R, I))
            # same-box A/B at B = 1024: 30.80 -> 30.37 ms/step.  A ScaleNorm ln2 always splits (the one-launch kernel has no ScaleNorm epilogue)
            split = self.sw.mlp_bwd_split or e.is_sn(p + ".ln2")
            # neither projection takes a gradient: only the weight-gradient products read t1 and g, the front half writes du alone
            dx_only = split and not up and not down and MLP_DX_ONLY
            d_ = K.mlp_desc(R, w_up=pu["Wp"], b_up=pu["bp"], drop=e._drop(tag + "/mlpdrop", dp), xhat=b[tag + "/ln2/xh"],
                            rstd=b[tag + "/ln2/rs"], dy=dS, w_down_t=pdn["WpT"], w_up_t=pu["WpTP"], t1=None if dx_only else t1b,
                            g=None if dx_only else gb, du=dub,
                            dx=None if split else dS, scalenorm=e.is_sn(p + ".ln2"), act=sd.act[0], act_beta=sd.act[1])
            if need_du or down:
                K.mlp_bwd(d_, plan=plan)
            if split and below:     # front half only above (t1, g, du); dX + LayerNorm backward + residual by the row-owner K = I kernel
                self.dx_ln(plan, dub, I, tag + "/ln2", p + ".mlp.up_proj", p + ".ln2", dS, dS)
            self.dlin(plan, t1b, gb, p + ".mlp.down_proj", R, H, I, defer=True)     # dW_down = t1^T g, db_down = colsum t1
            self.dlin_ln(plan, dub, tag + "/ln2", p + ".mlp.up_proj", p + ".ln2", I)
            self.flush_deferred(plan)
            return
        dSd = dS
        if dp > 0:                                                       # mm_utils.py:52 dropout(down_proj(.))
            if need_du or down:
                K.dropout_apply(dS, b["d/t1"], R, H, e._drop(tag + "/mlpdrop", dp), plan=plan)
            dSd = b["d/t1"]
        du = self.rows(b["d/u"], R, I)
        self.dlin(plan, dSd, b[tag + "/g"], p + ".mlp.down_proj", R, H, I, dX=du, need_dx=need_du, act=sd.act_grad, act_scale=sd.act[1],
                  gradmul_pre=b[tag + "/u"])
        self.norm_lin_back(plan, False, du, I, tag + "/ln2", p + ".mlp.up_proj", p + ".ln2", tag + "/h2", X_in, dS, dS, need_dx=below)

    def norm_lin_back(self, plan, fused, dYt, N, tag, wname, lnname, hkey, X_in, dres, dXout, need_dx=True):
        """Backward of a norm-fed linear [N, H] and its norm (input X_in; un-fused: normalised rows saved under `hkey`): the residual
        stream gradient dXout = dres + norm'(dYt W).  A parked weight gradient leaves with this one's (fused) or alone in front of it.
        need_dx: a later launch reads dXout.  The un-fused norm backward also runs for its own parameters' sake."""
        if fused:
            self.dlin_ln(plan, dYt, tag, wname, lnname, N)
            self.flush_deferred(plan)
            if need_dx:
                self.dx_ln(plan, dYt, N, tag, wname, lnname, dres, dXout)
        else:
            self.flush_deferred(plan)
            norm = self.keep(lnname, need_dx or self.trainable(self.norm_names(lnname)), self.norm_names(lnname))
            self.dlin(plan, dYt, self.b[hkey], wname, self.R, N, self.H, dX=self.b["d/h"], need_dx=norm)
            if norm:
                self.ln_b(plan, self.b["d/h"], X_in, lnname, tag, dres, dXout)

    def out_proj_back(self, plan, dS, a, wname, need_dx=True):
        """dW, db of an attention out_proj and d(attention output) -> d/t2 (need_dx: the attention backward behind it runs)."""
        R, H, t2 = self.R, self.H, self.b["d/t2"]
        if self.F_OUT:
            self.dlin(plan, dS, a, wname, R, H, H, defer=True)        # leaves with the next LayerNorm-fed linear's weight gradient
            if need_dx:
                K.rowgemm(dS, self.prep["v"][wname]["WpT"], t2, R, H, H, plan=plan)
        else:
            self.dlin(plan, dS, a, wname, R, H, H, dX=t2, need_dx=need_dx)

    def self_back(self, plan, dS, p, tag, flags, below=True):
        """below: a launch behind this block reads dS."""
        b, H = self.b, self.H
        attn = below or self.tl(p + ".attn.qkv", p + ".ln1")          # d/qkv feeds the projection's group and the dX of ln1
        self.out_proj_back(plan, dS, b[tag + "/a"], p + ".attn.out_proj", need_dx=attn)
        qkv, dqkv = b[tag + "/qkv"], b["d/qkv"]
        if attn:
            self.attn(plan, tag + "/sa", self.attn_desc(tag + "/sa", qkv, 3 * H, qkv, 3 * H, H, 2 * H, b[tag + "/a"], flags, d_o=b["d/t2"], dq=dqkv,
                                                        dkv=dqkv, lddq=3 * H, lddkv=3 * H, dkoff=H, dvoff=2 * H), backward=True)
        self.norm_lin_back(plan, self.F_QKV, dqkv, 3 * H, tag + "/ln1", p + ".attn.qkv", p + ".ln1", tag + "/h1", self.stream_in[tag], dS, dS,
                           need_dx=below)

    def cross_back(self, plan, dY, p, tag, dctx_in, below=True, ctx=True):
        """Cross attention (decoder_embeddings.py:143): query side -> the stream dY, context side -> d/ctx (added to `dctx_in`).
        below: a launch behind this block reads dY; ctx: something upstream of the context takes a gradient (d/ctx is needed)."""
        b, H, dqc = self.b, self.H, self.b["d/qc"]
        # grouped context side: every layer keeps its own d/kvc until the bridge segment sums their dX products (context_back)
        dkvc = b["d/kvc/" + tag[3:]] if self.ctx_group else b["d/kvc"]
        # the attention backward runs if dq (the query group, the stream) or dk / dv (the kv group, the context) is needed
        attn = below or ctx or self.tl(p + ".cross_attn.query", p + ".query_norm") or self.tl(p + ".cross_attn.kv", p + ".context_norm")
        self.out_proj_back(plan, dY, b[tag + "/a2"], p + ".cross_attn.out_proj", need_dx=attn)
        if attn:
            self.attn(plan, tag + "/xa", self.attn_desc(tag + "/xa", b[tag + "/qc"], H, b[tag + "/kvc"], 2 * H, 0, H, b[tag + "/a2"], self.enc_flags,
                                                        d_o=b["d/t2"], dq=dqc, dkv=dkvc, lddq=H, lddkv=2 * H, dkoff=0, dvoff=H), backward=True)
        self.norm_lin_back(plan, self.F_LNL, dqc, H, tag + "/qn", p + ".cross_attn.query", p + ".query_norm", tag + "/hq", b[tag + "/xa"], dY, dY,
                           need_dx=below)
        if self.ctx_group:       # the weight gradient where it was; no context-side dX here
            self.dlin_ln(plan, dkvc, tag + "/cn", p + ".cross_attn.kv", p + ".context_norm", 2 * H)
            self.flush_deferred(plan)
            return
        self.norm_lin_back(plan, self.F_LNL, dkvc, 2 * H, tag + "/cn", p + ".cross_attn.kv", p + ".context_norm", tag + "/hc", b["context"],
                           dctx_in, b["d/ctx"], need_dx=ctx)

    # ------------------------------------------------------------------ backward (segments fire DDP hooks)
    def needs(self):
        """Where the two gradient streams are still needed: a namespace of
          tok[side, slot]  (token_embed, projection, mod_emb / pos_embed) of a tokeniser take a gradient,
          ctx              d/ctx is needed: something upstream of the context is trainable,
          enc_below[i] / dec_below[i]    a launch behind encoder / decoder layer i reads the stream,
          dec_cross[i] / dec_mlp[i]      ... behind the cross-attention / the MLP block of decoder layer i,
          enc_mlp[i], enc_top, dec_top   ... behind the MLP block of encoder layer i, behind the bridge, behind decoder_norm."""
        c, t, tl = self.c, self.trainable, self.tl
        n = type("Needs", (), {})()
        n.tok = {}
        for side, mods in self.mods_of.items():
            for slot, (m, mod, _) in enumerate(mods):
                p = f"{side}_embeddings.{mod}.embedder"
                emb = [f"{c.mod_emb_owner(side, mod)}_embeddings.{mod}.embedder.mod_emb.weight"] + ([p + ".pos_embed.weight"] if self.sides[side].pos else [])
                # (a stitched modality's read-in takes its gradient through the token_embed's input gradient: d/z is needed for it too)
                n.tok[side, slot] = (tl(p + ".token_embed") or (m in self.st and t(self.sess_names(m, "in"))), tl(p + ".projection"), t(emb))
        bottom = {side: any(any(v) for (s, _), v in n.tok.items() if s == side) for side in ("encoder", "decoder")}
        layer = lambda side, i: t([k for k in self.e.layout.entries if k.startswith(f"{side}.{i}.")])
        enc = [layer("encoder", i) for i in range(c.n_enc)]
        n.enc_below = [bottom["encoder"] or any(enc[:i]) for i in range(c.n_enc)]
        n.enc_mlp = [tl(f"encoder.{i}.attn.qkv", f"encoder.{i}.ln1") or tl(f"encoder.{i}.attn.out_proj") or n.enc_below[i] for i in range(c.n_enc)]
        n.enc_top = bottom["encoder"] or any(enc)
        n.ctx = n.enc_top or tl("decoder_proj_context", "encoder_norm")
        # d/ctx needs every layer's d/kvc, and with it the stream down to layer 0's cross-attention
        dec = [layer("decoder", i) or n.ctx for i in range(c.n_dec)]
        n.dec_below = [bottom["decoder"] or any(dec[:i]) for i in range(c.n_dec)]
        n.dec_cross = [tl(f"decoder.{i}.attn.qkv", f"decoder.{i}.ln1") or tl(f"decoder.{i}.attn.out_proj") or n.dec_below[i] for i in range(c.n_dec)]
        n.dec_mlp = [n.ctx or n.dec_cross[i] or tl(f"decoder.{i}.cross_attn.out_proj") or tl(f"decoder.{i}.cross_attn.query", f"decoder.{i}.query_norm")
                     or tl(f"decoder.{i}.cross_attn.kv", f"decoder.{i}.context_norm") for i in range(c.n_dec)]
        n.dec_top = bottom["decoder"] or any(dec)
        return n

    def backward(self, refresh=True):
        e, c, b, buf = self.e, self.c, self.b, self.buf
        B, T, H, I, R, BT, Lq = self.B, self.T, self.H, self.Imax, self.R, self.BT, self.Lq
        nd = self.needs()
        dY, dydec = buf("d/stream", (R, H)), buf("d/ydec", (R, H))
        buf("d/t1", (R, H)); buf("d/t2", (R, H)); buf("d/h", (R, H)); buf("d/u", (R, I)); buf("d/qkv", (R, 3 * H)); dctx = buf("d/ctx", (R, H))
        ydec = b["ydec"]
        tokmask = b[self.mk("decoder", "tokmask")]
        # decoder_norm's backward reads d/ydec of every modality: it runs for the stream's sake or for its own parameters'
        norm = self.keep("decoder_norm", nd.dec_top or self.trainable(self.norm_names("decoder_norm")), self.norm_names("decoder_norm"))
        for j, (m, mod, n) in enumerate(self.mods_of["decoder"]):
            BT, (r0, r1), off = self.BTm[m], self.ydec_rows(j), self.off["decoder"][j]
            width, n = n, self.nd[m]
            dpred = buf(f"d/pred/{m}", (BT, n))
            ch = self.chan_rows(m, tokmask, off)
            s_out = m in self.st and self.keep(f"session_out.{mod}", self.trainable(self.sess_names(m, "out")), self.sess_names(m, "out"))
            if ch is not None:
                if norm or self.tl(f"decoder_embeddings.{mod}.out") or s_out:
                    K.masked_loss_chan_bwd(*self.loss_spec(mod), b[f"pred/{m}"], b[f"tgt/{m}"], ch[0], ch[1], self.Tm[m], BT, n, ch[2],
                                           b["gout"], b["inv_n"], dpred, plan=self.cur)
            elif (norm or self.tl(f"decoder_embeddings.{mod}.out")) and self.elem_tm(m) is not None and c.loss_kind[mod] == L.LOSS_SOFTMAX_CE:
                self.softmax_ce(self.cur, m, mod, b[f"pred/{m}"], b[f"tgt/{m}"], self.elem_tm(m), self.Tm[m], self.Tm[m], BT, n, dpred=dpred)
            elif (norm or self.tl(f"decoder_embeddings.{mod}.out") or s_out) and self.elem_tm(m) is not None:
                K.masked_loss_elem_bwd(*self.loss_spec(mod), b[f"pred/{m}"], b[f"tgt/{m}"], self.elem_tm(m), B, self.Tm[m], n,
                                       b["gout"], b["inv_n"], dpred, plan=self.cur)
            elif (norm or self.tl(f"decoder_embeddings.{mod}.out")) and c.loss_kind[mod] == L.LOSS_SOFTMAX_CE:
                self.softmax_ce(self.cur, m, mod, b[f"pred/{m}"], b[f"tgt/{m}"], tokmask[:, off:], Lq, self.Tm[m], BT, n, dpred=dpred)
            elif norm or self.tl(f"decoder_embeddings.{mod}.out"):
                self.loss(self.cur, mod, K.masked_loss_bwd, K.masked_loss_kind_bwd, b[f"pred/{m}"], b[f"tgt/{m}"], tokmask[:, off:],
                          Lq, self.Tm[m], BT, n, b["gout"], b["inv_n"], dpred)
            if m in self.st:        # dpred -> df = dpred . Wout (the head's output gradient), and the read-out's own gradients
                df = buf(f"d/sess/f/{m}", (BT, width))
                if norm or self.tl(f"decoder_embeddings.{mod}.out"):
                    K.session_reduce(self.sess_desc(m, "out", bias=False), dpred, df, plan=self.cur)
                if s_out:
                    self.sess_dw(self.cur, m, "out", dpred, b[f"sess/f/{m}"])
                dpred, n = df, width
            self.dlin(self.cur, dpred, ydec[r0:r1], f"decoder_embeddings.{mod}.out", BT, n, H, dX=dydec[r0:r1], need_dx=norm)
        if norm:
            self.ln_b(self.cur, dydec, self.dec_last, "decoder_norm", "decnorm", None, dY, **self.destitch())
        self.close_segment("head")
        buf("d/qc", (R, H))
        if self.ctx_group:
            for i in range(c.n_dec):
                buf(f"d/kvc/{i}", (R, 2 * H))
        else:
            buf("d/kvc", (R, 2 * H))
        for i in reversed(range(c.n_dec)):
            p, tag = f"decoder.{i}", f"dec{i}"
            self.mlp_back(self.cur, dY, p, tag, b[tag + "/yb"], below=nd.dec_mlp[i])
            # the last layer writes d/ctx, the others add (pruned plan: d/ctx is needed from every layer or from none, nd.ctx)
            self.cross_back(self.cur, dY, p, tag, None if i == c.n_dec - 1 else dctx, below=nd.dec_cross[i], ctx=nd.ctx)
            self.self_back(self.cur, dY, p, tag, self.dec_flags, below=nd.dec_below[i])
            self.close_segment(p)
        if c.n_dec == 0:
            raise NotImplementedError("n_dec == 0")
        # now dY = d(dec_tokens + dec_emb) and dctx = d(context); context = ctx_proj(enc_out) + encoder_emb (mm.py:292)
        dX = buf("d/xstream", (R, H))
        if self.ctx_group and nd.ctx:
            self.context_back(self.cur, dctx)
        self.norm_lin_back(self.cur, self.F_LNL, dctx, H, "encnorm", "decoder_proj_context", "encoder_norm", "enc_out", self.enc_last, None, dX,
                           need_dx=nd.enc_top)
        self.close_segment("bridge")
        for i in reversed(range(c.n_enc)):
            p, tag = f"encoder.{i}", f"enc{i}"
            self.mlp_back(self.cur, dX, p, tag, b[tag + "/xa"], below=nd.enc_mlp[i])
            self.self_back(self.cur, dX, p, tag, self.enc_flags, below=nd.enc_below[i])
            self.close_segment(p)
        # tokenisers: decoder side first (it overwrites the shared mod_emb gradient row, the encoder side adds).  The encoder side adds
        # only where a decoder tokeniser really wrote that row: a table no decoder tokeniser shares gets its gradient by overwriting,
        # and a table the decoder owns gets its own.  Pruned plan: a tokeniser's stitch backward runs if its d/tok or one of its tables
        # is needed.  The decoder-side writer of a shared row and the encoder-side adder read the same table's flag, so they run or go
        # together wherever that table takes a gradient; an adder left alone adds into a row nobody reads
        shared = {mod for _, mod, _ in self.mods_of["decoder"] if c.mod_emb_owner("decoder", mod) == "encoder"}
        for side, dS, dextra in (("decoder", dY, None), ("encoder", dX, dctx)):
            sd = self.sides[side]
            for slot, (m, mod, n) in enumerate(self.mods_of[side]):
                pS = f"{side}_embeddings.{mod}.embedder"
                emb = [f"{c.mod_emb_owner(side, mod)}_embeddings.{mod}.embedder.mod_emb.weight"] + ([pS + ".pos_embed.weight"] if sd.pos else [])
                if self.keep(pS + ".mod_emb+pos_embed", any(nd.tok[side, slot]), emb):
                    self.stitch_b(self.cur, side, slot, dS, dextra, acc_mod=side == "encoder" and mod in shared)
        # the softsign gradient from the activation itself (bf16), or from the saved pre-activation (fp32, and every other activation)
        s_in = {m: self.keep(f"session_in.{c.mods[m][0]}", self.trainable(self.sess_names(m, "in")), self.sess_names(m, "in")) for m in self.st}
        du_written = set()
        for side in ("decoder", "encoder"):
            sd = self.sides[side]
            saved = self.embed_saved(sd)
            for slot, (m, mod, n) in enumerate(self.mods_of[side]):
                p = f"{side}_embeddings.{mod}.embedder"
                n2 = n * sd.mult
                lv = self.lv.get((side, slot))
                BT = self.BTm[m]
                dz = self.rows(buf(f"d/z/{m}", (BT, n * self.mult_max)), BT, n2)
                self.dlin(self.cur, b[f"d/tok/{side}/{m}"], b[f"{side}/a/{m}"], p + ".projection", BT, H, n2, dX=dz, need_dx=nd.tok[side, slot][0],
                          act=L.ACT_SOFTSIGN_GRAD_OUT if saved == "a" else sd.emb_grad, act_scale=sd.scale,
                          gradmul_pre=b[f"{side}/{saved}/{m}"] if saved else None, live=lv)
                # a stitched modality's read-in: du [BT, P] = sum over the sides of dz . W_token_embed (the second side adds through the
                # residual epilogue), then its weight gradients from the padded batch and du
                du = dict(dX=buf(f"d/sess/u/{m}", (BT, n)), **(dict(residual=b[f"d/sess/u/{m}"], ldr=n) if m in du_written else {})) if s_in.get(m) else {}
                self.dlin(self.cur, dz, b[f"in/{m}"] if lv is None else b[self.mk(side, f"in_live/{m}")], p + ".token_embed", BT, n2, n,
                          ldx=_align(n, 8), live=lv, **du)
                if du:
                    du_written.add(m)
        for m in self.st:
            if s_in[m] and m in du_written:
                self.sess_dw(self.cur, m, "in", b[f"sin/{m}"], b[f"d/sess/u/{m}"])
        self.close_segment("embed")
        if self.used_wt and refresh:            # refresh the bf16 transposes once per step, in front of everything (the optimiser rewrote the weights)
            tw = e._wt_table()
            K.prep_weights(tw["table"], tw["n"], tw["tiles"], plan=self.fwd)
            self.fwd.insert(0, self.fwd.pop())
