"""The train-step engine: MultiModal forward / backward as a pre-bound plan of HIP kernel launches.

Reference path: `MultiModal.forward` (src/multi_modal/mm.py:242-308) + autograd of it
(`loss.backward()`, src/trainer/base.py:194-195).  Design (MI355X-first, not a translation):

* all parameters live in ONE flat fp32 buffer (`P`), gradients in a second (`G`); the nn.Module
  parameters of the API mirror are views into it.  The layout is forward order so that the
  gradient ranges complete back-to-front during backward: the DDP wrapper all-reduces contiguous
  buckets of `G` as soon as backward passes their start, overlapped with the rest of backward.
  Q/K/V (and cross-attention K/V) weights are adjacent, so one GEMM does the fused projection.
* activations/workspaces are allocated once per batch shape; a step is a fixed list of
  (C function, bound arguments) pairs -> no per-step allocation, marshalling or host sync, and
  the list can be captured into a hipGraph (`Engine.capture`).
* backward is written by hand (no autograd graph): LayerNorm backward fuses the residual-gradient
  add, dX GEMMs fuse the activation derivative, dW GEMMs are split-K over the token dimension with
  a deterministic slab reduction, dropout masks are regenerated from a counter RNG.
* there is no CPU / eager fallback: everything below calls libmmfm_hip.so.
"""
from __future__ import annotations

import itertools
import math
import os
from collections import namedtuple
from dataclasses import InitVar, dataclass, field, fields
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import ops as K
from .plan import PlanBuilder, _align, chan_buf, combine_chan, elem_buf, mask_key, read_switches

LOSS_KIND = {"ap": 0, "behavior": 1}       # mm.py:79-82: PoissonNLL(log_input) / MSE
HEAD_DIMS = (8, 16, 32, 64, 128)           # hidden_size / n_heads the attention kernels are instantiated for (csrc/attention.hip check_common)
MAX_PATTERNS = 4                           # freeze patterns per batch shape whose training plans (and graphs) are kept, most recently used
BLOCK_NORMS = ("ln1", "ln2", "query_norm", "context_norm")     # the sites `use_scalenorm` switches (encoder_norm / decoder_norm stay LayerNorm)


# what a side ("encoder" / "decoder") of the model runs with: EngineConfig.side
SideConfig = namedtuple("SideConfig", "heads inter dropout norm act embed_scale embed_dropout mult max_F embed_act embed_pos embed_bias attn_bias mlp_bias")
# The EngineConfig fields that have one value per side (the two YAML sections are independent): each holds ONE value, meaning both
# sides, or Sides(encoder, decoder).  A plain (encoder, decoder) tuple or list is taken as Sides too - for `act`, whose one value is
# itself a (kind, beta) pair, a pair of pairs.  __post_init__ folds a pair of equal values into the one value, so a config that names
# one value equals the config that names it twice, and the default config is field for field what it always was
PER_SIDE = ("heads", "inter", "dropout", "norm", "act", "embed_scale", "embed_dropout", "mult", "max_F")
# The embedder options (embedder.act / pos / bias), per side in the same way.  They are constructor keywords and attributes of the config but
# not dataclass fields (InitVar): the field list, asdict() and the constructor calls from before they existed are what they were
PER_SIDE_EMBED = ("embed_act", "embed_pos", "embed_bias")
# The modality sets of the two sides (modal_filter) and whether their tokenisers share mod_emb tables: constructor keywords and attributes
# like the embedder options, and like them no dataclass fields
MODAL = ("enc_mods", "dec_mods", "share_mod_emb")
# The class weights of the softmax cross-entropy modalities (loss_kind 7): a constructor keyword and attribute like the two groups above
# and like them no dataclass field - the field list, asdict() and the default config stay what they were
LOSS_EXTRA = ("loss_weight",)
# The attention window over time stamps (mm.yaml context.forward / context.backward under MultiModal.context_mask): a constructor keyword
# and attribute like the groups above, no dataclass field.  None - the default, and what (-1, -1) folds into - is today's model
CONTEXT = ("context",)
# The per-session read-in / read-out layers (use_session): `sessions` maps a stitched modality to the neuron counts of its
# sessions, in session-index order; such a modality's entry in `mods` carries the shared width P (what its tokenisers and its head run
# at).  stitch_bias: the session layers have biases.  Constructor keywords and attributes like the groups above, no dataclass fields;
# None - the default - is today's model
SESSION = ("sessions", "stitch_bias")
# Per-sample token masking (MultiModal.per_sample_mask): every sample's tokens are zeroed where its OWN mask is 1, not where
# sample 0's is.  A constructor keyword and attribute like the groups above, no dataclass field.  False - the default - is today's model
TOKEN_MASK = ("per_sample_mask",)
Sides = namedtuple("Sides", "encoder decoder")


@dataclass
class EngineConfig:
    # (the PER_SIDE fields - heads, inter, max_F, mult, embed_scale, embed_dropout, dropout, norm, act - hold the annotated type or a Sides of it)
    hidden: int
    heads: int
    inter: int
    n_enc: int
    n_dec: int
    max_F: int
    mult: int
    n_modality: int
    embed_scale: float
    embed_dropout: float
    dropout: float
    sep_mask: bool
    causal_mask: bool
    mods: List[Tuple[str, int]]                 # (name, channels) in avail_mod order
    loss_kind: Dict[str, int] = field(default_factory=lambda: dict(LOSS_KIND))    # modality -> MMFM_LOSS_* kind
    # per modality, for the kinds that have them (absent = 0): the kind's float (PoissonNLL eps, SmoothL1 beta, Huber delta) and its
    # flags (L.LOSS_FULL = PoissonNLLLoss(full=True)).  A modality of kind 0 / 1 without flags runs the two-kind entry points
    loss_param: Dict[str, float] = field(default_factory=dict)
    loss_flags: Dict[str, int] = field(default_factory=dict)
    norm: str = "layernorm"                     # the transformer blocks' norms: "layernorm" or "scalenorm" (use_scalenorm: true)
    act: Tuple[int, float] = (L.MLP_GELU, 1.0)  # the MLP activation (transformer.act): (MMFM_MLP_* kind, sigmoid beta), ops.mlp_act
    # transformer.attention_bias / transformer.mlp_bias, per side (the two YAML sections are independent): False = the side's
    # attn / cross_attn query, key, value, out_proj (attention) or mlp up_proj, down_proj (mlp) are nn.Linear(bias=False)
    enc_attn_bias: bool = True
    enc_mlp_bias: bool = True
    dec_attn_bias: bool = True
    dec_mlp_bias: bool = True
    # the embedder options, per side like the fields above (one value or Sides): embedder.act (a name of ops.EMBED_ACTS), embedder.pos
    # (False: no pos_embed table, emb = mod_emb row) and embedder.bias (False: token_embed is nn.Linear(bias=False))
    embed_act: InitVar[str] = "softsign"
    embed_pos: InitVar[bool] = True
    embed_bias: InitVar[bool] = True
    # modal_filter (train_multi_modal.py): the modalities the encoder / the decoder has tokenisers (and the decoder heads) for, names out
    # of `mods`; None = all of them.  Held in `mods` order, whatever order they were named in; a list that names every modality is
    # folded into None, so the config that names them all equals the config that names none.  share_mod_emb
    # (share_modality_embeddings): a decoder tokeniser of a modality the encoder has too reads the ENCODER's mod_emb table (mm.py:84-87);
    # False, or a modality the encoder lacks: the decoder tokeniser owns its table.  Read through `side_mods` / `mod_emb_owner`
    enc_mods: InitVar[Optional[List[str]]] = None
    dec_mods: InitVar[Optional[List[str]]] = None
    share_mod_emb: InitVar[bool] = True
    # loss_kind[mod] = L.LOSS_SOFTMAX_CE: loss_param[mod] is the label smoothing and loss_weight[mod] the class weights, one per channel
    # of the head (absent: 1).  Tuples, so that __eq__ and the plan pool compare them by value; uploaded once per engine
    loss_weight: InitVar[Optional[Dict[str, Tuple[float, ...]]]] = None
    # (context.forward, context.backward), both ints >= -1, or None: the encoder's self-attention and the cross-attention see a key only
    # inside the window over the tokens' time stamps (ops.context_window translates).  (-1, -1) is None
    context: InitVar[Optional[Tuple[int, int]]] = None
    sessions: InitVar[Optional[Dict[str, Tuple[int, ...]]]] = None
    stitch_bias: InitVar[bool] = True
    per_sample_mask: InitVar[bool] = False
    # `hidden` has no per-side form (decoder_proj_context is H -> H and cross-attention reads the encoder's rows), nor has
    # `n_modality` (a shared mod_emb is one tensor, mm.py:84-87, and the row is the modality's index in `mods` on either side).  Read a
    # side's values through `side()`

    def __post_init__(self, embed_act="softsign", embed_pos=True, embed_bias=True, enc_mods=None, dec_mods=None, share_mod_emb=True,
                      loss_weight=None, context=None, sessions=None, stitch_bias=True, per_sample_mask=False):
        if not isinstance(per_sample_mask, bool):
            raise ValueError(f"EngineConfig.per_sample_mask = {per_sample_mask!r}: True or False")
        self.per_sample_mask = per_sample_mask
        if sessions is not None:
            names = [m for m, _ in self.mods]
            sessions = {m: tuple(int(n) for n in sizes) for m, sizes in sessions.items()}
            for m, sizes in sessions.items():
                if m not in names or not sizes or any(n < 1 for n in sizes):
                    raise ValueError(f"EngineConfig.sessions[{m!r}] = {sizes}: a modality out of {names} and one neuron count >= 1 per session")
            sessions = sessions or None
        self.sessions, self.stitch_bias = sessions, bool(stitch_bias)
        if context is not None:
            context = tuple(context)
            if len(context) != 2:
                raise ValueError(f"EngineConfig.context = {context!r}: (forward, backward) or None")
            K.context_window(*context)              # refuses what is not an int >= -1
            context = None if context == (-1, -1) else context
        self.context = context
        self.embed_act, self.embed_pos, self.embed_bias = embed_act, embed_pos, embed_bias
        self.loss_weight = {m: tuple(float(x) for x in w) for m, w in (loss_weight or {}).items()}
        names = [m for m, _ in self.mods]
        for k, v in (("enc_mods", enc_mods), ("dec_mods", dec_mods)):
            if v is not None:
                v = list(v)
                unknown = [m for m in v if m not in names]
                if unknown or not v or len(set(v)) != len(v):
                    raise ValueError(f"EngineConfig.{k} = {v}: a non-empty list of distinct names out of mods {names}")
                v = [m for m in names if m in v]
            setattr(self, k, None if v == names else v)
        self.share_mod_emb = bool(share_mod_emb)
        for k in PER_SIDE + PER_SIDE_EMBED:
            v = getattr(self, k)
            pair = isinstance(v, (tuple, list)) and len(v) == 2 and (k != "act" or isinstance(v[0], (tuple, list)))
            if pair:
                enc, dec = (tuple(x) for x in v) if k == "act" else v
                setattr(self, k, enc if enc == dec else Sides(enc, dec))

    def __eq__(self, other):
        if other.__class__ is not self.__class__:
            return NotImplemented
        return all(getattr(self, k) == getattr(other, k) for k in tuple(f.name for f in fields(self)) + PER_SIDE_EMBED + MODAL + LOSS_EXTRA + CONTEXT + SESSION + TOKEN_MASK)

    __hash__ = None

    def side(self, side: str) -> SideConfig:
        """The per-side quantities of "encoder" or "decoder"."""
        if side not in ("encoder", "decoder"):
            raise ValueError(f"EngineConfig.side({side!r})")
        vals = (getattr(self, k) for k in PER_SIDE + PER_SIDE_EMBED)
        return SideConfig(*(getattr(v, side) if isinstance(v, Sides) else v for v in vals),
                          attn_bias=getattr(self, side[:3] + "_attn_bias"), mlp_bias=getattr(self, side[:3] + "_mlp_bias"))

    def side_mods(self, side: str) -> List[Tuple[int, str, int]]:
        """The modalities "encoder" or "decoder" has tokenisers for, in `mods` order: (index in `mods`, name, channels).  The index is the
        modality's mod_emb row (mod_to_indx) and names its buffers; its place in this list is its slot in the side's stitched sequence."""
        if side not in ("encoder", "decoder"):
            raise ValueError(f"EngineConfig.side_mods({side!r})")
        own = self.enc_mods if side == "encoder" else self.dec_mods
        return [(m, mod, n) for m, (mod, n) in enumerate(self.mods) if own is None or mod in own]

    def stitched(self, m: int):
        """The neuron counts of the sessions of modality index m where it is stitched (use_session), else None."""
        return None if not self.sessions else self.sessions.get(self.mods[m][0])

    def data_width(self, m: int) -> int:
        """The channels of modality m's inputs, targets and predictions: its tokenisers' channels, or - stitched - the largest session."""
        sizes = self.stitched(m)
        return self.mods[m][1] if sizes is None else max(sizes)

    def mod_emb_owner(self, side: str, mod: str) -> str:
        """The side whose tokeniser of `mod` owns the mod_emb table the tokeniser of `side` reads: the encoder's for a decoder tokeniser
        that shares it (mm.py:84-87), else `side` itself."""
        if side == "decoder" and self.share_mod_emb and (self.enc_mods is None or mod in self.enc_mods):
            return "encoder"
        return side

    def is_scalenorm(self, lnname: str) -> bool:
        """True where the norm named `lnname` is a ScaleNorm: a block norm (BLOCK_NORMS) of a side with use_scalenorm: true.
        `decoder.{i}.query_norm` and `context_norm` are the decoder's; encoder_norm / decoder_norm are LayerNorms always."""
        return lnname.rsplit(".", 1)[-1] in BLOCK_NORMS and self.side(lnname.split(".", 1)[0]).norm == "scalenorm"

    @staticmethod
    def from_model_config(mc, mods, per_side: bool = False, embedder_opts: bool = False, enc_mods=None, dec_mods=None,
                          share_mod_emb: bool = True, context_window: bool = False, sessions=None, stitch_bias: bool = True,
                          per_sample_mask: bool = False) -> "EngineConfig":
        """per_side = True (what MultiModal passes): every PER_SIDE quantity is read from its own section.  per_side = False, the
        two-argument call from before the sections were independent, keeps its contract for callers that rely on it: transformer
        sections that differ in n_heads, inter_size or dropout raise ValueError, in use_scalenorm or act NotImplementedError, as they
        always did (the embedder's keys are read per side either way: the decoder's used to be ignored without a word).
        embedder_opts = True (what MultiModal passes): embedder.act, pos and bias are read per side too (embed_act / embed_pos /
        embed_bias; an act without a kernel raises NotImplementedError naming the accepted ones).  Without it the call keeps the
        contract it had: any act but softsign, pos: false and bias: false raise NotImplementedError.
        enc_mods / dec_mods / share_mod_emb: the config's fields of those names (modal_filter, share_modality_embeddings).
        context_window = True (what MultiModal passes under its context_mask switch): context.forward / context.backward are read into
        `context` - a value that is not an int >= -1 raises ValueError here.  Without it the two keys are not looked at, as upstream.
        per_sample_mask = True (what MultiModal passes under its switch of that name): the field of that name."""
        context = None
        if context_window:
            ctx = mc["context"]
            context = (ctx["forward"], ctx["backward"])
        tf = {side: mc[side]["transformer"] for side in ("encoder", "decoder")}
        em = {side: mc[side]["embedder"] for side in ("encoder", "decoder")}
        et, dtf, ee = tf["encoder"], tf["decoder"], em["encoder"]
        if not per_side:
            for k in ("n_heads", "inter_size", "dropout"):
                if et[k] != dtf[k]:
                    raise ValueError(f"encoder/decoder transformer.{k} differ ({et[k]} vs {dtf[k]}): pass per_side=True to read each section for its side")
            if bool(et["use_scalenorm"]) != bool(dtf["use_scalenorm"]):
                raise NotImplementedError("use_scalenorm differs between encoder and decoder: pass per_side=True to read each section for its side")
            if et["act"] != dtf["act"]:
                raise NotImplementedError(f"transformer.act differs between encoder and decoder ({et['act']} vs {dtf['act']}): pass per_side=True "
                                          "to read each section for its side")
        if et["hidden_size"] != dtf["hidden_size"]:
            raise ValueError(f"encoder/decoder transformer.hidden_size differ ({et['hidden_size']} vs {dtf['hidden_size']}): not supported - "
                             "decoder_proj_context is hidden -> hidden and cross-attention reads the encoder's rows, so the two "
                             "stacks share one width")
        hs, per = int(et["hidden_size"]), {}
        for side in ("encoder", "decoder"):
            t, e = tf[side], em[side]
            if embedder_opts:
                K.embed_act(e["act"])
            elif e["act"] != "softsign":
                raise NotImplementedError(f"{side}.embedder.act={e['act']!r}: only act=softsign (embedder) is read by this call; pass "
                                          "embedder_opts=True for the other embedder activations")
            elif not e["pos"] or not e["bias"]:
                raise NotImplementedError(f"{side}.embedder.pos / bias = false: pass embedder_opts=True to read the embedder's act, pos and bias")
            nh = int(t["n_heads"])
            if nh <= 0 or hs % nh:
                raise ValueError(f"{side}.transformer.hidden_size {hs} is not a multiple of n_heads {nh}: the attention kernels take a "
                                 f"head dim in {HEAD_DIMS}")
            if hs // nh not in HEAD_DIMS:
                raise ValueError(f"{side}.transformer.hidden_size {hs} / n_heads {nh} = head dim {hs // nh}: the attention kernels take "
                                 f"a head dim in {HEAD_DIMS}")
            per[side] = dict(heads=t["n_heads"], inter=t["inter_size"], dropout=t["dropout"],
                             norm="scalenorm" if t["use_scalenorm"] else "layernorm", act=K.mlp_act(t["act"]),
                             embed_scale=float(hs ** 0.5 if e["scale"] is None else e["scale"]), embed_dropout=e["dropout"],
                             mult=e["mult"], max_F=e["max_F"], embed_act=str(e["act"]), embed_pos=bool(e["pos"]), embed_bias=bool(e["bias"]))
        return EngineConfig(hidden=et["hidden_size"], n_enc=et["n_layers"], n_dec=dtf["n_layers"], n_modality=ee["n_modality"],
                            sep_mask=bool(mc["decoder"]["decoder_sep_mask"]), causal_mask=bool(mc["decoder"]["decoder_causal_mask"]),
                            mods=list(mods), **{k: Sides(per["encoder"][k], per["decoder"][k]) for k in PER_SIDE + (PER_SIDE_EMBED if embedder_opts else ())},
                            enc_attn_bias=bool(et["attention_bias"]), enc_mlp_bias=bool(et["mlp_bias"]),
                            dec_attn_bias=bool(dtf["attention_bias"]), dec_mlp_bias=bool(dtf["mlp_bias"]),
                            enc_mods=enc_mods, dec_mods=dec_mods, share_mod_emb=share_mod_emb, context=context,
                            sessions=sessions, stitch_bias=stitch_bias, per_sample_mask=per_sample_mask)


# a block's linear: name, the norm that feeds it (None: plain), weight [N, K], has a bias, the adjacent nn.Linear's a fused projection aliases
Lin = namedtuple("Lin", "name norm N K bias parts")


def block_linears(cfg: EngineConfig, side: str, i: int) -> List[Lin]:
    """THE description of a block: the linears of encoder / decoder layer i (or of the "bridge" between the two stacks) in forward
    (= parameter) order.  ParamLayout, the prepared weights of the fused path (Engine._build_prep) and the plan's workspace sizing all
    read the model's structure from here."""
    H, p = cfg.hidden, f"{side}.{i}"
    if side == "bridge":
        return [Lin("decoder_proj_context", "encoder_norm", H, H, True, None)]
    sc = cfg.side(side)
    I, ab, mb = sc.inter, sc.attn_bias, sc.mlp_bias
    attn = [Lin(p + ".attn.qkv", p + ".ln1", 3 * H, H, ab, ("query", "key", "value")), Lin(p + ".attn.out_proj", None, H, H, ab, None)]
    cross = [Lin(p + ".cross_attn.query", p + ".query_norm", H, H, ab, None),
             Lin(p + ".cross_attn.kv", p + ".context_norm", 2 * H, H, ab, ("key", "value")),
             Lin(p + ".cross_attn.out_proj", None, H, H, ab, None)]
    mlp = [Lin(p + ".mlp.up_proj", p + ".ln2", I, H, mb, None), Lin(p + ".mlp.down_proj", None, H, I, mb, None)]
    return attn + (cross if side == "decoder" else []) + mlp


def model_linears(cfg: EngineConfig) -> List[Lin]:
    """Every block linear of the model in forward order: encoder layers, the bridge, decoder layers."""
    return [l for side, n in (("encoder", cfg.n_enc), ("bridge", 1), ("decoder", cfg.n_dec)) for i in range(n) for l in block_linears(cfg, side, i)]


class ParamLayout:
    """name -> (offset, shape) in the flat buffer; `groups` are the DDP buckets' atoms."""

    def __init__(self, cfg: EngineConfig):
        for side in ("encoder", "decoder"):
            if cfg.side(side).norm not in ("layernorm", "scalenorm"):
                raise ValueError(f"EngineConfig.norm ({side}) = {cfg.side(side).norm!r}")
        H = cfg.hidden
        self.entries: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.alias: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.segments: List[Tuple[str, int, int]] = []       # (segment name, start, end) in forward order
        self.n = 0

        def add(name, shape):
            self.entries[name] = (self.n, tuple(shape))
            self.n += int(math.prod(shape))

        def pad():
            self.n = _align(self.n)

        def lin(prefix, o, i, bias=True, parts=None):
            """weight [o, i] and (bias: a bias-free linear has no entry and leaves no slot behind) bias [o], each in its own aligned slot.
            parts: the adjacent nn.Linear's it is made of, one entry each; `prefix` then is an alias over them."""
            for kind, shape in ((".weight", (o, i)), (".bias", (o,)))[:2 if bias else 1]:
                pad()
                if not parts:
                    add(prefix + kind, shape)
                    continue
                self.alias[prefix + kind] = (self.n, shape)
                for nm in parts:
                    add(f"{prefix.rsplit('.', 1)[0]}.{nm}{kind}", (o // len(parts),) + shape[1:])

        def ln(prefix):
            if cfg.is_scalenorm(prefix):                   # the side that owns the norm decides
                pad(); add(prefix + ".scale", ())          # ScaleNorm's 0-dim gain, its own aligned slot (mm_utils.py:31-35)
                return
            pad(); add(prefix + ".weight", (H,)); pad(); add(prefix + ".bias", (H,))

        def layer(lins):
            """The norms of a run of norm-fed linears lie in front of the run (query_norm, context_norm, then cross_attn.query, kv)."""
            for j, l in enumerate(lins):
                if l.norm and (j == 0 or not lins[j - 1].norm):
                    for nl in itertools.takewhile(lambda nl: nl.norm, lins[j:]):
                        ln(nl.norm)
                lin(l.name, l.N, l.K, l.bias, l.parts)

        def segment(name, fill):
            pad()
            s = self.n
            fill()
            pad()
            self.segments.append((name, s, self.n))

        def embed():
            for side in ("encoder", "decoder"):
                sc = cfg.side(side)
                for _, mod, n in cfg.side_mods(side):       # (a side has no slot for a modality it has no tokeniser for)
                    p = f"{side}_embeddings.{mod}.embedder"
                    lin(p + ".token_embed", n * sc.mult, n, bias=sc.embed_bias)
                    lin(p + ".projection", H, n * sc.mult)
                    # a decoder tokeniser's mod_emb IS the encoder's tensor where the two share it (mm.py:84-87): no slot.  One of a
                    # modality the encoder lacks, or of an unshared model, owns its table
                    if cfg.mod_emb_owner(side, mod) == side:
                        pad(); add(p + ".mod_emb.weight", (cfg.n_modality, H))
                    if sc.embed_pos:            # embedder.pos: false builds no pos_embed module
                        pad(); add(p + ".pos_embed.weight", (sc.max_F, H))
            session("session_in", lambda n, width: (width,))

        def session(prefix, bias_shape):
            """The session layers of the stitched modalities, behind everything else of their segment: per session a [n_k, P] weight and
            (stitch_bias) its bias, each in its own aligned slot."""
            for m, (mod, width) in enumerate(cfg.mods):
                for k, n in enumerate(cfg.stitched(m) or ()):
                    pad(); add(f"{prefix}.{mod}.{k}.weight", (n, width))
                    if cfg.stitch_bias:
                        pad(); add(f"{prefix}.{mod}.{k}.bias", bias_shape(n, width))

        def head():
            ln("decoder_norm")
            for _, mod, n in cfg.side_mods("decoder"):
                lin(f"decoder_embeddings.{mod}.out", n, H)
            session("session_out", lambda n, width: (n,))

        segment("embed", embed)
        for side, n in (("encoder", cfg.n_enc), ("bridge", 1), ("decoder", cfg.n_dec)):
            for i in range(n):
                segment("bridge" if side == "bridge" else f"{side}.{i}", lambda: layer(block_linears(cfg, side, i)))
        segment("head", head)
        self.n = _align(self.n, 64)

    def has(self, name):
        return name in self.entries or name in self.alias

    def view(self, flat, name):
        off, shape = self.entries[name] if name in self.entries else self.alias[name]
        return flat[off: off + int(math.prod(shape))].view(shape)


class _StepFn(torch.autograd.Function):
    """Connects the engine to `loss.backward()` (trainer/base.py:194-195)."""

    @staticmethod
    def forward(ctx, anchor, engine, token):
        ctx.engine, ctx.token = engine, token
        return engine.b["loss"].clone().reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        ctx.engine.backward(grad_out, ctx.token)
        return None, None, None


class Engine:
    def __init__(self, cfg: EngineConfig, device, dtype: str = "fp32", seed: int = 0):
        if cfg.hidden % cfg.side("encoder").heads or cfg.hidden % cfg.side("decoder").heads:
            raise ValueError("Hidden dim is not multiple of head size")
        if dtype not in ("fp32", "bf16"):
            raise ValueError(dtype)
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the MI355X engine needs a CUDA/HIP device; there is no CPU fallback "
                               "(the CPU restatement lives in oracle/ and is test infrastructure only)")
        L.check(L.lib().mmfm_device_check(self.device.index or 0), "mmfm_device_check")
        self.dtype = dtype
        self.adt = torch.float32 if dtype == "fp32" else torch.bfloat16
        self.code = L.F32 if dtype == "fp32" else L.BF16
        self.layout = ParamLayout(cfg)
        n = self.layout.n
        self.P = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.G = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.Pw = self.P if dtype == "fp32" else torch.zeros(n, dtype=torch.bfloat16, device=self.device)
        self.rng = torch.zeros(2, dtype=torch.int32, device=self.device)
        K.rng_seed(self.rng, seed)
        self.params: Dict[str, torch.nn.Parameter] = {}
        self.adoptions = 0               # bumped by adopt(): whoever caches facts about `params` (the optimiser) re-derives them
        self.plans: Dict[Tuple, dict] = {}
        # Buffers are owned per batch shape (B, T): a plan (and its captured hipGraphs) holds raw device pointers, so a
        # buffer must never be re-allocated while a plan that names it is alive.  `self.b` is the pool of the shape in
        # use; pools (with their plans) are evicted least-recently-used beyond MMFM_MAX_SHAPES.
        self._pools: Dict[Tuple[int, int], Dict[str, torch.Tensor]] = {}
        self._pool_lru: List[Tuple[int, int]] = []
        # Training plans are also owned per freeze pattern (`freeze_pattern`): the backward of a pattern launches only what its trainable
        # parameters need.  Per batch shape the MAX_PATTERNS most recently used patterns keep their plans and graphs
        self._pattern_lru: Dict[Tuple[int, int], list] = {}
        self._pattern = None
        # ... and per element-mask pattern (`elem_key`: the compact shapes of each modality's corruption and target mask, whose strides
        # are launch arguments of the plan): again the MAX_PATTERNS most recently used per batch shape
        self._elem_lru: Dict[Tuple[int, int], list] = {}
        self.max_shapes = max(1, int(os.environ.get("MMFM_MAX_SHAPES", "4")))
        self._shared: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, torch.Tensor] = self._shared
        self._shape = None
        self._token = 0
        self._fwd_token = -1
        self._sites: Dict[str, int] = {}
        self.linears = model_linears(cfg)
        self._prep = None                                             # prepared weights of the fused path (_build_prep)
        self._wt = dict(views={}, entries=[], table=None)             # bf16 transposes for the big-GEMM dX products (_w_transposed)
        self.grad_ready_hooks = []       # DDP: callables(segment_name) fired as backward completes a segment of G
        self.backward_done_hooks = []    # DDP: wait for the collectives (stream-side) before anyone reads G
        self.forward_done_hooks = []     # DDP over per-session layers: callables() fired behind a forward that takes a gradient
        self._shared_tables: Dict[str, dict] = {}
        self._absent = frozenset()       # the parameters of the sessions without a sample in the last forward's batch (use_session)
        self._stash = None               # G's size, allocated by the first backward that accumulates (caller skipped zero_grad()), never before
        self._param_spans, self._spans_of = [], -1
        # hipGraph replay of the step plan: the plan neither allocates nor synchronises, so after one eager
        # (warm-up) run per batch shape it is captured once and replayed.  MMFM_GRAPH=0 disables.
        self.use_graphs = os.environ.get("MMFM_GRAPH", "1") != "0"
        self._shared["loss"] = torch.zeros(1, device=self.device)
        self._shared["inv_n"] = torch.zeros(1, device=self.device)
        self._shared["gout"] = torch.ones(1, device=self.device)
        # softmax cross-entropy modalities: the label smoothing is checked and the class weights are uploaded here, once per engine
        # (a modality without weights, or of another kind, has no entry: the launches pass NULL)
        self.loss_w: Dict[str, torch.Tensor] = {}
        chans = dict(cfg.mods)
        for mod, kind in cfg.loss_kind.items():
            w = getattr(cfg, "loss_weight", {}).get(mod)
            if kind != L.LOSS_SOFTMAX_CE:
                continue
            if not 0.0 <= float(cfg.loss_param.get(mod, 0.0)) <= 1.0:
                raise ValueError(f"EngineConfig.loss_param[{mod!r}] = {cfg.loss_param[mod]}: the label smoothing must be in [0, 1]")
            if w is not None:
                if len(w) != chans.get(mod) or any(not x >= 0 for x in w):
                    raise ValueError(f"EngineConfig.loss_weight[{mod!r}]: {len(w)} class weights for a head of {chans.get(mod)} channels "
                                     "(one non-negative weight per channel)")
                self.loss_w[mod] = torch.tensor(w, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ parameters
    def adopt(self, named_params: Dict[str, torch.nn.Parameter]):
        """Copy the module's parameters into the flat buffer and re-point them at views of it."""
        missing = set(self.layout.entries) - set(named_params)
        extra = set(named_params) - set(self.layout.entries)
        if missing or extra:
            raise KeyError(f"parameter set mismatch: missing {sorted(missing)[:4]}, unexpected {sorted(extra)[:4]}")
        with torch.no_grad():
            for name, p in named_params.items():
                v = self.layout.view(self.P, name)
                if tuple(p.shape) != tuple(v.shape):
                    raise ValueError(f"{name}: shape {tuple(p.shape)} != {tuple(v.shape)}")
                v.copy_(p.data.to(self.device, torch.float32))
                p.data = v
                p.grad = None
                self.params[name] = p
        self.adoptions += 1
        self.refresh_weights()

    def owns(self, named_params) -> bool:
        """True while the module's parameters are still views of our flat buffer (e.g. `.to()` breaks it)."""
        lo, hi = self.P.data_ptr(), self.P.data_ptr() + self.P.numel() * 4
        return all(lo <= p.data_ptr() < hi for p in named_params.values())

    def owns_one(self, p) -> bool:
        lo = self.P.data_ptr()
        return p.device == self.P.device and lo <= p.data_ptr() < lo + self.P.numel() * 4

    def refresh_weights(self):
        """bf16 mode: refresh the bf16 weight copy from the fp32 master (the fused AdamW does it itself)."""
        if self.dtype == "bf16":
            K.cast_bf16(self.P, self.Pw, self.P.numel())

    def W(self, name):
        return self.layout.view(self.Pw, name)

    def Pf(self, name):          # fp32 master view (LayerNorm affine, biases, embedding tables)
        return self.layout.view(self.P, name)

    def Gv(self, name):
        return self.layout.view(self.G, name)

    def Pb(self, wname):         # the bias of linear `wname` (fp32 master view), None for a bias-free linear (attention_bias / mlp_bias: false)
        return self.Pf(wname + ".bias") if self.layout.has(wname + ".bias") else None

    def Gb(self, wname):         # its gradient, None likewise
        return self.Gv(wname + ".bias") if self.layout.has(wname + ".bias") else None

    def session_tables(self, m):
        """The device tables of stitched modality m (EngineConfig.sessions), made once: n int32 [S] and the element offsets (int64 [S]) of
        every session's read-in / read-out weight and bias in the flat buffers (P, Pw and G share the layout)."""
        key = f"sess/tables/{m}"
        if key not in self._shared_tables:
            mod, sizes, ent = self.cfg.mods[m][0], self.cfg.stitched(m), self.layout.entries
            off = lambda which, kind: torch.tensor([ent[f"session_{which}.{mod}.{k}.{kind}"][0] for k in range(len(sizes))], dtype=torch.int64,
                                                   device=self.device)
            t = dict(n=torch.tensor(sizes, dtype=torch.int32, device=self.device), w_in=off("in", "weight"), w_out=off("out", "weight"))
            if self.cfg.stitch_bias:
                t.update(b_in=off("in", "bias"), b_out=off("out", "bias"))
            self._shared_tables[key] = t
        return self._shared_tables[key]

    def is_sn(self, lnname):
        """True where the norm named `lnname` is a ScaleNorm (the block norms of a side with use_scalenorm: true)."""
        return self.cfg.is_scalenorm(lnname)

    # ------------------------------------------------------------------ buffers
    def _select_pool(self, B, T):
        """Make the buffer pool of batch shape (B, T) current (creating it, and evicting the least recently used
        shape - pool, plans and graphs together - beyond `max_shapes`)."""
        key = (B, T)
        pool = self._pools.get(key)
        if pool is None:
            while len(self._pools) >= self.max_shapes:
                old = self._pool_lru.pop(0)
                torch.cuda.synchronize(self.device)          # nothing may still be replaying the evicted graphs
                for pk in [k for k in self.plans if (k[0], k[1]) == old]:
                    del self.plans[pk]
                del self._pools[old]
                self._pattern_lru.pop(old, None)
                self._elem_lru.pop(old, None)
            pool = dict(self._shared)
            self._pools[key] = pool
        if key in self._pool_lru:
            self._pool_lru.remove(key)
        self._pool_lru.append(key)
        self.b = pool
        return pool

    def _buf(self, name, shape, dtype=None, zero=False):
        dtype = self.adt if dtype is None else dtype
        t = self.b.get(name)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            self.b[name] = t
        elif tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            raise RuntimeError(f"engine buffer {name}: {tuple(t.shape)}/{t.dtype} re-requested as {tuple(shape)}/{dtype} "
                               "inside one batch-shape pool (plans hold raw pointers; buffers are never re-allocated)")
        return t

    def _site(self, key):
        if key not in self._sites:
            self._sites[key] = len(self._sites) + 1
        return self._sites[key]

    def _drop(self, key, p):
        return K.dropout(self.rng, self._site(key), p) if p > 0 else None

    # ------------------------------------------------------------------ row-owner fused path (bf16, width 256 / 512)
    def _fused_mask(self, R, sw=None):
        """Which op groups run as row-owner fused kernels (csrc/rowchain.h): bit 0 ln1+qkv, bit 1 the other LayerNorm-fed
        linears (cross-attention query / key-value, decoder_proj_context), bit 2 the MLP block, bit 3 attention out_proj.
        MMFM_FUSED overrides (0 = the un-fused kernels of round 1).  Bits 0, 1 and 3 (K = 256 linears) hold for both sides; bit 2
        holds for the sides whose inter_size is 512 (`fused_mlp`), the other side runs the un-fused up / down GEMMs.  A model
        with no such side stays on the un-fused kernels altogether, as it always has."""
        c, sw = self.cfg, sw or read_switches()
        if self.dtype != "bf16" or c.hidden != 256 or 512 not in (c.side("encoder").inter, c.side("decoder").inter) or (R + 128) * 1024 * 2 >= 2 ** 31:
            return 0
        if R < 12288 and sw.fused is None:
            # a row-owner pass is 128 rows: below ~100 passes per launch the grid cannot fill 256 CUs.  Since round 4 the forward-type linears
            # split N into column blocks there (rowgemm.hip), which makes the LayerNorm-fed linears and out_proj worth fusing at the reference's
            # batch of 16 too; the MLP kernels (chained products, no column split) stay off.  ms/step un-fused / 11 / 15: B=16 4.45 / 4.08 / 4.19,
            # B=32 4.85 / 4.71 / -, B=64 5.46 / 5.50 / 5.48 (R = 12,800: the default 15)
            return 11
        return (15 if sw.fused is None else sw.fused) & 15        # default: everything fused, the fastest end to end (35.6 vs 36.3 ms)

    def fused_mlp(self, side, fm):
        """True where the MLP blocks of `side` run the row-owner MLP kernels under fused mask `fm` (csrc/mlp_fused.hip: inter 512)."""
        return bool(fm & 4) and self.cfg.side(side).inter == 512

    # ------------------------------------------------------------------ bf16 transposes for the compute-bound dX products
    def _w_transposed(self, wname, N, Kd, Mr, sw=None):
        """W^T [Kd, N] (bf16) of an nn.Linear weight [N, Kd] when its dX = dY[Mr, N] . W belongs to the 256-tile GEMM (csrc/gemm_big.hip:
        reduction N a multiple of 64 and >= 512; d_model-512 configurations and any layer this wide): that kernel wants both operands
        reduction-contiguous.  The views are refreshed by ONE mmfm_prep_weights launch at the top of every training step."""
        if not (sw or read_switches()).gemm_big or N < 512 or N % 64 or Kd % 8 or Kd < 128 or Mr < 1024:
            return None
        reg = self._wt
        if wname not in reg["views"]:
            t = torch.zeros(Kd, N, dtype=torch.bfloat16, device=self.device)
            reg["views"][wname] = t
            reg["entries"].append(dict(W=self.Pf(wname + ".weight"), WpT=t))
            reg["table"] = None
        return reg["views"][wname]

    def _wt_table(self):
        reg = self._wt
        if reg["table"] is None:
            table, n, tiles = K.prep_table(reg["entries"], self.device)
            reg["table"] = dict(table=table, n=n, tiles=tiles)
        return reg["table"]

    def _build_prep(self):
        """Prepared weights of the fused path: per LayerNorm-fed linear Wp = bf16(W * gamma), WpT, bp = b + W beta
        (mmfm_prep_weights); per ScaleNorm-fed linear Wp = bf16(g * W), bp = b (scalar gain); per plain linear only the bf16
        transpose (the dX products read K-contiguous rows).  A bias-free linear behind a LayerNorm keeps bp = W beta (beta is folded
        into the linear either way); behind a ScaleNorm it has no bp at all (None: the consuming kernel adds nothing)."""
        if self._prep is not None:
            return self._prep
        sites = [(l.name, l.norm) for l in self.linears]
        nW = sum(self.Pf(w + ".weight").numel() for w, _ in sites)
        nWp = sum(self.Pf(w + ".weight").numel() for w, ln in sites if ln)
        has_bp = {w: self.Pb(w) is not None or not self.is_sn(ln) for w, ln in sites if ln}
        nb = sum(self.Pf(w + ".weight").shape[0] for w, ln in sites if ln and has_bp[w])
        # unit-permuted copies for the MLP kernels' LDS-DMA weight ring (include/mmfm.h: mmfm_prep_entry.WpP / WpTP)
        # (only for the sides whose MLP blocks the kernels take: inter 512)
        mlp_up = {w for w, _ in sites if w.endswith(".mlp.up_proj") and self.fused_mlp(w.split(".", 1)[0], 4)}
        mlp_down = {w for w, _ in sites if w.endswith(".mlp.down_proj") and self.fused_mlp(w.split(".", 1)[0], 4)}
        nPm = sum(self.Pf(w + ".weight").numel() for w in mlp_up | mlp_down)
        WpT = torch.zeros(nW + 64, dtype=torch.bfloat16, device=self.device)
        Wp = torch.zeros(nWp + 64, dtype=torch.bfloat16, device=self.device)
        Wpm = torch.zeros(nPm + 64, dtype=torch.bfloat16, device=self.device)
        bp = torch.zeros(nb + 64, dtype=torch.float32, device=self.device)
        views, entries, oT, oW, ob, oP = {}, [], 0, 0, 0, 0
        for w, ln in sites:
            Wm = self.Pf(w + ".weight")
            N, Kd = Wm.shape
            e = dict(W=Wm, WpT=WpT[oT:oT + N * Kd].view(Kd, N))
            oT += N * Kd
            v = dict(WpT=e["WpT"])
            if w in mlp_up:                         # backward: d(x_hat) += W_up^T[:, tile] . du, du an accumulator tile
                e["WpTP"] = v["WpTP"] = Wpm[oP:oP + N * Kd].view(Kd, N)
                oP += N * Kd
            elif w in mlp_down:                     # forward: y += W_down[:, tile] . g, g an accumulator tile
                e["WpP"] = v["WpP"] = Wpm[oP:oP + N * Kd].view(N, Kd)
                oP += N * Kd
            if ln:
                if self.is_sn(ln):
                    e.update(gamma=self.Pf(ln + ".scale"), scalar_gain=True)
                else:
                    e.update(gamma=self.Pf(ln + ".weight"), beta=self.Pf(ln + ".bias"))
                e.update(bias=self.Pb(w), Wp=Wp[oW:oW + N * Kd].view(N, Kd), bp=bp[ob:ob + N] if has_bp[w] else None)
                oW += N * Kd
                ob += N if has_bp[w] else 0
                v.update(Wp=e["Wp"], bp=e["bp"])
            views[w] = v
            entries.append(e)
        table, n, tiles = K.prep_table(entries, self.device)
        self._prep = dict(table=table, n=n, tiles=tiles, v=views, keep=(WpT, Wp, Wpm, bp, entries))
        return self._prep

    # ------------------------------------------------------------------ plan construction
    def _dw_split(self, M, N, R, ldn=None, sw=None):
        """Split-K factor for a dW GEMM ([M,N] output, reduction over R tokens).
        bf16 shapes the streaming kernel takes (csrc/gemm_dw.hip: 16-B aligned rows of dY [R, M] and X [R, ldn]): ONE (tile, K-slab) item per CU - the slab
        traffic is items x 64 KB, so fewer, longer items beat filling the chip three times over.
        Otherwise (fp32 parity path, the 668-wide tokeniser shapes): tiles x splits fills the persistent grid of the 128-tile
        kernel (256 CUs x 3 workgroups) exactly once - measured against 512 items at B = 1024: qkv dW 182 -> 155 us, token-embed
        dW 639 -> 508 us - capped at 128 slabs (the slab reduction costs S x M x N x 4 bytes)."""
        tiles = -(-M // 128) * -(-N // 128)
        stream = self.code == L.BF16 and M % 8 == 0 and (ldn or N) % 8 == 0 and (sw or read_switches()).gemm_dw
        if stream:
            tiles = L.lib().mmfm_gemm_dw_tiles(M, N, R)
        if R <= 8192:                     # launch-bound regime (reference batch 16 -> R = 3200): <= 15 slabs = one-stage reduce
            S = max(1, min(R // 256, 15))
        elif stream:
            S = max(1, min(R // 512, 256 // tiles))
        else:
            S = max(1, min(R // 512, max(1, 768 // tiles), 128))
        kchunk = _align(-(-R // S), 64)          # multiple of both kernels' BK (32 fp32, 64 bf16)
        return -(-R // kchunk), kchunk

    def freeze_pattern(self):
        """The requires_grad flags of the adopted parameters in layout order, or None while every one is True (or nothing is adopted):
        what a plan with a backward is keyed by besides its batch shape and mode."""
        if not self.params:
            return None
        pattern = tuple(self.params[name].requires_grad for name in self.layout.entries)
        return None if all(pattern) else pattern

    def elem_key(self, elem):
        """What an element-masked plan is keyed by besides the rest: per modality (cfg.mods order) None or the compact shapes of its
        (corruption mask, target mask) - the broadcast pattern, since B, T and N are fixed.  None: no modality carries element masks."""
        if elem is None or all(e is None for e in elem):
            return None
        if len(elem) != len(self.cfg.mods):
            raise ValueError(f"engine: {len(self.cfg.mods)} modalities, {len(elem)} element-mask entries")
        return tuple(None if e is None else (tuple(e[0].shape), None if e[1] is None else tuple(e[1].shape)) for e in elem)

    def fold_chan(self, B, T, elem, chan):
        """Folds the channel masks `chan` (per modality None or u8 [B or 1, N]; neuron padding) into the element masks:
        returns (elem', chan', padded) with plan.combine_chan applied per modality - elem' carries every such modality's staging mask,
        chan' the channel mask of those whose loss runs the chan form, padded the modalities that came with a channel mask.  chan None
        or all None: (elem, None, ()), the call it always was."""
        if chan is None or all(v is None for v in chan):
            return elem, None, ()
        mods = self.cfg.mods
        if len(chan) != len(mods) or (elem is not None and len(elem) != len(mods)):
            raise ValueError(f"engine: {len(mods)} modalities, {len(chan)} channel-mask entries")
        elem = list(elem) if elem is not None else [None] * len(mods)
        out = [None] * len(mods)
        width = getattr(self.cfg, "data_width", lambda m: mods[m][1])       # (a stitched modality's mask spans its largest session)
        for m, v in enumerate(chan):
            if v is not None:
                if elem[m] is not None and torch.is_tensor(v) and v.device != elem[m][0].device:      # the masker's masks live where it drew them
                    v = v.to(elem[m][0].device)
                elem[m], out[m] = combine_chan(elem[m], v, B, T[m] if isinstance(T, tuple) else T, width(m))
        return elem, (None if all(v is None for v in out) else out), tuple(m for m, v in enumerate(chan) if v is not None)

    @staticmethod
    def chan_key(chan):
        """What a channel-masked plan is keyed by besides the rest: per modality None or the shape of its channel mask."""
        return None if chan is None else tuple(None if v is None else tuple(v.shape) for v in chan)

    def plan_key(self, B, T, training, grad=True, pattern=None, elem=None):
        """The key of a step plan in `plans`.  Without a context window (EngineConfig.context None) the keys are what they always were:
        (B, T, training, grad), with the freeze pattern behind it where there is one, and the six-entry form (..., pattern, elem) for an
        element-masked plan.  Under a window the key is always the six-entry form with ("window", lo, hi) behind it; under per-sample
        token masks (EngineConfig.per_sample_mask) the marker ("rows",) stands behind the six-entry form, or behind the window's entry."""
        rows = (("rows",),) if getattr(self.cfg, "per_sample_mask", False) else ()       # (a config from before the switch has none)
        if self.cfg.context is not None:
            return (B, T, bool(training), bool(grad), pattern, elem, ("window",) + K.context_window(*self.cfg.context)) + rows
        if rows:
            return (B, T, bool(training), bool(grad), pattern, elem) + rows
        if elem is not None:
            return (B, T, bool(training), bool(grad), pattern, elem)
        return (B, T, bool(training), bool(grad)) + (() if pattern is None else (pattern,))

    def _plan(self, B, T, training, grad=True, pattern=None, elem=None, chan=None):
        """The cached step plan of (batch shape, mode, freeze pattern); built by plan.PlanBuilder the first time.
        grad = False: a forward-only plan (evaluation under no_grad) that skips the tensors saved for the backward.
        pattern (`freeze_pattern`; None: all trainable, the key and the plan are what they always were): the plan's backward is pruned
        to what the trainable parameters need.  A forward-only plan has no pattern.
        elem (`elem_key`; None: the key and the plan are what they always were): the modalities whose loss runs under a per-element
        mask, with the masks' compact shapes.
        chan (`chan_key`; None: the key and the plan are what they always were): the modalities whose loss runs under a channel mask.
        Such plans are pooled with the element-masked ones, under `mask_key`."""
        pattern = pattern if grad else None
        elem_arg, elem = elem, mask_key(elem, chan)
        key = self.plan_key(B, T, training, grad, pattern, elem)
        self._select_pool(B, T)
        if grad:
            lru = self._pattern_lru.setdefault((B, T), [])
            if pattern in lru:
                lru.remove(pattern)
            lru.append(pattern)
            while len(lru) > MAX_PATTERNS:
                old = lru.pop(0)
                torch.cuda.synchronize(self.device)          # nothing may still be replaying the dropped graphs
                for pk in [k for k in self.plans if k[:2] == (B, T) and k[3] and (k[4] if len(k) > 4 else None) == old]:
                    del self.plans[pk]
        if key not in self.plans:
            frozen = None if pattern is None else [name for name, on in zip(self.layout.entries, pattern) if not on]
            self.plans[key] = PlanBuilder(self, B, T, training, grad, frozen=frozen, elem=elem_arg, chan=chan).build()
        if elem is not None:                # (behind the build: a refused mask shape leaves no trace)
            lru = self._elem_lru.setdefault((B, T), [])
            if elem in lru:
                lru.remove(elem)
            lru.append(elem)
            while len(lru) > MAX_PATTERNS:
                old = lru.pop(0)
                torch.cuda.synchronize(self.device)          # nothing may still be replaying the dropped graphs
                for pk in [k for k in self.plans if k[:2] == (B, T) and len(k) > 5 and k[5] == old]:
                    del self.plans[pk]
        return self.plans[key]

    def backward_report(self, B, T):
        """What the backward of the training plan of batch shape (B, T) launches under the current freeze pattern:
          segments  [(segment name, launches of this plan, launches of the all-trainable plan)] in backward order,
          pruned    the gradient groups none of whose launches is emitted (a linear with its bias - and, on the fused path, the norm
                    that feeds it; a stand-alone norm; a tokeniser's mod_emb + pos_embed),
          pruned_params      the parameters no emitted launch writes the gradient of (G is unspecified in their spans),
          launches / full    the two totals.
        Read-only, builds nothing and launches nothing: the plan must exist (one training forward ran at this shape and pattern)."""
        pattern = self.freeze_pattern()
        key = self.plan_key(B, T, True, True, pattern)
        if key not in self.plans:
            # element-masked plans (input masking) have keys of their own: the most recently used one of this shape and pattern.  Their
            # backward differs from the plain plan's in the loss launches' entry points alone
            for elem in reversed(self._elem_lru.get((B, T), [])):
                if self.plan_key(B, T, True, True, pattern, elem) in self.plans:
                    key = self.plan_key(B, T, True, True, pattern, elem)
                    break
        if key not in self.plans:
            raise KeyError(f"backward_report({B}, {T}): no training plan of this shape under the current freeze pattern has been built yet")
        rep = self.plans[key]["report"]
        return dict(segments=list(rep["segments"]), pruned=list(rep["pruned"]), pruned_params=list(rep["pruned_params"]), launches=sum(s[1] for s in rep["segments"]),
                    full=sum(s[2] for s in rep["segments"]))

    def backward_summary(self, B, T):
        """`backward_report` as one line."""
        r = self.backward_report(B, T)
        live = [f"{name} {n}/{full}" for name, n, full in r["segments"] if n]
        return (f"backward: {r['launches']} of {r['full']} launches, {len(r['pruned'])} gradient groups pruned; "
                f"segments with launches: {', '.join(live) if live else 'none'}")

    def dropout_sites(self, B, T):
        """Read-only description of the dropout sites of the built training plan of batch shape (B, T), for tests that read the masks
        back off the kernels: one dict per site with
          key    the site's name (`{side}/embdrop/{m}`, `<tag>/p`, `<tag>/o`, `<tag>/mlpdrop`),
          site   its id in the counter hash, p its drop probability,
          kind   "flat" (counter row * N + col over shape (R, N): GEMM epilogue / mmfm_dropout_apply / stitch_bwd / attention drop_o),
                 "rowdrop" (the fused MLP's row-keyed hash over (R, 256)) or "attn" (drop_p over (B, heads, Lq, Lk)),
          shape  as above, and for "attn" also dh and keepbits: the site's keep-bit workspace, or None when both directions hash.
        Builds nothing and launches nothing: the plan must exist (one training forward ran at this shape)."""
        plan = self.plans[self.plan_key(B, T, True, True)]
        c = self.cfg
        Tm = (lambda m: T[m]) if isinstance(T, tuple) else (lambda m: T)          # a segmented plan: per-modality lengths
        H, Lq = c.hidden, sum(Tm(m) for m, _, _ in c.side_mods("encoder"))
        out = []
        for key, site in self._sites.items():
            side = "encoder" if key.startswith("enc") else "decoder"          # `encoder/embdrop/0`, `enc0/sa/p`, `dec1/mlpdrop`
            sc = c.side(side)
            if "/embdrop/" in key:
                d = dict(p=sc.embed_dropout, kind="flat", shape=(B * Tm(int(key.rsplit("/", 1)[1])), H))
            elif key.endswith("/mlpdrop"):
                d = dict(p=sc.dropout, kind="rowdrop" if self.fused_mlp(side, plan["fused"]) else "flat", shape=(B * Lq, H))
            elif key.endswith("/o"):
                d = dict(p=sc.dropout, kind="flat", shape=(B * Lq, H))
            else:
                d = dict(p=sc.dropout, kind="attn", shape=(B, sc.heads, Lq, Lq), dh=H // sc.heads,
                         keepbits=plan["b"].get(key[:-2] + "/keep") if plan["use_keep"] else None)
            out.append(dict(key=key, site=site, **d))
        return out

    def _run(self, plan, which, entries_fn, tag=None):
        """Run a piece of the plan: eagerly the first time (lazy one-off initialisation such as the >64 KB LDS
        opt-in must not happen inside a capture), then capture it into a hipGraph and replay."""
        tag = which if tag is None else tag
        g = plan["graphs"].get(tag)
        if g is not None:
            g.replay()
            return
        if not self.use_graphs or plan["runs"][which] < 1:
            entries_fn()
            return
        graph = torch.cuda.CUDAGraph()
        # thread_local: with the DDP wrapper the previous bucket's all-reduce may still be running on RCCL's stream while the next
        # backward segment is captured; the default (global) mode would treat that foreign-stream activity as a capture violation
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            entries_fn()
        plan["graphs"][tag] = graph
        graph.replay()

    # ------------------------------------------------------------------ data in
    def load_inputs(self, B, T, inputs, targets, masks, ts, attn, elem=None, chan=None, padded=(), sess=None):
        """Copy one batch into the static input buffers (device tensors or host tensors).  T a tuple (a segmented plan): modality m
        has T[m] bins and its own stamps ts[m] and attention mask attn[m].  elem[m] = (cm, tm, corrupted or None): the modality's
        element masks go into their static buffers, and its inputs are staged by mmfm_stage_masked - zeroed under cm on the way - or,
        where the masker corrupted them itself, copied from `corrupted`.  chan[m] (with elem[m] from `combine_chan`: tm may be None):
        the modality's channel mask goes into its static buffer.  padded: the modalities whose cm holds padded channels (`fold_chan`) -
        their inputs are always staged by mmfm_stage_masked; for `corrupted` inputs cm is the padding alone (plan.combine_chan), so the
        masker's noise and kept values stay and only the padded channels are zeroed."""
        seg = isinstance(T, tuple)
        dec = {m for m, _, _ in self.cfg.side_mods("decoder")}
        for m in sorted(dec | {m for m, _, _ in self.cfg.side_mods("encoder")}):      # (a modality no side has is not staged)
            Tm = T[m] if seg else T
            e = elem[m] if elem is not None else None
            if e is not None:
                cm, tm, corrupted = e
                cmb = self.b[elem_buf("cm", m, cm.shape)]
                cmb.copy_(cm, non_blocking=True)
                if tm is not None:
                    self.b[elem_buf("tm", m, tm.shape)].copy_(tm, non_blocking=True)
            if chan is not None and chan[m] is not None:
                self.b[chan_buf(m, chan[m].shape)].copy_(chan[m], non_blocking=True)
            stitched = self.cfg.stitched(m) is not None
            if stitched:                # the session of every sample and the run table of the weight gradients: data of the one captured plan
                sid = sess[m]
                self.b[f"sess/sid/{m}"].copy_(torch.tensor(sid, dtype=torch.int32), non_blocking=True)
                runs = K.session_runs(sid, len(self.cfg.stitched(m)), K.session_dw_chunk(B))
                self.b[f"sess/runs/{m}"].copy_(torch.from_numpy(runs), non_blocking=True)
            in_key = f"sin/{m}" if stitched else f"in/{m}"          # a stitched modality's batch is staged as it came; the read-in writes in/{m}
            if e is not None and (corrupted is None or m in padded):
                dst = self.b[in_key]
                src = (inputs[m] if corrupted is None else corrupted).to(self.device, torch.float32, non_blocking=True).contiguous()
                K.stage_masked(src, cmb, B, Tm, src.shape[-1], dst, dst.shape[-1])
            else:
                x = inputs[m] if e is None else corrupted
                self.b[in_key].view(B, Tm, -1)[..., :x.shape[-1]].copy_(x, non_blocking=True)
            if m in dec:
                tgt = self.b[f"tgt/{m}"].view(B, Tm, -1)         # (a stitched modality's batch may be narrower or wider than its largest session)
                width = min(tgt.shape[-1], targets[m].shape[-1])
                tgt[..., :width].copy_(targets[m][..., :width], non_blocking=True)
            self.b[f"mask/{m}"].copy_(masks[m], non_blocking=True)
            if seg:
                self.b[f"ts/{m}"].copy_(ts[m], non_blocking=True)
                self.b[f"attn/{m}"].copy_(attn[m], non_blocking=True)
        if not seg:
            self.b["ts"].copy_(ts, non_blocking=True)
            self.b["attn"].copy_(attn, non_blocking=True)

    def batch_key(self, T, ts, attn):
        """What a batch's plan is keyed by besides B, with its stamps and attention masks in the matching form: (T, ts, attn) with T an
        int and one tensor each - every modality has T bins and they share stamps and mask: the plan it always was - or T the tuple of
        per-modality lengths in cfg.mods order and one tensor per modality: a segmented plan.  Sharing is by identity:
        a caller that holds equal copies (MultiModal.forward compares them) passes the same tensor."""
        n = len(self.cfg.mods)
        per_mod = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
        Ts = tuple(int(t) for t in T) if isinstance(T, (list, tuple)) else (int(T),) * n
        tss, attns = per_mod(ts), per_mod(attn)
        if not (len(Ts) == len(tss) == len(attns) == n):
            raise ValueError(f"engine: {n} modalities, {len(Ts)} lengths, {len(tss)} time-stamp and {len(attns)} attention-mask tensors")
        if len(set(Ts)) == 1 and all(t is tss[0] for t in tss) and all(a is attns[0] for a in attns):
            return Ts[0], tss[0], attns[0]
        return Ts, tss, attns

    # ------------------------------------------------------------------ run
    def stitch_batch(self, B, inputs, elem, chan, sess):
        """A batch of a model with stitched modalities (EngineConfig.sessions): sess[m] = the session index of every sample of stitched
        modality m.  Returns (inputs, elem, chan, absent): chan[m] becomes v[b, c] = c < n_s(b) over the modality's full width (a
        space_attn_mask that came with it is not read); a batch narrower than that width has its inputs and element masks padded to
        it (zeros; never read beyond n_s); absent = the parameters of the sessions without a sample in this batch."""
        mods = self.cfg.mods
        if sess is None or len(sess) != len(mods):
            raise ValueError(f"engine: a model with per-session layers needs sess = one entry per modality of {[m for m, _ in mods]}")
        pad_to = lambda t, N: t if t is None or t.shape[-1] in (1, N) else torch.nn.functional.pad(t, (0, N - t.shape[-1]))
        inputs, chan, absent = list(inputs), list(chan) if chan is not None else [None] * len(mods), set()
        elem = list(elem) if elem is not None else None
        for m, (mod, _) in enumerate(mods):
            sizes = self.cfg.stitched(m)
            if sizes is None:
                if sess[m] is not None:
                    raise ValueError(f"engine: modality {mod!r} has no per-session layers, sess[{m}] must be None")
                continue
            N, sid = self.cfg.data_width(m), sess[m]
            if sid is None or len(sid) != B or any(not 0 <= int(k) < len(sizes) for k in sid):
                raise ValueError(f"engine: modality {mod!r}: sess[{m}] must hold {B} session indices in [0, {len(sizes)})")
            if len(set(sid)) > L.SESSION_MAX_PER_BATCH:
                raise ValueError(f"engine: modality {mod!r}: {len(set(sid))} distinct sessions in one batch, at most {L.SESSION_MAX_PER_BATCH} are built")
            w = inputs[m].shape[-1]
            if any(sizes[k] > w for k in sid):
                raise ValueError(f"engine: modality {mod!r}: a batch {w} channels wide for sessions of up to {max(sizes[k] for k in sid)} neurons")
            if w > N:                   # padded beyond the largest session: those columns belong to nobody and are dropped unread
                cut = lambda t: t if t is None or t.shape[-1] != w else t[..., :N]
                inputs[m] = cut(inputs[m])
                if elem is not None and elem[m] is not None:
                    elem[m] = tuple(cut(t) for t in elem[m])
                w = N
            n_b = torch.tensor([sizes[k] for k in sid], dtype=torch.int64)
            chan[m] = (torch.arange(N)[None, :] < n_b[:, None]).to(torch.uint8)
            if w < N:
                inputs[m] = pad_to(inputs[m], N)
                if elem is not None and elem[m] is not None:
                    elem[m] = tuple(pad_to(t, N) for t in elem[m])
            kinds = ("weight", "bias") if self.cfg.stitch_bias else ("weight",)
            absent |= {f"session_{which}.{mod}.{k}.{kind}" for k in set(range(len(sizes))) - set(sid) for which in ("in", "out") for kind in kinds}
        return inputs, elem, chan, frozenset(absent)

    def forward(self, B, T, inputs, targets, masks, ts, attn, training=True, anchor=None, elem=None, chan=None, sess=None):
        """T: the number of bins, or a tuple of per-modality numbers in cfg.mods order; ts / attn: one tensor [B, T], or one per modality.
        elem (None: the call it always was): per modality, in cfg.mods order, None or (cm, tm, corrupted or None) - the corruption mask
        and the target mask as uint8 tensors [B or 1, T or 1, N or 1] (Masker.element_masks) and, where the masker corrupted the inputs
        itself, the corrupted inputs.  Such a modality's loss is summed over the set elements of tm and its count is their number;
        its token mask (`masks`) is expected all zero.  DESIGN.md §3w.
        chan (None, or all None: the call it always was): per modality, in cfg.mods order, None or its channel mask, uint8 [B, N] or
        [1, N], 1 = a real channel.  Such a modality's inputs are zeroed in the other channels on both sides, its loss is summed over
        row mask x channel mask and its count is the number of those elements.  DESIGN.md §3x."""
        T, ts, attn = self.batch_key(T, ts, attn)
        seg = isinstance(T, tuple)
        want_grad = anchor is not None and torch.is_grad_enabled() and anchor.requires_grad
        self._pattern = self.freeze_pattern() if want_grad else None          # read once per forward
        self._absent = frozenset()
        if getattr(self.cfg, "sessions", None):               # (sess is read only by a model with per-session layers; None elsewhere is the call it always was)
            inputs, elem, chan, self._absent = self.stitch_batch(B, inputs, elem, chan, sess)
        elif sess is not None and any(s is not None for s in sess):
            raise ValueError("engine: sess names sessions, the model has no per-session layers (EngineConfig.sessions)")
        elem, chan, padded = self.fold_chan(B, T, elem, chan)
        ekey = self.elem_key(elem)
        plan = self._plan(B, T, training, want_grad, self._pattern, elem=ekey, chan=self.chan_key(chan))
        self.load_inputs(B, T, inputs, targets, masks, ts, attn, elem=None if ekey is None else elem, chan=chan, padded=padded, sess=sess)
        advance = training and any(sc.dropout > 0 or sc.embed_dropout > 0 for sc in map(self.cfg.side, ("encoder", "decoder")))

        def fwd_entries():
            if advance:
                K.rng_advance(self.rng)
            K.run_plan(plan["fwd"])
        self._run(plan, "fwd", fwd_entries)
        plan["runs"]["fwd"] += 1
        self._token += 1
        self._fwd_token = self._token
        self._last = plan
        # per decoder modality, in the decoder's order (all of `mods` unless dec_mods says otherwise)
        dec, count = self.cfg.side_mods("decoder"), self.b[plan["count"]]
        out = dict(mod_loss=[self.b["loss_sum"][j].clone() for j in range(len(dec))],
                   mod_n=[count[j].clone() for j in range(len(dec))],
                   preds=[self.b[f"pred/{m}"].view(B, T[m] if seg else T, -1) for m, _, _ in dec])
        if want_grad:
            for hook in self.forward_done_hooks:
                hook()
            out["loss"] = _StepFn.apply(anchor, self, self._token)
        else:
            out["loss"] = self.b["loss"].clone().reshape(())
        return out

    def backward(self, grad_out=None, token=None):
        if token is not None and token != self._fwd_token:
            raise RuntimeError("backward() must follow the forward() that produced this loss: the engine keeps one "
                               "set of activation buffers")
        if grad_out is None:
            self.b["gout"].fill_(1.0)
        else:
            self.b["gout"].copy_(grad_out.reshape(1).to(torch.float32))
        plan = self._last
        if plan["bwd"] is None:
            raise RuntimeError("backward(): the last forward ran without gradient tracking (forward-only plan)")
        if (plan["B"], plan["T"]) not in self._pools or self._pools[(plan["B"], plan["T"])] is not plan["b"]:
            raise RuntimeError("backward(): the batch shape of this loss was evicted (MMFM_MAX_SHAPES) before its backward ran")
        self.b = plan["b"]
        # caller did not zero_grad(): keep torch's += semantics.  The backward kernels overwrite G, so the accumulating runs are stashed
        # before the first launch and added back behind the launches that wrote them; the launches are not part of the plan
        runs = self.accumulating_runs()
        if runs:
            if self._stash is None:                # one persistent buffer, from the first accumulating backward on
                self._stash = torch.empty_like(self.G)
            for s, e in runs:
                K.grad_accumulate(self.G, self._stash, s, e, L.GRAD_STASH)
        if self.grad_ready_hooks:
            for name, seg in plan["bwd"]:          # DDP: one graph per segment, collectives issued in between
                if seg:                            # (a segment a pruned plan left without launches is neither run nor captured; its hook still fires)
                    self._run(plan, "bwd", lambda seg=seg: K.run_plan(seg), tag="bwd/" + name)
                if runs:
                    lo, hi = self.segment_range(name)
                    for s, e in runs:
                        if max(s, lo) < min(e, hi):
                            K.grad_accumulate(self.G, self._stash, max(s, lo), min(e, hi), L.GRAD_ADD)
                for hook in self.grad_ready_hooks:
                    hook(name)
        else:
            self._run(plan, "bwd", lambda: [K.run_plan(seg) for _, seg in plan["bwd"] if seg])
            for s, e in runs:
                K.grad_accumulate(self.G, self._stash, s, e, L.GRAD_ADD)
        plan["runs"]["bwd"] += 1
        for hook in self.backward_done_hooks:
            hook()
        # requires_grad is honoured twice: the plan of this freeze pattern launched only what the trainable parameters need (plan.py,
        # DESIGN.md §10), so G in the span of a frozen parameter is unspecified - and a frozen parameter never sees its slice
        for name, p in self.params.items():
            # a session without a sample in this batch: nothing wrote its span, .grad stays what it was.  (Under data parallelism with
            # session_sync, EngineDDP.finish has replaced the set by the sessions absent on EVERY rank: the others' spans hold the mean)
            if name in self._absent:
                continue
            if not p.requires_grad:
                p.grad = None
            elif p.grad is None or p.grad.data_ptr() != self.Gv(name).data_ptr():
                p.grad = self.Gv(name)

    def accumulating_runs(self):
        """The [start, end) ranges of G the next backward adds into instead of overwriting.  Torch's rule, per parameter: a trainable
        parameter whose .grad is not None when backward() starts accumulates; one whose .grad is None ends with this backward's gradient
        alone.  The accumulating parameters form maximal contiguous runs in layout order; alignment padding between two members joins
        their run.  Empty after zero_grad() - the ordinary step."""
        if self._spans_of != self.adoptions:          # (parameter, start, end) in layout order, rebuilt when adopt() re-points them
            self._param_spans = [(self.params[name], off, off + int(math.prod(shape))) for name, (off, shape) in self.layout.entries.items()
                                 if name in self.params]
            self._spans_of = self.adoptions
        runs, open_run = [], False
        absent = {id(self.params[name]) for name in self._absent if name in self.params}
        for p, s, e in self._param_spans:
            if p.grad is not None and p.requires_grad and id(p) not in absent:
                if open_run:
                    runs[-1][1] = e
                else:
                    runs.append([s, e])
                    open_run = True
            else:
                open_run = False
        return [(s, e) for s, e in runs]

    def segment_range(self, name):
        for n, s, e in self.layout.segments:
            if n == name:
                return s, e
        raise KeyError(name)
