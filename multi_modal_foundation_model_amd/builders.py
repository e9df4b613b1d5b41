"""Builders shared by bench.py, scripts/ and the tests: the API mirror's model exactly as train_multi_modal.py builds it
(train_multi_modal.py:160-210: construction order = RNG contract)."""
import copy
import os

import torch

import sys

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "src")
if SRC not in sys.path:
    sys.path.insert(0, SRC)


def load_config():
    from utils.config_utils import config_from_kwargs, update_config
    cwd = os.getcwd()
    os.chdir(os.path.dirname(SRC))          # config paths are 'src/configs/...' relative, like the reference
    try:
        cfg = config_from_kwargs({"model": "include:src/configs/multi_modal/mm.yaml"})
        cfg = update_config("src/configs/multi_modal/trainer_mm.yaml", cfg)
    finally:
        os.chdir(cwd)
    return cfg


def model_config(H=None, heads=None, inter=None, n_enc=None, n_dec=None, max_F=None, dropout=None, emb_dropout=None,
                 sep=None, causal=None, n_modality=None, scalenorm=None, act=None, attn_bias=None, mlp_bias=None):
    """attn_bias / mlp_bias (transformer.attention_bias / mlp_bias): a bool for both sides or an (encoder, decoder) pair."""
    from utils.config_utils import DictConfig
    m = copy.deepcopy(dict(load_config()["model"]))
    for key, val in (("attention_bias", attn_bias), ("mlp_bias", mlp_bias)):
        if val is not None:
            enc, dec = val if isinstance(val, (tuple, list)) else (val, val)
            m["encoder"]["transformer"][key], m["decoder"]["transformer"][key] = bool(enc), bool(dec)
    for side in ("encoder", "decoder"):
        e, t = m[side]["embedder"], m[side]["transformer"]
        if max_F is not None: e["max_F"] = max_F
        if n_modality is not None: e["n_modality"] = n_modality
        if emb_dropout is not None: e["dropout"] = emb_dropout
        if H is not None: t["hidden_size"] = H
        if heads is not None: t["n_heads"] = heads
        if inter is not None: t["inter_size"] = inter
        if dropout is not None: t["dropout"] = dropout
        if scalenorm is not None: t["use_scalenorm"] = bool(scalenorm)
        if act is not None: t["act"] = act
    if n_enc is not None: m["encoder"]["transformer"]["n_layers"] = n_enc
    if n_dec is not None: m["decoder"]["transformer"]["n_layers"] = n_dec
    if sep is not None: m["decoder"]["decoder_sep_mask"] = sep
    if causal is not None: m["decoder"]["decoder_causal_mask"] = causal
    return DictConfig(m)


def tiny_config(**kw):
    base = dict(H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8, dropout=0.0, emb_dropout=0.0)
    base.update(kw)
    return model_config(**base)


def _filtered(mods, modal_filter):
    """(encoder modalities, decoder modalities) of `modal_filter` = dict(input=[...], output=[...]) (train_multi_modal.py), each in the
    order the filter names them - the construction order, which is the RNG contract; None: every modality on both sides."""
    if modal_filter is None:
        return list(mods), list(mods)
    chan = dict(mods)
    return [(m, chan[m]) for m in modal_filter["input"]], [(m, chan[m]) for m in modal_filter["output"]]


def build_model(mcfg, n_ap, n_beh, seed=None, modal_filter=None, share_modality_embeddings=True, input_masking=False, neuron_padding=False,
                context_mask=False, sessions=None, per_sample_mask=False):
    """train_multi_modal.py:160-189 (construction order = RNG contract).  modal_filter: dict(input=[...], output=[...]), the
    modalities the encoder / the decoder gets tokenisers for (None: both get both).  input_masking: MultiModal.input_masking.
    neuron_padding: MultiModal.neuron_padding.  context_mask: MultiModal.context_mask.  per_sample_mask: MultiModal.per_sample_mask.  sessions: the ordered eid -> n_k mapping of a
    `use_session: true` config (n_ap is then not read: the stitched modalities run at stitcher.width)."""
    return build_model_mods(mcfg, [("ap", n_ap), ("behavior", n_beh)], seed=seed, modal_filter=modal_filter,
                            share_modality_embeddings=share_modality_embeddings, input_masking=input_masking, neuron_padding=neuron_padding,
                            context_mask=context_mask, sessions=sessions, per_sample_mask=per_sample_mask)


def build_model_mods(mcfg, mods, seed=None, modal_filter=None, share_modality_embeddings=True, input_masking=False, neuron_padding=False,
                     context_mask=False, sessions=None, per_sample_mask=False):
    """Same construction order for an arbitrary modality list [(name, channels)] (BASELINE configs[4]: 3 modalities).  Under
    `use_session: true` the stitched modalities' tokenisers and heads are built with n_channel = stitcher.width, whatever `mods` says,
    and MultiModal creates the session layers of `sessions` behind everything else."""
    from multi_modal.mm import MultiModal
    from multi_modal.encoder_embeddings import EncoderEmbedding
    from multi_modal.decoder_embeddings import DecoderEmbedding
    from multi_modal.session_layers import read_stitch_config
    use, st = read_stitch_config(mcfg)
    if use:
        mods = [(m, st.width if m in st.mods else n) for m, n in mods]
    if seed is not None:
        torch.manual_seed(seed)
    enc_mods, dec_mods = _filtered(mods, modal_filter)
    enc = {m: EncoderEmbedding(hidden_size=mcfg.encoder.transformer.hidden_size, n_channel=n, config=mcfg.encoder) for m, n in enc_mods}
    dec = {m: DecoderEmbedding(hidden_size=mcfg.decoder.transformer.hidden_size, n_channel=n, output_channel=n, config=mcfg.decoder)
           for m, n in dec_mods}
    return MultiModal(enc, dec, avail_mod=[m for m, _ in mods], config=mcfg, share_modality_embeddings=share_modality_embeddings,
                      **({"input_masking": True} if input_masking else {}), **({"neuron_padding": True} if neuron_padding else {}),
                      **({"context_mask": True} if context_mask else {}), **({"sessions": sessions} if sessions is not None else {}),
                      **({"per_sample_mask": per_sample_mask} if per_sample_mask is not False else {}))


def make_optimizer(model, total_steps, lr=1e-4, wd=0.01, eps=1e-8):
    from torch.optim.lr_scheduler import OneCycleLR
    from multi_modal_foundation_model_amd.optim import make_optimizer as mk
    opt = mk(model, lr=lr, weight_decay=wd, eps=eps)
    sch = OneCycleLR(optimizer=opt, total_steps=total_steps, max_lr=lr, pct_start=0.15, div_factor=10)
    return opt, sch
