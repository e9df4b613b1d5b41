"""Per-session read-in / read-out layers (`use_session: true`): a linear map from a session's n_k neurons to the shared width P in
front of the modality's tokenisers, and one from P back to n_k behind its head.

    read-in    u[b, t, :]    = sum_{c < n_s(b)} x[b, t, c] Win_s(b)[c, :] + bin_s(b)
    read-out   pred[b, t, c] = sum_p f[b, t, p] Wout_s(b)[c, p] + bout_s(b)[c]   for c < n_s(b), exactly 0 beyond

These modules hold the parameters only: the products run in the engine's plan (mmfm_session_reduce / _expand / _dw, csrc/session_linear.hip).
Parameters are named by session INDEX (eids may contain dots): session_in.{mod}.{k}.weight [n_k, P], .bias [P]; session_out.{mod}.{k}.weight
[n_k, P], .bias [n_k].  Both weights are [n_k, P]: every row has the fixed length P."""
from collections import OrderedDict

import torch
import torch.nn as nn


class StitchConfig:
    """The `stitcher:` section of the model config: width (P; None = encoder.embedder.n_channels), bias, mods."""

    def __init__(self, width, bias=True, mods=("ap",)):
        self.width, self.bias, self.mods = width, bias, tuple(mods)


def read_stitch_config(config):
    """(use_session, StitchConfig or None) of a model config.  Values of the wrong type raise ValueError here, when the config is read."""
    get = config.get if hasattr(config, "get") else lambda k, d=None: getattr(config, k, d)
    use = get("use_session", False)
    if not isinstance(use, bool):
        raise ValueError(f"use_session = {use!r}: true or false")
    sec = get("stitcher", None)
    sget = (lambda k, d: d) if sec is None else (sec.get if hasattr(sec, "get") else lambda k, d=None: getattr(sec, k, d))
    width, bias, mods = sget("width", None), sget("bias", True), sget("mods", ["ap"])
    if width is not None and (isinstance(width, bool) or not isinstance(width, int) or width < 1):
        raise ValueError(f"stitcher.width = {width!r}: an int >= 1")
    if not isinstance(bias, bool):
        raise ValueError(f"stitcher.bias = {bias!r}: true or false")
    if isinstance(mods, str) or not hasattr(mods, "__iter__") or not all(isinstance(m, str) for m in mods) or not list(mods) \
            or len(set(mods)) != len(list(mods)):
        raise ValueError(f"stitcher.mods = {mods!r}: a non-empty list of distinct modality names")
    if not use:
        return False, None
    if width is None:
        width = config["encoder"]["embedder"]["n_channels"]
        if isinstance(width, bool) or not isinstance(width, int) or width < 1:
            raise ValueError(f"encoder.embedder.n_channels = {width!r}: the default stitcher.width must be an int >= 1")
    return True, StitchConfig(int(width), bias, list(mods))


def check_sessions(sessions):
    """An ordered eid -> n_k mapping -> OrderedDict of str -> int; ValueError for anything else."""
    if not hasattr(sessions, "items") or not len(sessions):
        raise ValueError(f"sessions = {sessions!r}: a non-empty ordered mapping eid -> number of neurons")
    out = OrderedDict()
    for eid, n in sessions.items():
        if not isinstance(eid, str) or isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"sessions[{eid!r}] = {n!r}: eids are strings, neuron counts ints >= 1")
        out[eid] = int(n)
    return out


class SessionIn(nn.Module):
    """One session's read-in: the values of nn.Linear(n, P), the weight stored transposed ([n, P])."""

    def __init__(self, n, width, bias=True):
        super().__init__()
        lin = nn.Linear(n, width, bias=bias)
        self.weight = nn.Parameter(lin.weight.detach().t().contiguous())
        self.bias = nn.Parameter(lin.bias.detach().clone()) if bias else None


class SessionOut(nn.Module):
    """One session's read-out: the values of nn.Linear(P, n) ([n, P] as torch stores it)."""

    def __init__(self, n, width, bias=True):
        super().__init__()
        lin = nn.Linear(width, n, bias=bias)
        self.weight = nn.Parameter(lin.weight.detach().clone())
        self.bias = nn.Parameter(lin.bias.detach().clone()) if bias else None


def build_session_layers(mods, sizes, width, bias):
    """(session_in, session_out): per stitched modality the read-in layers in session order, then its read-out layers in session order -
    the order the generator is drawn from."""
    s_in, s_out = nn.ModuleDict(), nn.ModuleDict()
    for mod in mods:
        s_in[mod] = nn.ModuleList([SessionIn(n, width, bias) for n in sizes])
        s_out[mod] = nn.ModuleList([SessionOut(n, width, bias) for n in sizes])
    return s_in, s_out


def session_ids(eid, B, index, sizes, N_max, mod="ap"):
    """The per-sample session indices of a batch: `eid` is one string for the whole batch or a sequence of B strings.  ValueError -
    before any draw or launch - for an unknown eid and for a batch whose padded width N_max is smaller than a present session's n_k."""
    if eid is None or isinstance(eid, (bytes, int, float)) or not (isinstance(eid, str) or hasattr(eid, "__iter__")):
        raise ValueError(f"modality {mod!r}: a stitched modality needs `eid` in its mod_dict entry - one string for the batch or one per sample - got {eid!r}")
    eids = [eid] * B if isinstance(eid, str) else list(eid)
    if len(eids) != B:
        raise ValueError(f"modality {mod!r}: {len(eids)} eids for a batch of {B}")
    sid = []
    for e in eids:
        if not isinstance(e, str) or e not in index:
            raise ValueError(f"modality {mod!r}: unknown session eid {e!r} (known: {', '.join(list(index)[:8])}{', ...' if len(index) > 8 else ''})")
        k = index[e]
        if sizes[k] > N_max:
            raise ValueError(f"modality {mod!r}: session {e!r} has {sizes[k]} neurons, the batch is padded to {N_max}")
        sid.append(k)
    return sid


def session_channel_mask(sid, sizes, N):
    """v[b, c] = c < n_s(b) as uint8 [B, N] (host): the channel mask the loss takes for a stitched modality."""
    n = torch.tensor([sizes[k] for k in sid], dtype=torch.int64)
    return (torch.arange(N)[None, :] < n[:, None]).to(torch.uint8)
