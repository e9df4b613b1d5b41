"""Plain-torch restatement of the per-session read-in / read-out layers (use_session) and the fp64 references of their kernels.

Semantics (include/mmfm.h, MMFM_SESSION_LINEAR): session k has n_k real channels in columns [0, n_k) of the padded [B, T, N_max]
tensor; s(b) is the session of sample b.
    read-in    u[b, t, :]    = sum_{c < n_s(b)} x[b, t, c] Win_s(b)[c, :] + bin_s(b)
    read-out   pred[b, t, c] = sum_p f[b, t, p] Wout_s(b)[c, p] + bout_s(b)[c]   for c < n_s(b), exactly 0 beyond
Both weights are stored [n_k, P].  Everything here works sample by sample with the weights of the sample's session - `read_in` /
`read_out` through nn.functional.linear, so torch autograd gives the gradients (tests/test_session_stitch_cpu.py checks the
closed forms below against it in fp64) - and never reads a column >= n_s(b).

The *_ref functions return, beside the value, what the derived bounds of tests/edge_refs.py need: sum|terms| per element and the
number of fp32 roundings of the kernel's sum (bound_n)."""
import numpy as np
import torch
import torch.nn.functional as F

MIXES = ("one", "interleaved", "absent", "distinct")
# (B, T, P, N_max, sizes): the sizes are the first sessions' neuron counts; further sessions (the `distinct` mix needs B of them) cycle them
SHAPES = [(5, 7, 24, 12, (12, 7, 1)), (6, 33, 72, 150, (150, 129, 64, 1)), (3, 100, 40, 70, (70, 33)), (2, 1, 3, 5, (5, 2))]


def f64(t):
    return t.to(torch.float64)


def session_sizes(B, sizes):
    """The neuron counts of S = max(len(sizes), B) sessions: `sizes`, then cycled."""
    return [sizes[k % len(sizes)] for k in range(max(len(sizes), B))]


def mix(name, B, n_base):
    """Per-sample session indices of a named mix over the first n_base sessions (distinct: over B sessions)."""
    if name == "one":
        return [1 % n_base] * B                              # a session smaller than N_max where there is one
    if name == "interleaved":
        return [b % n_base for b in range(B)]
    if name == "absent":
        return [b % (n_base - 1) for b in range(B)]          # the last base session has no sample
    if name == "distinct":
        return list(range(B))[::-1]
    raise KeyError(name)


def layout(sizes, P, bias_is_n, gap=8):
    """Element offsets of the sessions' [n_k, P] matrices and of their biases ([n_k] if bias_is_n else [P]) in two flat buffers, each
    slot on a multiple of `gap` with at least one unused element behind it.  Returns (w_off, b_off, w_elems, b_elems)."""
    w_off, b_off, w, b = [], [], 0, 0
    for n in sizes:
        w_off.append(w)
        b_off.append(b)
        w = (w + n * P + gap) // gap * gap
        b = (b + (n if bias_is_n else P) + gap) // gap * gap
    return w_off, b_off, w, b


def spans(sizes, off, length):
    """Boolean numpy mask per session over a flat buffer of `length` elements: True on the session's span."""
    out = []
    for n, o in zip(sizes, off):
        m = np.zeros(length, dtype=bool)
        m[o:o + n] = True
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------- the layers, sample by sample
def read_in(x, sid, sizes, Win, bin_):
    """x [B, T, N_max] -> u [B, T, P]; Win[k] [n_k, P] (an nn.Linear(n_k, P) weight, transposed), bin_[k] [P] or None."""
    return torch.stack([F.linear(x[b, :, :sizes[k]], Win[k].t(), None if bin_ is None else bin_[k]) for b, k in enumerate(sid)])


def read_out(f, sid, sizes, Wout, bout, N_max):
    """f [B, T, P] -> pred [B, T, N_max]; Wout[k] [n_k, P] (an nn.Linear(P, n_k) weight), bout[k] [n_k] or None."""
    rows = []
    for b, k in enumerate(sid):
        y = F.linear(f[b], Wout[k], None if bout is None else bout[k])
        rows.append(F.pad(y, (0, N_max - sizes[k])))
    return torch.stack(rows)


def channel_mask(sid, sizes, N_max, device=None):
    """v[b, c] = c < n_s(b), uint8 [B, N_max]: the channel mask the loss takes for a stitched modality."""
    n = torch.tensor([sizes[k] for k in sid], device=device)
    return (torch.arange(N_max, device=device)[None, :] < n[:, None]).to(torch.uint8)


# ------------------------------------------------------------------------------------------------- fp64 references of the kernels
def reduce_ref(x, sid, sizes, W, bias):
    """mmfm_session_reduce: (y, sum_abs, bound_n), y [B, T, P] fp64.  bound_n: n_s FMAs and the bias addition, one more for the
    second-order terms of the product of (1 + u) factors (it covers them as long as n_s < 4000)."""
    ys, sa, nn = [], [], []
    for b, k in enumerate(sid):
        xb, w = f64(x[b, :, :sizes[k]]), f64(W[k])
        y, a = xb @ w, xb.abs() @ w.abs()
        if bias is not None:
            y, a = y + f64(bias[k]), a + f64(bias[k]).abs()
        ys.append(y)
        sa.append(a)
        nn.append(torch.full_like(y, sizes[k] + 2))
    return torch.stack(ys), torch.stack(sa), torch.stack(nn)


def expand_ref(f, sid, sizes, W, bias, N_max):
    """mmfm_session_expand: (y, sum_abs, bound_n), y [B, T, N_max] fp64 with zeros beyond n_s; the sums run over P."""
    P = f.shape[-1]
    ys, sa = [], []
    for b, k in enumerate(sid):
        fb, w = f64(f[b]), f64(W[k])
        y, a = fb @ w.t(), fb.abs() @ w.abs().t()
        if bias is not None:
            y, a = y + f64(bias[k]), a + f64(bias[k]).abs()
        ys.append(F.pad(y, (0, N_max - sizes[k])))
        sa.append(F.pad(a, (0, N_max - sizes[k])))
    y = torch.stack(ys)
    return y, torch.stack(sa), torch.full_like(y, P + 2)


def dw_ref(a, q, sid, sizes):
    """mmfm_session_dw: per present session k a dict dW [n_k, P], db_q [P] (read-in bias gradient), db_a [n_k] (read-out), the sums of
    absolute terms abs_* and bound_n = the number of summed rows + the number of samples + 1 (one rounding per row, one per slab of the
    second level - never more slabs than samples - and one for the second-order terms)."""
    out = {}
    for k in sorted(set(sid)):
        rows = [b for b, s in enumerate(sid) if s == k]
        A = f64(torch.cat([a[b, :, :sizes[k]] for b in rows]))
        Q = f64(torch.cat([q[b] for b in rows]))
        out[k] = dict(dW=A.t() @ Q, abs_W=A.abs().t() @ Q.abs(), db_q=Q.sum(0), abs_q=Q.abs().sum(0), db_a=A.sum(0), abs_a=A.abs().sum(0),
                      bound_n=A.shape[0] + len(rows) + 1)
    return out


# ------------------------------------------------------------------------------------------------- argument refusals (no HIP call)
FAKE = 0x10000           # a non-NULL "device pointer": the checks return before anything dereferences or launches
BAD_DESC = {
    "unknown dtype": (dict(dtype=2), "dtype"),
    "B = 0": (dict(B=0), ">= 1"),
    "T = 0": (dict(T=0), ">= 1"),
    "P = 0": (dict(P=0), ">= 1"),
    "N_max = 0": (dict(N_max=0), ">= 1"),
    "S = 0": (dict(S=0), ">= 1"),
    "B beyond the grid": (dict(B=65536), "grid"),
    "ld_pad < N_max": (dict(ld_pad=11), "ld_pad"),
    "ld_p < P": (dict(ld_p=7), "ld_p"),
    "NULL sid": (dict(sid=None), "session table"),
    "NULL n": (dict(n=None), "session table"),
    "NULL w_off": (dict(w_off=None), "session table"),
    "w_elems = 0": (dict(w_elems=0), "w_elems"),
}
BAD_FWD = {
    "NULL weights": (dict(w=None), "weights"),
    "bias without b_off": (dict(b_off=None), "bias"),
    "bias without b_elems": (dict(b_elems=0), "bias"),
}


def fake_desc(L, **kw):
    d = L.SessionDesc()
    base = dict(dtype=L.BF16, B=4, T=8, P=8, N_max=12, S=3, ld_pad=12, ld_p=8, sid=FAKE, n=FAKE, w_off=FAKE, b_off=FAKE, w=FAKE, w_elems=1000,
                bias=FAKE, b_elems=100)
    for k, v in dict(base, **kw).items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------- the stitched model on the fp64 oracle
def oracle_forward(sd, md, cfg, sid, sizes, mods=("ap",), training=True, dropout_fn=None):
    """The model with per-session layers on oracle.mm_oracle (plain torch, any dtype): `read_in` in front of the stitched modalities'
    tokenisers, the oracle's forward at the shared width P, `read_out` behind their heads, and the loss with v[b, c] = c < n_s(b) as one
    more factor of the mask.  sd: the model's state dict (session_in.* / session_out.* beside the oracle's keys); md: the mod dict with
    eval_mask set.  Returns loss, mod_loss, mod_n_examples, mod_preds like the oracle."""
    from oracle import mm_oracle as O
    trunk = {k: v for k, v in sd.items() if not k.startswith("session_")}
    md2, pads = {m: dict(d) for m, d in md.items()}, {}
    for mod in mods:
        d = md2[mod]
        S = len(sizes)
        Win = [sd[f"session_in.{mod}.{k}.weight"] for k in range(S)]
        bin_ = [sd[f"session_in.{mod}.{k}.bias"] for k in range(S)] if f"session_in.{mod}.0.bias" in sd else None
        pads[mod] = (d["inputs"].shape[-1], d["targets"])
        d["inputs"] = read_in(d["inputs"], sid, sizes, Win, bin_)
        d["targets"] = torch.zeros_like(d["inputs"])          # (the oracle's own loss of this modality is not used)
    out = O.forward(trunk, md2, cfg, training=training, dropout_fn=dropout_fn)
    mod_loss, mod_n, preds = dict(out["mod_loss"]), dict(out["mod_n_examples"]), dict(out["mod_preds"])
    for mod in mods:
        N, tg = pads[mod]
        S = len(sizes)
        Wout = [sd[f"session_out.{mod}.{k}.weight"] for k in range(S)]
        bout = [sd[f"session_out.{mod}.{k}.bias"] for k in range(S)] if f"session_out.{mod}.0.bias" in sd else None
        pr = read_out(out["mod_preds"][mod], sid, sizes, Wout, bout, N)
        v = channel_mask(sid, sizes, N, device=pr.device).to(pr.dtype)
        w = out["masks"][mod].to(pr.dtype)[:, :, None] * v[:, None, :]
        el = torch.exp(pr) - tg * pr if mod == "ap" else (pr - tg) ** 2
        mod_loss[mod], mod_n[mod], preds[mod] = (el * w).sum(), w.sum(), pr
    return dict(loss=sum(mod_loss.values()) / sum(mod_n.values()), mod_loss=mod_loss, mod_n_examples=mod_n, mod_preds=preds, masks=out["masks"])


# ------------------------------------------------------------------------------------------------- the golden cases (tests/golden/session_stitch_*)
TINY = dict(B=4, T=8, N_max=12, P=8, n_beh=2, max_F=8)
SESSIONS = {"ses.12": 12, "ses.7": 7, "ses.1": 1}          # eid -> neurons (eids with dots: parameters are named by index)
MODEL_SEED, DATA_SEED, MASKER_SEED, PAD = 7, 3, 11, -1.0
OBJECTIVES = ("encoding", "decoding", "token_masking")
EIDS = list(SESSIONS)
# case -> (eid of every sample, objective, stitcher.bias, permutation of the batch's samples or None)
CASES = {f"single{n}/{obj}": ([e] * TINY["B"], obj, True, None) for e, n in SESSIONS.items() for obj in OBJECTIVES}
CASES.update({
    "mixed": ([EIDS[1], EIDS[0], EIDS[0], EIDS[2]], "token_masking", True, None),
    "mixed_perm": ([EIDS[0], EIDS[1], EIDS[2], EIDS[0]], "token_masking", True, [1, 0, 3, 2]),      # the same samples, another sample 0
    "absent": ([EIDS[0], EIDS[1], EIDS[1], EIDS[0]], "token_masking", True, None),
    "nobias": ([EIDS[1], EIDS[0], EIDS[0], EIDS[2]], "token_masking", False, None),
})
FULL_GRAD = ("mixed", "nobias")                              # cases that store every gradient tensor (the others: norms, and the session layers')
CURVE_STEPS, ACCUM, ACCUM_STEPS = 50, 3, 17


def pad_batch(spikes, eids, pad=PAD):
    """The padded batch of the samples' sessions: columns >= n_s(b) of sample b hold `pad`."""
    out = spikes.clone()
    for b, e in enumerate(eids):
        out[b, :, SESSIONS[e]:] = pad
    return out


def case_batch(batch, case, pad=PAD):
    """The tiny batch (a dict of tensors, oracle.mm_oracle.synth_batch's keys) as case `case` sees it: permuted, then padded."""
    eids, _, _, perm = CASES[case]
    if perm is not None:
        batch = {k: v[perm] for k, v in batch.items()}
    batch = dict(batch)
    batch["spikes_data"] = pad_batch(batch["spikes_data"], eids, pad)
    return batch


class RefLayers(torch.nn.Module):
    """The session layers beside a reference model, with the names and the initial values of the model's own: per stitched modality
    nn.Linear(n_k, P) in session order (weight stored transposed), then nn.Linear(P, n_k) in session order."""

    def __init__(self, sizes, width, bias=True, mod="ap"):
        super().__init__()
        lin_in = [torch.nn.Linear(n, width, bias=bias) for n in sizes]
        lin_out = [torch.nn.Linear(width, n, bias=bias) for n in sizes]
        mk = lambda lins, tr: torch.nn.ModuleDict({mod: torch.nn.ModuleList([_Holder(l, tr) for l in lins])})
        self.session_in, self.session_out = mk(lin_in, True), mk(lin_out, False)

    def tensors(self, which, mod="ap"):
        layers = getattr(self, "session_" + which)[mod]
        return [l.weight for l in layers], ([l.bias for l in layers] if layers[0].bias is not None else None)


class _Holder(torch.nn.Module):
    def __init__(self, lin, transpose):
        super().__init__()
        self.weight = torch.nn.Parameter(lin.weight.detach().t().contiguous() if transpose else lin.weight.detach().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().clone()) if lin.bias is not None else None


# further cases on ragged-format batches (tests/mod_segments.py): modality segments T = (8, 5), and input masking in two modes
XEIDS = [EIDS[1], EIDS[0], EIDS[0], EIDS[2]]
XCASES = {"seg": dict(T=(8, 5)), "im_temporal": dict(mode="temporal"), "im_neuron": dict(mode="neuron")}


def xcase_batch(case, pad=PAD):
    import mod_segments as S
    batch = S.ragged_batch(TINY["B"], XCASES[case].get("T", (TINY["T"], TINY["T"])), TINY["N_max"], TINY["n_beh"], DATA_SEED, max_F=TINY["max_F"])
    batch["ap"]["inputs"] = pad_batch(batch["ap"]["inputs"], XEIDS, pad)
    return batch


def xcase_mod_dict(case, batch):
    """The mod_dict of an XCASES batch: token masking, or the trainer's masking_mode on every modality (input masking)."""
    import input_masking as IM
    import mod_segments as S
    mode = XCASES[case].get("mode")
    md = IM.make_mod_dict(batch, mode) if mode else S.make_mod_dict(batch, "token_masking")
    md["ap"]["eid"] = list(XEIDS)
    return md
