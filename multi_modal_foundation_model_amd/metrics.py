"""Evaluation metrics on the device: drop-ins for the host loops of the reference's eval path.

* `r2_series(gt, pred)`      - what `utils/utils.py:107-115` computes with 50 x B torcheval calls: R^2 of every (g, c) series
                               of a [G, S, C] pair over S, one launch, strided views accepted as they are.
* `trial_avg_r2(gt, pred)`   - `metrics_list(..., metrics=["r2"])["r2"]`: nan/inf-masked mean over c, mean over g.
* `bits_per_spike(rates, spikes)` - `utils/eval_utils.py:1095-1119` (NLB co-smoothing metric).

* `bits_per_spike_per_neuron(rates, spikes)` - the per-neuron loop of `spiking_activity_recon_eval`
                               (`utils/eval_utils.py:846-851`, N host calls upstream) in one pass; inf -> nan like upstream.

* `confusion(pred, target, mask=None)` - the [C, C] count matrix of a categorical modality (row = target class): arg-max of the
                               logits against arg-max of the targets over the masked tokens, one launch (mmfm_argmax_confusion).
* `accuracy(...)`, `balanced_accuracy(...)` - its trace over its sum, and the mean recall of the classes that occur.

There is no CPU path here: tensors must live on the GPU (the CPU restatement is oracle/metrics_oracle.py, test-only).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .ops import P, _stream as stream


def _need_cuda(*ts):
    for t in ts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError("multi_modal_foundation_model_amd.metrics runs on the MI355X; move the tensors to the GPU")


def r2_series(gt: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """gt, pred: [G, S, C] fp32 CUDA tensors (any strides).  Returns [G, C] fp32: 1 - SS_res / SS_tot over S."""
    _need_cuda(gt, pred)
    if gt.shape != pred.shape or gt.dim() != 3:
        raise ValueError(f"r2_series: expected two [G, S, C] tensors, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    gt = gt if gt.dtype == torch.float32 else gt.float()
    pred = pred if pred.dtype == torch.float32 else pred.float()
    G, S, Cn = gt.shape
    out = torch.empty(G, Cn, device=gt.device, dtype=torch.float32)
    gs, ps = (C.c_int64 * 3)(*gt.stride()), (C.c_int64 * 3)(*pred.stride())
    L.check(L.lib().mmfm_r2_series(P(gt), gs, P(pred), ps, G, S, Cn, P(out), stream()), "mmfm_r2_series")
    return out


def trial_avg_r2(gt: torch.Tensor, pred: torch.Tensor) -> float:
    """metrics_list(gt, pred, metrics=["r2"])["r2"] (utils/utils.py:109-115): for every g the invalid-masked mean over the
    c series of R^2 over S, then the mean over g."""
    vals = r2_series(gt, pred).double().cpu().numpy()
    return float(np.mean([np.ma.masked_invalid(v).mean() for v in vals]))


def bits_per_spike(rates, spikes) -> float:
    """utils/eval_utils.py:1095-1119 on the device.  rates, spikes: [..., N] (trials x bins x neurons), same shape."""
    rates, spikes = torch.as_tensor(rates), torch.as_tensor(spikes)
    _need_cuda(rates, spikes)
    if rates.shape != spikes.shape:
        raise AssertionError(f"neg_log_likelihood: Rates and spikes should be of the same shape. spikes: {tuple(spikes.shape)}, "
                             f"rates: {tuple(rates.shape)}")
    N = rates.shape[-1]
    r = rates.reshape(-1, N).float().contiguous()
    s = spikes.reshape(-1, N).float().contiguous()
    R = r.shape[0]
    ws = torch.empty(L.lib().mmfm_bits_per_spike_workspace(R, N), dtype=torch.uint8, device=r.device)
    out = torch.empty(4, device=r.device, dtype=torch.float32)
    L.check(L.lib().mmfm_bits_per_spike(P(r), P(s), R, N, P(out), P(ws), ws.numel(), stream()), "mmfm_bits_per_spike")
    return float(out[0].item())


def bits_per_spike_per_neuron(rates, spikes) -> torch.Tensor:
    """[..., N] rates / spikes -> [N] fp32 (on the device): bits_per_spike(rates[..., [n]], spikes[..., [n]]) for every n,
    with upstream's `if np.isinf(bps): bps = np.nan` applied (utils/eval_utils.py:846-851)."""
    rates, spikes = torch.as_tensor(rates), torch.as_tensor(spikes)
    _need_cuda(rates, spikes)
    if rates.shape != spikes.shape:
        raise AssertionError("neg_log_likelihood: Rates and spikes should be of the same shape.")
    N = rates.shape[-1]
    r = rates.reshape(-1, N).float().contiguous()
    s = spikes.reshape(-1, N).float().contiguous()
    R = r.shape[0]
    ws = torch.empty(L.lib().mmfm_bits_per_spike_neurons_workspace(R, N), dtype=torch.uint8, device=r.device)
    out = torch.empty(N, device=r.device, dtype=torch.float32)
    L.check(L.lib().mmfm_bits_per_spike_neurons(P(r), P(s), R, N, P(out), P(ws), ws.numel(), stream()), "mmfm_bits_per_spike_neurons")
    return torch.where(torch.isinf(out), torch.full_like(out, float("nan")), out)


def confusion(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
    """pred [..., C] logits (fp32 or bf16), target [..., C] (one-hot labels or class probabilities), mask [...] or None (every
    token): int64 [C, C] on the device, conf[i, j] = masked tokens whose target arg-max is i and whose predicted arg-max is j.  The
    lowest index wins a tie on either side."""
    _need_cuda(pred, target)
    if pred.shape != target.shape or pred.dim() < 1:
        raise ValueError(f"confusion: pred {tuple(pred.shape)} and target {tuple(target.shape)} must have one shape [..., C]")
    Cn = pred.shape[-1]
    p = pred if pred.dtype in (torch.float32, torch.bfloat16) else pred.float()
    p, t = p.reshape(-1, Cn).contiguous(), target.reshape(-1, Cn).float().contiguous()
    R = p.shape[0]
    conf = torch.empty(Cn, Cn, dtype=torch.int64, device=p.device)
    if R == 0:
        return conf.zero_()
    m = None
    if mask is not None:
        _need_cuda(mask)
        if tuple(mask.shape) != tuple(pred.shape[:-1]):
            raise ValueError(f"confusion: mask {tuple(mask.shape)} must be pred's shape without the class axis {tuple(pred.shape[:-1])}")
        m = (mask.reshape(-1) != 0).to(torch.uint8).contiguous()
    dtype = L.F32 if p.dtype == torch.float32 else L.BF16
    L.check(L.lib().mmfm_argmax_confusion(dtype, P(p), P(t), P(m), 1, 1, R, Cn, P(conf), stream()), "mmfm_argmax_confusion")
    return conf


def accuracy(pred, target, mask=None) -> float:
    """Correct over counted tokens (NaN when nothing is counted)."""
    conf = confusion(pred, target, mask).double()
    return float((conf.diagonal().sum() / conf.sum()).item())


def balanced_accuracy(pred, target, mask=None) -> float:
    """The mean over the classes that occur among the targets of their recall (sklearn's balanced_accuracy_score); NaN when none does."""
    conf = confusion(pred, target, mask).double()
    support = conf.sum(1)
    seen = support > 0
    return float((conf.diagonal()[seen] / support[seen]).mean().item())
