"""Losses for `MultiModal.loss_mod` beyond torch's elementwise modules.

`SoftmaxCrossEntropy` is the loss of a categorical modality (an animal's `choice`, the `block` prior, a reward flag): one classifier
over the C channels of the head instead of the C independent detectors `BCEWithLogitsLoss` on a one-hot target trains.

Upstream evaluates `(loss_mod[mod](preds, targets) * targets_mask[B,T,N]).sum()` and `n = targets_mask.sum()` (mm.py:217-239), so an
entry must return a [B, T, N] tensor.  `nn.CrossEntropyLoss` does not fit that contract - it reads dim 1 as the class axis and returns
[B, T] - and stays refused by `MultiModal`.  This module returns the [..., C] tensor

    e[c] = - w[c] t'[c] log_softmax(p)[c],        t'[c] = (1 - eps) t[c] + eps / C

whose sum over c is `F.cross_entropy(p, t, weight=w, label_smoothing=eps, reduction='none')` for index (one-hot) and probability
targets alike.  Its `forward` is plain torch: dropped into upstream's `loss_mod` the same object computes upstream what the HIP engine
computes here (mmfm_softmax_ce_fwd / _bwd; `MultiModal` reads the weights and the smoothing off the module and never calls it).
"""
from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F


class SoftmaxCrossEntropy(nn.Module):
    """weight: one non-negative weight per class (None: 1), label_smoothing in [0, 1].  Targets are [..., C] like the predictions:
    one-hot labels (`one_hot_labels`) or any non-negative weights."""

    def __init__(self, weight: Optional[Sequence[float]] = None, label_smoothing: float = 0.0):
        super().__init__()
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"SoftmaxCrossEntropy: label_smoothing {label_smoothing} outside [0, 1]")
        w = None if weight is None else torch.as_tensor(weight, dtype=torch.float32).reshape(-1).clone()
        if w is not None and (w.numel() == 0 or not bool((w >= 0).all())):
            raise ValueError("SoftmaxCrossEntropy: weight must hold one non-negative number per class")
        self.register_buffer("weight", w)
        self.label_smoothing = float(label_smoothing)

    def forward(self, preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        C = preds.shape[-1]
        if self.weight is not None and self.weight.numel() != C:
            raise ValueError(f"SoftmaxCrossEntropy: {self.weight.numel()} class weights for {C} classes")
        t = (1.0 - self.label_smoothing) * targets.to(preds.dtype) + self.label_smoothing / C
        if self.weight is not None:
            t = self.weight.to(device=preds.device, dtype=preds.dtype) * t
        return -t * F.log_softmax(preds, dim=-1)

    def extra_repr(self) -> str:
        return f"weight={None if self.weight is None else self.weight.tolist()}, label_smoothing={self.label_smoothing}"


def one_hot_labels(labels: torch.Tensor, C: int) -> torch.Tensor:
    """[B, T] int64 class indices -> [B, T, C] fp32 one-hot: a categorical modality's inputs and targets."""
    if labels.dtype != torch.int64:
        raise TypeError(f"one_hot_labels: int64 class indices expected, got {labels.dtype}")
    return F.one_hot(labels, int(C)).to(torch.float32)
