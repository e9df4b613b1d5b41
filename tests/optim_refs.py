"""fp64 restatement of the range-table optimiser (include/mmfm.h, MMFM_OPTIM_RANGES; multi_modal_foundation_model_amd/optim.py):
the chunk table, the per-range update with its hyper row, per-parameter step counts, the fused clip and the non-finite skip.

tests/test_optim_ranges_cpu.py proves it against torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ in fp64; the GPU tests compare the
kernels and FusedAdamW with it.  The single-range update itself is edge_refs.adamw_step (already proven against torch there)."""
import math

import torch

import edge_refs as E

CHUNK = 4096                  # MMFM_OPTIM_CHUNK
U64 = 2.0 ** -53              # unit roundoff of fp64


def build_chunks(ranges, chunk=CHUNK):
    """ranges: [(start, end, hyper_row)], sorted and disjoint.  Each is cut at the multiples of `chunk` counted from element 0.
    Returns ([(start, len, range, hyper_row)], first_chunk[n_ranges + 1])."""
    chunks, first = [], []
    for r, (s, e, row) in enumerate(ranges):
        first.append(len(chunks))
        for k in range(s // chunk, (e - 1) // chunk + 1):
            lo, hi = max(s, k * chunk), min(e, (k + 1) * chunk)
            chunks.append((lo, hi - lo, r, row))
    first.append(len(chunks))
    return chunks, first


def clip_coef(total_sumsq, max_norm):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2): min(1, max_norm / (norm + 1e-6)); max_norm <= 0 or inf: 1."""
    if max_norm is None or not (max_norm > 0) or math.isinf(max_norm):
        return 1.0
    return min(1.0, max_norm / (math.sqrt(total_sumsq) + 1e-6))


def sumsq_bound(n_terms):
    """Relative error bound of ANY summation order of n non-negative fp64 terms: (n - 1) 2^-53 (to first order; the squares of fp32
    values are exact in fp64, so the terms carry no error of their own)."""
    return max(n_terms - 1, 1) * U64


def range_step(P, G, M, V, ranges, hyper, clip=1.0):
    """One mmfm_adamw_step_ranges on fp64 state tensors (in place): range r is updated by edge_refs.adamw_step with row hyper[row] on
    the gradient G * clip; nothing outside the ranges is touched."""
    for s, e, row in ranges:
        E.adamw_step(P[s:e], E.f64(G[s:e]) * clip, M[s:e], V[s:e], torch.as_tensor(hyper[row], dtype=torch.float64))


class RangeAdamW:
    """FusedAdamW's host logic on fp64 tensors: `params` is {name: fp64 tensor} (updated in place), `groups` a list of dicts with
    "names", lr, betas, eps, weight_decay.  step(grads) takes {name: gradient or None}; None skips the parameter, which keeps its own
    step count, as torch's.  With skip_nonfinite a step whose norm is inf / NaN changes no tensor but the counts still advance."""

    def __init__(self, params, groups, max_grad_norm=None, skip_nonfinite=False, grad_scale=1.0):
        self.params, self.groups = params, groups
        self.max_grad_norm, self.skip_nonfinite, self.grad_scale = max_grad_norm, skip_nonfinite, grad_scale
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}
        self.steps = {k: 0 for k in params}
        self.skipped = 0
        self.last_total = self.last_coef = None

    def step(self, grads):
        live = [(gi, k) for gi, g in enumerate(self.groups) for k in g["names"] if grads.get(k) is not None]
        if not live:
            return
        clip = 1.0
        if self.max_grad_norm is not None or self.skip_nonfinite:
            total = sum(float((E.f64(grads[k]) * self.grad_scale).pow(2).sum()) for _, k in live)
            self.last_total, self.last_coef = total, clip_coef(total, self.max_grad_norm)
            clip = self.last_coef
            if self.skip_nonfinite and not math.isfinite(total):
                self.skipped += 1
                for _, k in live:
                    self.steps[k] += 1
                return
        for gi, k in live:
            g = self.groups[gi]
            self.steps[k] += 1
            h = E.adamw_hyper(self.steps[k], g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale)
            E.adamw_step(self.params[k].view(-1), E.f64(grads[k]).reshape(-1) * clip, self.m[k].view(-1), self.v[k].view(-1),
                         torch.tensor(h, dtype=torch.float64))
