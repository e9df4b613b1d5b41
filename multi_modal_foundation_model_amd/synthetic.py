"""Synthetic batches with the reference loader's batch contract (loader/base.py:436-450,
make_loader.py:4-53): the HuggingFace datasets the reference trains on are not reachable offline.

Recipe: host generator seeded 1000*rank + step; spikes ~ Poisson(0.3) counts,
behaviour ~ N(0,1), attention masks all ones (or right-padded), time stamps arange(T).
"""
from __future__ import annotations

from typing import List, Optional

import torch


def synth_batch(B, T, n_ap, n_beh, seed, pad: Optional[List[int]] = None, eid="synthetic", full_contract=True):
    g = torch.Generator().manual_seed(seed)
    spikes = torch.poisson(torch.full((B, T, n_ap), 0.3), generator=g)
    beh = torch.randn(B, T, n_beh, generator=g)
    attn = torch.ones(B, T, dtype=torch.int64)
    if pad is not None:
        for b, nb in enumerate(pad):
            if nb:
                attn[b, T - nb:] = 0
    batch = dict(spikes_data=spikes, target=beh, time_attn_mask=attn,
                 spikes_timestamps=torch.arange(T, dtype=torch.int64)[None].repeat(B, 1))
    if full_contract:
        batch.update(space_attn_mask=torch.ones(B, n_ap, dtype=torch.int64),
                     spikes_spacestamps=torch.arange(n_ap, dtype=torch.int64)[None].repeat(B, 1),
                     neuron_depths=torch.zeros(B, n_ap), neuron_regions=[["XX"] * B for _ in range(n_ap)],
                     eid=[eid] * B, choice=torch.zeros(B), block=torch.zeros(B), reward=torch.zeros(B))
    return batch


class SyntheticLoader:
    """Iterable of `n_batches` synthetic batches; deterministic per (rank, step)."""

    def __init__(self, n_batches, batch_size, T=100, n_ap=668, n_beh=2, rank=0, seed0=0, device=None, cache=False):
        self.n, self.B, self.T, self.n_ap, self.n_beh = n_batches, batch_size, T, n_ap, n_beh
        self.rank, self.seed0, self.device = rank, seed0, device
        self._cache = {} if cache else None

    def __len__(self):
        return self.n

    def _make(self, step):
        b = synth_batch(self.B, self.T, self.n_ap, self.n_beh, seed=1000 * self.rank + self.seed0 + step)
        if self.device is not None:
            b = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
        return b

    def __iter__(self):
        for step in range(self.n):
            if self._cache is None:
                yield self._make(step)
            else:
                if step not in self._cache:
                    self._cache[step] = self._make(step)
                yield dict(self._cache[step])


def session_sizes(n_sessions, n_ap, seed=2024):
    """n_k, the neurons of session k: drawn once from numpy's default_rng(seed).integers(300, n_ap + 1), one draw per session in order."""
    import numpy as np
    if n_ap < 300:
        raise ValueError(f"multi-session batches draw 300..n_ap neurons per session: n_ap = {n_ap} < 300")
    rng = np.random.default_rng(seed)
    return [int(rng.integers(300, n_ap + 1)) for _ in range(n_sessions)]


class MultiSessionLoader(SyntheticLoader):
    """Synthetic multi-session pretraining batches as the reference loader pads them (loader/base.py:399-425): batch i belongs to
    session i % n_sessions, session k has n_k of the n_ap channels (`session_sizes`), the others are right-padded with pad_value = -1
    and cleared in space_attn_mask; eid names the session.  The values of the real channels are synth_batch's own.
    world > 1 (data parallelism): batch i of rank r belongs to session (i * world + r) % n_sessions, so that the ranks of one step hold
    different sessions; world = 1 is the sequence above, whatever the rank."""

    def __init__(self, n_batches, batch_size, T=100, n_ap=668, n_beh=2, n_sessions=2, rank=0, seed0=0, device=None, cache=False, world=1):
        super().__init__(n_batches, batch_size, T, n_ap, n_beh, rank=rank, seed0=seed0, device=device, cache=cache)
        if n_sessions < 1:
            raise ValueError(f"n_sessions must be >= 1, got {n_sessions}")
        if world < 1 or (world > 1 and not 0 <= rank < world):
            raise ValueError(f"world must be >= 1 and, beyond 1, rank in [0, world): got world {world}, rank {rank}")
        self.n_sessions, self.sizes, self.world = n_sessions, session_sizes(n_sessions, n_ap), world

    def session_of(self, step):
        """The session of batch `step` of this rank."""
        return (step * self.world + self.rank) % self.n_sessions if self.world > 1 else step % self.n_sessions

    def _make(self, step):
        k = self.session_of(step)
        b = synth_batch(self.B, self.T, self.n_ap, self.n_beh, seed=1000 * self.rank + self.seed0 + step, eid=f"session{k}")
        b["spikes_data"][:, :, self.sizes[k]:] = -1.0
        b["space_attn_mask"][:, self.sizes[k]:] = 0
        if self.device is not None:
            b = {key: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for key, v in b.items()}
        return b
