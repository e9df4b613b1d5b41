"""Random mask generator (reference: models/masker.py:56-174).

Host-side by design: the reference draws from torch's CPU generator (and Python's `random` for
region sampling), and the masked-pretraining path keeps only `mask[:, :, 0]` (mm.py:267-270), so
moving this to the GPU would change the random stream for no gain.  The order and shapes of the
generator calls below are what makes the masks bit-exact against the reference
(tests/golden/masker_bits.npz): bernoulli(expand_prob) [, randint], bernoulli(mask_probs),
bernoulli(zero_ratio x shape), bernoulli(random_ratio x shape), rand(shape) — all on the CPU
generator, wherever `spikes` lives.  Where the values of the three [B, T, N] draws are read (zero_ratio < 1) and
`spikes` is an fp32 CUDA tensor, the same generator outputs are produced on the device instead (`_device_corrupt`,
csrc/mt_device.hip) and the CPU generator jumps past them: the stream and the bits stay the reference's.
"""
import os
import random

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

TOKEN_MODES = ("temporal", "random_token", "causal")


class _PinnedRing:
    """Asynchronous host->device copies of small tensors.  `t.to(device)` from pageable memory is a synchronous
    copy that drains the stream (a ~5 ms stall per call once the GPU runs ahead); staging through pinned
    buffers makes it truly asynchronous.  A slot is reused only after the copy that last read it completed."""

    def __init__(self, slots=8):
        self.slots, self.i, self.bufs, self.events = slots, 0, {}, {}

    def to(self, t, device):
        device = torch.device(device)
        if device.type != "cuda" or t.is_cuda:
            return t.to(device)
        key = (tuple(t.shape), t.dtype)
        if key not in self.bufs:
            self.bufs[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(self.slots)]
            self.events[key] = [None] * self.slots
        self.i = (self.i + 1) % self.slots
        ev = self.events[key][self.i]
        if ev is not None:
            ev.synchronize()
        buf = self.bufs[key][self.i]
        buf.copy_(t)
        out = buf.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[key][self.i] = ev
        return out


class Masker(nn.Module):

    def __init__(self, config):
        super().__init__()
        self.force_active = config.force_active if "force_active" in config else False
        self.mode = config.mode
        self.ratio = config.ratio
        self.zero_ratio = config.zero_ratio
        self.random_ratio = config.random_ratio
        self.expand_prob = config.expand_prob
        self.max_timespan = config.max_timespan
        self.channels = config.channels
        self.timesteps = config.timesteps
        self.mask_regions = config.mask_regions
        self.target_regions = config.target_regions
        self.n_mask_regions = config.n_mask_regions
        self.causal_zero = config.causal_zero
        # Throughput switch of ONE training run, set by the trainer (trainer/base.py: it IS the trainer's default for
        # mask_type 'embd'; `training.exact_masker_stream: true` / MMFM_EXACT_MASKER=1 keeps it off): in the `embd` masking
        # path the caller discards the corrupted spikes, so only the token-level draw matters.  Skipping the three full-size
        # draws shortens the walk through the CPU generator: masks stay identically distributed but, from the second masker
        # call on, are NOT the reference's bit for bit.  It is honoured only by callers that discard the spikes (they pass it
        # per call, mm.py) and it is never pickled: a checkpoint always starts on the reference's stream.
        self.token_mask_only = False
        self._ring = _PinnedRing()
        self._mt_ws = {}                       # (device, ops.mt_plan of the call) -> workspace of the device-side draws
        self.device_draws = 0                  # masker calls whose [B, T, N] draws were generated on the device

    def __getstate__(self):                    # checkpoints pickle the whole model: drop pinned buffers / events
        state = self.__dict__.copy()
        state["_ring"] = None
        state["_mt_ws"] = {}
        state["device_draws"] = 0
        state["token_mask_only"] = False       # a run's throughput switch must not leak into model_best.pt / model_last.pt
        return state

    @staticmethod
    def _no_mask(spikes):
        return spikes, torch.zeros_like(spikes).to(torch.int64)

    # ---- the [B, T, N] draws whose values are read, generated on the device (csrc/mt_device.hip) bit for bit as the CPU generator hands
    # them out; the generator itself moves on by jump-ahead.  MMFM_MASKER_DEVICE=0 (or MMFM_MASKER_JUMP=0) keeps the host draws; so does
    # anything but a contiguous fp32 CUDA tensor below 2^31 elements, and a generator blob rngjump does not know.
    @staticmethod
    def _device_position(spikes):
        if not (spikes.is_cuda and spikes.dtype == torch.float32 and spikes.is_contiguous() and 0 < spikes.numel() < 2 ** 31):
            return None
        if os.environ.get("MMFM_MASKER_JUMP", "1") == "0" or os.environ.get("MMFM_MASKER_DEVICE", "1") == "0":
            return None
        from multi_modal_foundation_model_amd.rngjump import cpu_generator_position
        return cpu_generator_position()

    def _device_ws(self, n, dev):
        from multi_modal_foundation_model_amd import ops
        ws = getattr(self, "_mt_ws", None)
        if ws is None:
            ws = self._mt_ws = {}
        key = (dev, ops.mt_plan(n))
        if key not in ws:
            ws[key] = ops.mt_workspace(n, device=dev)
        return ws[key]

    def _device_bernoulli(self, spikes, p):
        """torch.bernoulli(torch.full(spikes.shape, p)) as a uint8 tensor on spikes.device, or None (take it on the host)."""
        p = float(p)
        pos = self._device_position(spikes) if 0.0 <= p <= 1.0 else None
        if pos is None:
            return None
        from multi_modal_foundation_model_amd import ops
        from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
        n = spikes.numel()
        out = ops.mt_bernoulli(pos[0], pos[1], n, p, device=spikes.device, ws=self._device_ws(n, spikes.device))
        advance_cpu_generator(n)
        self.device_draws = getattr(self, "device_draws", 0) + 1
        return out.view(spikes.shape)

    def _device_corrupt(self, spikes, cm8, out):
        """The zero / random corruption of `spikes` under the device mask cm8 (uint8, broadcast dimensions of size 1 or stride 0) into `out`
        (`spikes` itself: in place), the three draws taken from the generator's position and the generator moved past them.  None: the host
        lines run."""
        zr, rr = float(self.zero_ratio), float(self.random_ratio)
        pos = self._device_position(spikes) if (0.0 <= zr <= 1.0 and 0.0 <= rr <= 1.0) else None
        if pos is None:
            return None
        from multi_modal_foundation_model_amd import ops
        from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
        n = spikes.numel()
        out = ops.mt_corrupt(pos[0], pos[1], spikes, cm8, zr, rr, out=out, ws=self._device_ws(n, spikes.device))
        advance_cpu_generator(3 * n)
        self.device_draws = getattr(self, "device_draws", 0) + 1
        return out

    def forward(self, spikes, neuron_regions=None, token_mask_only=False, spikes_discarded=False):
        """`token_mask_only=True` (callers that discard the returned spikes only): skip the zero / random corruption draws.
        `spikes_discarded=True` (the same callers): stay on the reference's generator stream, but move the CPU generator past the
        three [B, T, N] corruption draws by jump-ahead (rngjump.py) instead of taking them; the spikes come back untouched, the masks
        and the generator state afterwards are those of the drawing path.  MMFM_MASKER_JUMP=0 takes the three draws for real (and
        still leaves the spikes alone)."""
        inactive = (not self.training and not self.force_active) or self.target_regions is None \
            or self.mask_regions is None or self.ratio == 0
        if inactive:
            return self._no_mask(spikes)
        if "all" in self.mask_regions:
            self.mask_regions = list(np.unique(neuron_regions))
        if "all" in self.target_regions:
            self.target_regions = list(np.unique(neuron_regions))

        B, T, N = spikes.shape
        dev = spikes.device
        ratio = self.ratio
        targets_sel = None
        if self.mode in TOKEN_MODES:
            timespan = 1
            if torch.bernoulli(torch.tensor(self.expand_prob).float()):
                timespan = torch.randint(1, self.max_timespan + 1, (1,)).item()
            probs = torch.full((B, T), ratio / timespan)
            if self.mode == "causal":
                timespan = torch.randint(1, self.max_timespan + 1, (1,)).item()
                probs = torch.full((B, T), 0.01)
        elif self.mode == "neuron":
            probs = torch.full((B, N), ratio)
        elif self.mode == "random":
            probs = torch.full((B, T, N), ratio)
        elif self.mode == "co-smooth":
            assert self.channels is not None, "No channels to mask"
            probs = torch.zeros(N)
            probs[list(self.channels)] = 1
        elif self.mode == "forward-pred":
            assert self.timesteps is not None, "No time steps to mask"
            probs = torch.zeros(T)
            probs[list(self.timesteps)] = 1
        elif self.mode == "inter-region":
            assert neuron_regions is not None, "Can't mask region without brain region information"
            probs = torch.zeros(B, N)
            for region in random.sample(self.mask_regions, self.n_mask_regions):
                probs[torch.tensor(neuron_regions == region)] = 1
        elif self.mode == "intra-region":
            assert neuron_regions is not None, "Can't mask region without brain region information"
            probs = torch.ones(B, N)
            targets_sel = torch.zeros(B, N)
            for region in random.sample(self.target_regions, self.n_mask_regions):
                sel = torch.tensor(neuron_regions == region)
                probs[sel] = ratio
                targets_sel[sel] = 1
        else:
            raise Exception(f"Masking mode {self.mode} not implemented")

        if self._ring is None:
            self._ring = _PinnedRing()
        drawn = self._device_bernoulli(spikes, ratio) if self.mode == "random" else None
        if drawn is None:
            drawn = self._ring.to(torch.bernoulli(probs), dev)
        causal_target = None
        if self.mode in TOKEN_MODES:
            if timespan > 1:
                drawn = self.expand_timesteps(drawn, timespan)
            if self.causal_zero and self.mode == "causal":
                first = torch.argmax(drawn.int(), dim=1).int()
                causal_target = drawn.clone()
                for b in range(B):
                    drawn[b, first[b]:] = 1
            mask = drawn.unsqueeze(2).expand(B, T, N).bool()
        elif self.mode in ("neuron", "region", "intra-region", "inter-region"):
            mask = drawn.unsqueeze(1).expand(B, T, N).bool()
        elif self.mode == "co-smooth":
            mask = drawn[None, None, :].expand(B, T, N).bool()
        elif self.mode == "forward-pred":
            mask = drawn[None, :, None].expand(B, T, N).bool()
        else:
            mask = drawn.bool()

        if token_mask_only:
            pass
        elif spikes_discarded:
            # bernoulli(zero_ratio x shape), bernoulli(random_ratio x shape), rand(shape): one 32-bit output per element each, and
            # nobody reads the values
            if os.environ.get("MMFM_MASKER_JUMP", "1") != "0":
                from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
                advance_cpu_generator(3 * B * T * N)
            else:
                torch.bernoulli(torch.full((B, T, N), float(self.zero_ratio)))
                torch.bernoulli(torch.full((B, T, N), float(self.random_ratio)))
                torch.rand((B, T, N))
        elif self._device_corrupt(spikes, mask.view(torch.uint8), spikes) is not None:
            pass                                                     # corrupted in place, the generator moved on
        else:
            zero_idx = torch.bernoulli(torch.full((B, T, N), float(self.zero_ratio))).to(dev).bool() & mask
            spikes[zero_idx] = 0
            rand_idx = torch.bernoulli(torch.full((B, T, N), float(self.random_ratio))).to(dev).bool() & mask & ~zero_idx
            # CPU generator on purpose (the reference draws this one on `spikes.device`; the CPU oracle that
            # produced the fixtures has its data on the CPU, SURVEY.md §7 "Masker RNG")
            noise = (spikes.max() * torch.rand((B, T, N)).to(dev)).to(spikes.dtype)
            spikes[rand_idx] = noise[rand_idx]

        if causal_target is not None:
            targets_mask = causal_target.unsqueeze(2).expand(B, T, N).bool()
        elif self.mode == "intra-region":
            targets_mask = mask & targets_sel.unsqueeze(1).expand(B, T, N).bool().to(dev)
        else:
            targets_mask = mask
        return spikes, targets_mask.to(torch.int64)

    def element_masks(self, spikes, neuron_regions=None):
        """The masks of `forward(spikes, neuron_regions)` in compact form, for the engine's per-element loss (mask_type: input with
        `MultiModal.input_masking`).  Returns (cm, tm, corrupted):
          cm, tm     the corruption mask and the target mask as uint8 tensors on `spikes.device` with broadcast dimensions kept at size
                     1: [B,T,1] (temporal / random_token / causal), [B,1,N] (neuron / inter-region / intra-region), [1,1,N] (co-smooth),
                     [1,T,1] (forward-pred), [B,T,N] (random).  tm expanded is `forward`'s targets_mask; the two differ in intra-region
                     and in causal with causal_zero only.  An inactive masker returns two [1,1,1] zeros.
          corrupted  None when zero_ratio == 1: bernoulli(1.0) is always 1, so the zeroed elements are exactly cm and nothing takes
                     noise - the caller zeroes `spikes` under cm itself, and the three [B,T,N] draws are passed by jump-ahead
                     (MMFM_MASKER_JUMP=0: taken for real), as `forward(spikes_discarded=True)` passes them.  For any other zero_ratio the
                     corrupted copy of `spikes` is returned, with `forward`'s bits: for an fp32 CUDA tensor the three draws are generated
                     on the device (ops.mt_corrupt) from the CPU generator's position and the generator jumps past them; otherwise
                     (a CPU tensor, another dtype, MMFM_MASKER_DEVICE=0) they are taken on the host as `forward` takes them.
        The generator calls, their order and shapes, and the states of the CPU generator and of Python's `random` afterwards are
        `forward`'s.  `spikes` is not modified."""
        B, T, N = spikes.shape
        dev = spikes.device
        if self._ring is None:
            self._ring = _PinnedRing()
        inactive = (not self.training and not self.force_active) or self.target_regions is None \
            or self.mask_regions is None or self.ratio == 0
        if inactive:
            zero = torch.zeros(1, 1, 1, dtype=torch.uint8, device=dev)
            return zero, zero, None
        if "all" in self.mask_regions:
            self.mask_regions = list(np.unique(neuron_regions))
        if "all" in self.target_regions:
            self.target_regions = list(np.unique(neuron_regions))
        ratio, mode = self.ratio, self.mode
        tm = None
        if mode in TOKEN_MODES:
            timespan = 1
            if torch.bernoulli(torch.tensor(self.expand_prob).float()):
                timespan = torch.randint(1, self.max_timespan + 1, (1,)).item()
            probs = torch.full((B, T), ratio / timespan)
            if mode == "causal":
                timespan = torch.randint(1, self.max_timespan + 1, (1,)).item()
                probs = torch.full((B, T), 0.01)
            drawn = torch.bernoulli(probs)
            if timespan > 1:
                drawn = self.expand_timesteps(drawn, timespan)
            if self.causal_zero and mode == "causal":
                first = torch.argmax(drawn.int(), dim=1)
                tm = drawn.bool().unsqueeze(2)
                drawn = drawn.clone()
                for b in range(B):
                    drawn[b, first[b]:] = 1
            cm = drawn.bool().unsqueeze(2)
        elif mode in ("neuron", "inter-region", "intra-region"):
            sel = None
            if mode == "neuron":
                probs = torch.full((B, N), ratio)
            else:
                assert neuron_regions is not None, "Can't mask region without brain region information"
                if mode == "inter-region":
                    probs = torch.zeros(B, N)
                    for region in random.sample(self.mask_regions, self.n_mask_regions):
                        probs[torch.tensor(neuron_regions == region)] = 1
                else:
                    probs = torch.ones(B, N)
                    sel = torch.zeros(B, N)
                    for region in random.sample(self.target_regions, self.n_mask_regions):
                        s = torch.tensor(neuron_regions == region)
                        probs[s] = ratio
                        sel[s] = 1
            cm = torch.bernoulli(probs).bool().unsqueeze(1)
            if sel is not None:
                tm = cm & sel.bool().unsqueeze(1)
        elif mode == "co-smooth":
            assert self.channels is not None, "No channels to mask"
            probs = torch.zeros(N)
            probs[list(self.channels)] = 1
            cm = torch.bernoulli(probs).bool()[None, None, :]
        elif mode == "forward-pred":
            assert self.timesteps is not None, "No time steps to mask"
            probs = torch.zeros(T)
            probs[list(self.timesteps)] = 1
            cm = torch.bernoulli(probs).bool()[None, :, None]
        elif mode == "random":
            cm = self._device_bernoulli(spikes, ratio)                # uint8 on the device already, or None
            if cm is None:
                cm = torch.bernoulli(torch.full((B, T, N), ratio)).bool()
        else:
            raise Exception(f"Masking mode {self.mode} not implemented")
        tm = cm if tm is None else tm
        cm8 = cm if cm.is_cuda else self._ring.to(cm.to(torch.uint8).contiguous(), dev)
        tm8 = cm8 if tm is cm else self._ring.to(tm.to(torch.uint8).contiguous(), dev)

        corrupted = None
        if float(self.zero_ratio) == 1.0:
            if os.environ.get("MMFM_MASKER_JUMP", "1") != "0":
                from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
                advance_cpu_generator(3 * B * T * N)
            else:
                torch.bernoulli(torch.full((B, T, N), float(self.zero_ratio)))
                torch.bernoulli(torch.full((B, T, N), float(self.random_ratio)))
                torch.rand((B, T, N))
        elif (corrupted := self._device_corrupt(spikes, cm8, None)) is not None:
            pass
        else:
            mask = cm.to(dev).bool().expand(B, T, N)
            corrupted = spikes.clone()
            zero_idx = torch.bernoulli(torch.full((B, T, N), float(self.zero_ratio))).to(dev).bool() & mask
            corrupted[zero_idx] = 0
            rand_idx = torch.bernoulli(torch.full((B, T, N), float(self.random_ratio))).to(dev).bool() & mask & ~zero_idx
            noise = (corrupted.max() * torch.rand((B, T, N)).to(dev)).to(corrupted.dtype)
            corrupted[rand_idx] = noise[rand_idx]
        return cm8, tm8, corrupted

    @staticmethod
    def expand_timesteps(mask, width=1):
        kernel = torch.ones(width, device=mask.device).view(1, 1, -1)
        return F.conv1d(mask.unsqueeze(1), kernel, padding="same").squeeze(1) >= 1
