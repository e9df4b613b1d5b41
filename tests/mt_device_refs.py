"""Helpers of the device-side MT19937 tests: generator positions, the (state, consumed) pair the library takes, and the masker's host
corruption lines as the oracle."""
import torch

from multi_modal_foundation_model_amd import rngjump

PRIORS = (None, 1, 226, 227, 396, 397, 453, 454, 622, 623, 624, 625)      # None: freshly seeded, nothing drawn
LENGTHS = (1, 2, 623, 624, 625, 1253, 10007)
PS = (0.0, 0.01, 0.3, 0.5, 1.0)
RATIOS = ((0.5, 1.0), (0.8, 0.5), (0.0, 1.0), (1.0, 1.0), (0.5, 0.0))
N_MID = 3 * 1068800                    # the B = 16 masker call
N_BIG = 3 * 68403200                   # the B = 1024 masker call
GUARD = 1024


def seek(prior, seed=1234):
    """Puts torch's CPU generator `prior` outputs behind `seed` and returns its blob."""
    torch.manual_seed(seed)
    if prior:
        torch.empty(prior, dtype=torch.int32).random_()
    return torch.get_rng_state()


def position(blob=None):
    """(state int32[624], consumed) of a generator blob (default: the current one), as ops.mt_* take them."""
    _, left, _, nxt, words, _ = rngjump.parse_state(torch.get_rng_state() if blob is None else blob)
    return words.to(torch.int32), (rngjump.N_WORDS if (left == 1 and nxt == 0) else nxt)


def cm_of(kind, B, T, N, gen, device):
    shape = {"BT1": (B, T, 1), "B1N": (B, 1, N), "11N": (1, 1, N), "1T1": (1, T, 1), "BTN": (B, T, N)}[kind]
    return (torch.rand(shape, generator=gen) < 0.6).to(torch.uint8).to(device)


def host_corrupt(spikes, cm, zero_ratio, random_ratio):
    """models/masker.py's corruption lines (element_masks' non-trivial branch), drawing on torch's CPU generator."""
    B, T, N = spikes.shape
    dev = spikes.device
    mask = cm.bool().expand(B, T, N)
    corrupted = spikes.clone()
    zero_idx = torch.bernoulli(torch.full((B, T, N), float(zero_ratio))).to(dev).bool() & mask
    corrupted[zero_idx] = 0
    rand_idx = torch.bernoulli(torch.full((B, T, N), float(random_ratio))).to(dev).bool() & mask & ~zero_idx
    noise = (corrupted.max() * torch.rand((B, T, N)).to(dev)).to(corrupted.dtype)
    corrupted[rand_idx] = noise[rand_idx]
    return corrupted, zero_idx, rand_idx


def guarded(n, dtype, device="cuda"):
    """A sentinel-filled buffer of n + GUARD elements and its first n (NaN for floats, 0xA5 for bytes)."""
    full = torch.full((n + GUARD,), float("nan") if dtype.is_floating_point else 0xA5, dtype=dtype, device=device)
    return full, full[:n]


def guard_intact(full, n):
    tail = full[n:]
    return bool(tail.isnan().all()) if full.dtype.is_floating_point else bool((tail == 0xA5).all())
