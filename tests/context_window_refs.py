"""References of the attention window over time stamps (MMFM_ATTN_WINDOW, include/mmfm.h): the translation of mm.yaml's
(context.forward, context.backward) into the closed interval [lo, hi] the kernels see, the brute-force allowed(b, q, k) with the window,
the stamp recipes and the windows of the kernel tests.  In the style of attn_refs.py, on which the GPU tests rest for everything else.

The rule:  allowed(b, q, k) = (DIAG && q == k) | (keypad[b][k] && lo <= pos[b][k] - pos[b][q] <= hi),  pos = the tokens' time stamps."""
import torch

import dropout_refs as DR

INF = 1 << 30               # "unbounded" of lo / hi (MMFM_ATTN_WINDOW: beyond it they are clamped to it)
POS_CLAMP = 1 << 29         # mmfm_attn_pos_prep clamps the stamps to +-2^29: a difference always fits beside lo / hi

GRID_N = (1, 2, 4, 5, 33, 100)


def grid_values(N):
    """F and Bk of the translation grid: {-1, 0, 1, 2, 5, N - 1, N, N + 3}."""
    return (-1, 0, 1, 2, 5, N - 1, N, N + 3)


def translate(F, Bk):
    """(context.forward, context.backward) -> (lo, hi): -1 is unbounded, and so is backward 0 (upstream's `if context_backward > 0`)."""
    return (-Bk if Bk > 0 else -INF), (F if F >= 0 else INF)


def band(lo, hi, pos):
    """bool [B, L, L]: lo <= pos[b][k] - pos[b][q] <= hi, in int64."""
    d = pos.long()[:, None, :] - pos.long()[:, :, None]
    return (d >= lo) & (d <= hi)


def window_allowed(kp, flags, pos, lo, hi):
    """allowed[b, q, k] under a window, on dropout_refs.allowed_mask (key padding; the diagonal of DIAG); asserts, as attn_refs.build_allowed
    does, that every query row keeps an allowed key: no case may build a row of NaNs.  CAUSAL / SEP are not built under a window."""
    assert not flags & 6, "CAUSAL / SEP are refused under a window"
    B, L = kp.shape
    al = DR.allowed_mask(kp, 0, L) & band(lo, hi, pos.to(kp.device))
    if flags & 1:
        al = al | DR.allowed_mask(torch.zeros_like(kp), 1, L)
    assert bool(al.any(-1).all()), "a query row without an allowed key"
    return al


STAMP_RECIPES = ("arange", "two_mod", "shift7", "shuffled", "constant", "huge")


def stamps(recipe, B, L):
    """int64 [B, L] time stamps.  arange: one modality; two_mod: two modalities arange(T) twice with the boundary inside a 32-tile (T = 20 at
    L = 40, T = 100 at L = 200, else L // 2 moved off a multiple of 32); shift7: arange + 7 b per sample; shuffled: a fixed permutation of
    arange per sample (not monotone inside tiles); constant: every token at stamp 3; huge: arange scaled beyond +-2^29 in samples 0 and 1
    (the clamp of mmfm_attn_pos_prep: every difference saturates) and plain arange in the others."""
    t = torch.arange(L, dtype=torch.int64)
    if recipe == "arange":
        p = t[None].repeat(B, 1)
    elif recipe == "two_mod":
        T = L // 2
        if T % 32 == 0 and L > 2:
            T += 4
        p = torch.cat([torch.arange(T), torch.arange(L - T)])[None].repeat(B, 1)
    elif recipe == "shift7":
        p = t[None] + 7 * torch.arange(B, dtype=torch.int64)[:, None]
    elif recipe == "shuffled":
        p = torch.stack([t[torch.randperm(L, generator=torch.Generator().manual_seed(100 + b))] for b in range(B)])
    elif recipe == "constant":
        p = torch.full((B, L), 3, dtype=torch.int64)
    elif recipe == "huge":
        p = t[None].repeat(B, 1)
        p[0] = (t - L // 2) * (1 << 31)
        if B > 1:
            p[1] = (1 << 40) + t
    else:
        raise ValueError(recipe)
    return p.contiguous()


def clamp_pos(ts):
    """What mmfm_attn_pos_prep writes for the stamps ts: int32 clamp(ts, -2^29, 2^29)."""
    return ts.clamp(-POS_CLAMP, POS_CLAMP).to(torch.int32)


# (name, flags, lo, hi) of the kernel tests.  Windows that exclude a query's own stamp carry DIAG, so that no row is empty.
WINDOWS = [
    ("pm3", 0, -3, 3),
    ("self", 1, 0, 0),
    ("causal_time", 0, -INF, 0),
    ("fwd5", 0, 0, 5),
    ("back8", 0, -8, 0),
    ("far", 1, -40, -33),
    ("all", 0, -INF, INF),
    ("wider", 0, -1000, 1000),
]
