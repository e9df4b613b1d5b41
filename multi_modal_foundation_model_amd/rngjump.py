"""Advance torch's CPU generator by a known number of 32-bit outputs without drawing them.

The generator is MT19937; `get_state()` returns its legacy blob:

    uint64 seed | int32 left | int32 seeded | uint64 next | 624 state words as uint64 each | 40-byte tail

(the tail is the cached normal sample and its valid flags: untouched here).  The engine hands out `state[next]` after
regenerating all 624 words in place whenever `--left == 0`, so between draws `left + next == 625`; a freshly seeded engine is
`left = 1, next = 0` over a seed-initialised block of which nothing has been handed out.  `advance_cpu_generator(n)` parses the
blob, moves the 624 words on through the library's jump-ahead (ops.mt19937_jump: linear algebra over GF(2), no draw) and writes
the bookkeeping that `n` real draws would have left.  Anything unexpected in the blob falls back to really drawing `n` int32
values, which is always correct.
"""
from __future__ import annotations

import torch

N_WORDS = 624
_HEAD = 3                                  # int64 words before the state: seed, (left, seeded), next
_BLOB_BYTES = 5056
_DRAW_CHUNK = 1 << 24


def parse_state(blob):
    """(seed, left, seeded, next, words[624] int64, tail bytes) of a generator blob, or None if it does not read as one."""
    if blob.dtype != torch.uint8 or blob.dim() != 1 or blob.numel() != _BLOB_BYTES:
        return None
    q = blob.view(torch.int64)
    left, seeded = (int(v) for v in q[1:2].view(torch.int32))
    nxt = int(q[2])
    words = q[_HEAD:_HEAD + N_WORDS].clone()
    tail = blob[(_HEAD + N_WORDS) * 8:].clone()
    if seeded != 1 or int(words.min()) < 0 or int(words.max()) > 0xFFFFFFFF:
        return None
    if not ((left == 1 and nxt == 0) or (1 <= left <= N_WORDS and left + nxt == N_WORDS + 1)):
        return None
    return int(q[0]), left, seeded, nxt, words, tail


def build_state(seed, left, seeded, nxt, words, tail):
    blob = torch.empty(_BLOB_BYTES, dtype=torch.uint8)
    q = blob.view(torch.int64)
    q[0] = seed
    q[1:2].view(torch.int32).copy_(torch.tensor([left, seeded], dtype=torch.int32))
    q[2] = nxt
    q[_HEAD:_HEAD + N_WORDS] = words
    blob[(_HEAD + N_WORDS) * 8:] = tail
    return blob


def _position(gen):
    """(parsed blob, state int32[624], consumed) of a CPU generator, or None if its blob is not the layout this module knows."""
    blob = gen.get_state()
    parsed = parse_state(blob)
    if parsed is None or not torch.equal(build_state(*parsed), blob):
        return None
    _, left, _, nxt, words, _ = parsed
    return parsed, words.to(torch.int32), (N_WORDS if (left == 1 and nxt == 0) else nxt)     # wraps: the 32 bits of every word


def cpu_generator_position(generator=None):
    """(state, consumed) of `generator` (default: torch's global CPU generator) as ops.mt19937_jump and the device draws (ops.mt_uniform,
    mt_bernoulli, mt_corrupt) take them, or None where `advance_cpu_generator` would fall back to drawing."""
    pos = _position(torch.default_generator if generator is None else generator)
    return None if pos is None else pos[1:]


def _jump(gen, n):
    from . import ops
    pos = _position(gen)
    if pos is None:
        return False
    (seed, left, seeded, nxt, words, tail), state, consumed = pos
    consumed = ops.mt19937_jump(state, consumed, n)
    words = state.to(torch.int64) & 0xFFFFFFFF
    gen.set_state(build_state(seed, N_WORDS + 1 - consumed, seeded, consumed, words, tail))
    return True


def _draw(gen, n):
    buf = torch.empty(min(n, _DRAW_CHUNK), dtype=torch.int32)
    while n > 0:
        k = min(n, _DRAW_CHUNK)
        buf[:k].random_(generator=gen)
        n -= k


def advance_cpu_generator(n, generator=None):
    """Leaves `generator` (default: torch's global CPU generator) where `n` int32 draws would: `torch.empty(n, dtype=torch.int32)
    .random_()`, or any CPU draws that take `n` 32-bit outputs (float bernoulli / rand of `n` elements)."""
    n = int(n)
    if n < 0:
        raise ValueError(f"advance_cpu_generator: n = {n}")
    if n == 0:
        return
    gen = torch.default_generator if generator is None else generator
    if gen.device.type != "cpu":
        raise ValueError("advance_cpu_generator: a CPU generator is expected")
    if not _jump(gen, n):
        _draw(gen, n)
