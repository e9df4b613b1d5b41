"""MT19937 jump-ahead behind the reference-exact masker stream (csrc/mt_jump.cpp, rngjump.py, models/masker.py): the CPU
generator after a jump must be, byte for byte, the generator after the draws that the jump replaces.  No GPU involved: the
stream belongs to torch's CPU generator and the jump is host code of the library."""
import random
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import ROOT, load_npz

N_BIG = 3 * 1024 * 100 * 668          # 205,209,600: the default 'ap' modality at B = 1024
SEEDS = (0, 42, 20240229)
PRE_DRAWS = (0, 5, 623, 624)          # 0: freshly seeded, nothing drawn
SMALL_N = (0, 1, 623, 624, 625, 19937, 3 * 2 * 8 * 12, 3 * 16 * 100 * 668)


def _start(seed, pre):
    torch.manual_seed(seed)
    if pre:
        torch.empty(pre, dtype=torch.int32).random_()


def _draw(n):
    if n:
        torch.empty(n, dtype=torch.int32).random_()


def _after():
    """Everything that tells two generator states apart: the blob and the next float / normal draws."""
    blob = torch.get_rng_state()
    return blob, torch.rand(3), torch.randn(3)


def _assert_same(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: get_rng_state() blobs differ"
    assert torch.equal(got[1], want[1]), f"{what}: next rand(3) differs"
    assert torch.equal(got[2], want[2]), f"{what}: next randn(3) differs"


@pytest.fixture(scope="module")
def big_draws():
    """The 205 M real draws, once: the state they leave (from a mid-block start) and what they cost."""
    _start(7, 5)
    t0 = time.perf_counter()
    _draw(N_BIG)
    dt = time.perf_counter() - t0
    return dict(seed=7, pre=5, after=_after(), seconds=dt)


@pytest.mark.parametrize("pre", PRE_DRAWS)
@pytest.mark.parametrize("seed", SEEDS)
def test_jump_equals_draws(seed, pre):
    from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
    for n in SMALL_N:
        _start(seed, pre)
        _draw(n)
        want = _after()
        _start(seed, pre)
        advance_cpu_generator(n)
        _assert_same(_after(), want, f"seed {seed}, {pre} draws before, n = {n}")


def test_jump_equals_draws_at_full_size(big_draws):
    from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
    _start(big_draws["seed"], big_draws["pre"])
    advance_cpu_generator(N_BIG)
    _assert_same(_after(), big_draws["after"], f"n = {N_BIG}")


def test_bookkeeping_fresh_and_block_boundary():
    """n = 0 keeps a fresh state fresh (left = 1, next = 0); a jump that ends on a block boundary leaves left = 1, next = 624 as
    real draws do; a normal sample cached in the blob's tail survives a jump."""
    from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator, parse_state
    torch.manual_seed(5)
    fresh = torch.get_rng_state()
    advance_cpu_generator(0)
    assert torch.equal(torch.get_rng_state(), fresh)
    assert parse_state(fresh)[1:4] == (1, 1, 0)
    for n in (624, 624 * 5000):
        torch.manual_seed(5)
        advance_cpu_generator(n)
        assert parse_state(torch.get_rng_state())[1:4] == (1, 1, 624), n
    torch.manual_seed(5)
    torch.randn(1)                                     # leaves the second normal of the pair cached in the tail
    tail = torch.get_rng_state()[-40:].clone()
    advance_cpu_generator(624 * 5000 + 3)
    assert torch.equal(torch.get_rng_state()[-40:], tail)
    gen = torch.Generator().manual_seed(11)            # a generator of one's own, the global one untouched
    before = torch.get_rng_state()
    advance_cpu_generator(3206400, generator=gen)
    ref = torch.Generator().manual_seed(11)
    torch.empty(3206400, dtype=torch.int32).random_(generator=ref)
    assert torch.equal(gen.get_state(), ref.get_state()) and torch.equal(torch.get_rng_state(), before)


def test_c_abi_checks_arguments_and_needs_no_device():
    from multi_modal_foundation_model_amd import _lib as L, ops
    st = torch.zeros(624, dtype=torch.int32)
    with pytest.raises(L.MmfmError, match="consumed"):
        ops.mt19937_jump(st, 625, 1)
    with pytest.raises(TypeError):
        ops.mt19937_jump(torch.zeros(623, dtype=torch.int32), 0, 1)
    assert ops.mt19937_jump(st, 3, 0) == 3 and ops.mt19937_jump(st, 3, 621) == 624 and ops.mt19937_jump(st, 624, 1) == 1
    # a long jump in a process of its own: the HIP runtime is never initialised by it
    code = ("import torch\n"
            "from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator\n"
            "torch.manual_seed(1); advance_cpu_generator(3206400); a = torch.get_rng_state()\n"
            "torch.manual_seed(1); torch.empty(3206400, dtype=torch.int32).random_()\n"
            "assert torch.equal(a, torch.get_rng_state()) and not torch.cuda.is_initialized()\n"
            "print('jump-ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "jump-ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("shape", [(2, 8, 12), (16, 100, 668)])
@pytest.mark.parametrize("probs", [(1.0, 1.0), (0.3, 0.7)])
def test_discarded_draws_are_a_pure_advance(shape, probs):
    """What the feature rests on: bernoulli(full(shape, p)) twice plus rand(shape) moves the generator by 3 * B * T * N outputs."""
    from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
    B, T, N = shape
    for pre in (0, 5):
        _start(13, pre)
        torch.bernoulli(torch.full(shape, probs[0]))
        torch.bernoulli(torch.full(shape, probs[1]))
        torch.rand(shape)
        want = _after()
        _start(13, pre)
        advance_cpu_generator(3 * B * T * N)
        _assert_same(_after(), want, f"{shape}, p = {probs}, {pre} draws before")


def _run_masker(cfg, x, regions, seed, rseed, calls=2, **kw):
    from models.masker import Masker
    from utils.config_utils import DictConfig
    mk = Masker(DictConfig(cfg))
    mk.train()
    torch.manual_seed(seed)
    random.seed(rseed)
    outs = [mk(x.clone(), regions, **kw) for _ in range(calls)]
    return outs, torch.get_rng_state(), random.getstate()


def _masker_cases():
    z, cases = load_npz("masker_bits.npz")
    for c in cases:
        yield f"bits{c['id']}", c["cfg"], torch.from_numpy(z[f"c{c['id']}/ap"]), np.full((4, 9), "XX"), c["seed"], 1
    z, meta = load_npz("masker_modes.npz")
    for cid, c in enumerate(meta):
        ap = torch.from_numpy(z[f"c{cid}/ap"])
        yield f"modes{cid}:{c['cfg']['mode']}", c["cfg"], ap, np.asarray([c["regions"]] * ap.shape[0]), 3 + cid, 17 + cid


@pytest.mark.parametrize("jump_env", ["1", "0"])
def test_masker_spikes_discarded_matches_drawing(monkeypatch, jump_env):
    """Every masker_bits case and every mode of masker_modes, two consecutive calls: spikes_discarded=True gives the masks and leaves
    the torch and `random` states of the drawing path, and hands the spikes back untouched.  MMFM_MASKER_JUMP=0 takes the draws."""
    from multi_modal_foundation_model_amd import rngjump
    calls = []
    real = rngjump.advance_cpu_generator
    monkeypatch.setattr(rngjump, "advance_cpu_generator", lambda n, generator=None: (calls.append(n), real(n, generator))[1])
    monkeypatch.setenv("MMFM_MASKER_JUMP", jump_env)
    seen = 0
    for name, cfg, x, regions, seed, rseed in _masker_cases():
        want, t_want, r_want = _run_masker(cfg, x, regions, seed, rseed)
        assert calls == [], "callers that use the spikes never reach the jump"
        got, t_got, r_got = _run_masker(cfg, x, regions, seed, rseed, spikes_discarded=True)
        for (xs_w, m_w), (xs_g, m_g) in zip(want, got):
            assert torch.equal(m_g, m_w), f"{name}: masks differ"
            assert torch.equal(xs_g, x), f"{name}: the discarded spikes are handed back untouched"
        assert torch.equal(t_got, t_want), f"{name}: torch generator states differ"
        assert r_got == r_want, f"{name}: random states differ"
        B, T, N = x.shape
        assert calls == ([3 * B * T * N] * 2 if jump_env == "1" else []), name
        calls.clear()
        seen += 1
    assert seen >= 11
    # token_mask_only wins over spikes_discarded (the trainer's default stream is unchanged)
    name, cfg, x, regions, seed, rseed = next(_masker_cases())
    a = _run_masker(cfg, x, regions, seed, rseed, token_mask_only=True)
    b = _run_masker(cfg, x, regions, seed, rseed, token_mask_only=True, spikes_discarded=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0][1][1], b[0][1][1]) and calls == []


def test_unparsable_blob_falls_back_to_drawing(monkeypatch):
    from multi_modal_foundation_model_amd import ops, rngjump
    jumps = []
    real = ops.mt19937_jump
    monkeypatch.setattr(ops, "mt19937_jump", lambda *a: (jumps.append(a[2]), real(*a))[1])
    n = 3 * 16 * 100 * 668
    _start(9, 5)
    _draw(n)
    want = _after()
    monkeypatch.setattr(rngjump, "parse_state", lambda blob: None)
    _start(9, 5)
    rngjump.advance_cpu_generator(n)
    _assert_same(_after(), want, "parser refuses the blob")
    assert jumps == []
    monkeypatch.undo()
    # a blob of another length is refused by the real parser, and one that does not survive the round trip by _jump
    assert rngjump.parse_state(torch.zeros(5048, dtype=torch.uint8)) is None
    monkeypatch.setattr(rngjump, "build_state", lambda *a: torch.zeros(5056, dtype=torch.uint8))
    _start(9, 5)
    rngjump.advance_cpu_generator(n)
    _assert_same(_after(), want, "round-trip check fails")


def test_jump_is_not_drawing_in_disguise(big_draws):
    """At n = 205,209,600 with the polynomial cached, the jump takes at most 1/25 of the real int32 draws' time (330 ms of draws
    per step against a 29.6 ms GPU step: 1/25 of the draws hides behind the step).  Expected: several hundred times faster."""
    from multi_modal_foundation_model_amd import ops
    from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator
    ops.mt19937_jump_reset()
    _start(big_draws["seed"], big_draws["pre"])
    t0 = time.perf_counter()
    advance_cpu_generator(N_BIG)
    cold = time.perf_counter() - t0
    _assert_same(_after(), big_draws["after"], "cold jump")
    warm = []
    for _ in range(3):
        _start(big_draws["seed"], big_draws["pre"])
        t0 = time.perf_counter()
        advance_cpu_generator(N_BIG)
        warm.append(time.perf_counter() - t0)
    _assert_same(_after(), big_draws["after"], "warm jump")
    draws = big_draws["seconds"]
    print(f"\nn = {N_BIG}: real int32 draws {draws * 1e3:.1f} ms; jump, polynomial cached {min(warm) * 1e3:.3f} ms "
          f"(x{draws / min(warm):.0f}); cold (phi + t^e mod phi for one block count + jump) {cold * 1e3:.1f} ms")
    assert max(warm) <= draws / 25, f"jump {max(warm) * 1e3:.2f} ms against draws {draws * 1e3:.1f} ms"
