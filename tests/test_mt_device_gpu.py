"""MT19937 on the device (csrc/mt_device.hip: mmfm_mt_uniform / _bernoulli / _corrupt) against torch's own CPU generator set to the same
state.  Everything is compared with torch.equal: there is no tolerance anywhere in this feature.  Runs on the MI355X only."""
import pytest
import torch

import mt_device_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


@pytest.mark.parametrize("prior", R.PRIORS, ids=lambda p: "fresh" if p is None else f"after{p}")
def test_uniform_and_bernoulli_are_torch_s_bits(ops, prior):
    """Every start position x every length x skip in {0, n, 2n}: mt_uniform == torch.rand, mt_bernoulli == torch.bernoulli(full(p)) for
    every p; outputs start as sentinels with guard elements behind them."""
    blob = R.seek(prior)
    state, consumed = R.position(blob)
    for n in R.LENGTHS:
        torch.set_rng_state(blob)
        want_u = torch.rand(3 * n).cuda()
        want_b = {}
        for p in R.PS:
            torch.set_rng_state(blob)
            want_b[p] = torch.bernoulli(torch.full((3 * n,), p)).to(torch.uint8).cuda()
        for skip in (0, n, 2 * n):
            full, out = R.guarded(n, torch.float32)
            ops.mt_uniform(state, consumed, n, skip=skip, out=out)
            assert torch.equal(out, want_u[skip:skip + n]) and R.guard_intact(full, n), (prior, n, skip)
            for p in R.PS:
                full, out = R.guarded(n, torch.uint8)
                ops.mt_bernoulli(state, consumed, n, p, skip=skip, out=out)
                assert torch.equal(out, want_b[p][skip:skip + n]) and R.guard_intact(full, n), (prior, n, skip, p)
    assert torch.equal(R.position(blob)[0], state), "the caller's state array is only read"


@pytest.fixture(scope="module")
def mid_reference():
    """torch.rand / torch.bernoulli(0.3) of the B = 16 masker call's 3 * 1,068,800 outputs from one position (computed once)."""
    blob = R.seek(397, seed=99)
    want_u = torch.rand(R.N_MID).cuda()
    torch.set_rng_state(blob)
    want_b = torch.bernoulli(torch.full((R.N_MID,), 0.3)).to(torch.uint8).cuda()
    return R.position(blob), want_u, want_b


def test_streams_do_not_change_the_bits(ops, mid_reference):
    """Forced stream counts 1, 2, 3, 8 (and the library's choice) at n = 10,007 and at 3 * 1,068,800, and the count the library picks for the
    B = 1024 call forced onto 3 * 1,068,800: the production decomposition (jump tree included) at a size the host reproduces quickly."""
    production = ops.mt_plan(R.N_BIG)[0]
    assert production > 8, "the B = 1024 call is cut into many runs"
    blob = R.seek(5, seed=7)
    state, consumed = R.position(blob)
    want = torch.rand(10007).cuda()
    for streams in (None, 1, 2, 3, 8):
        full, out = R.guarded(10007, torch.float32)
        ops.mt_uniform(state, consumed, 10007, streams=streams, out=out)
        assert torch.equal(out, want) and R.guard_intact(full, 10007), streams
    (state, consumed), want_u, want_b = mid_reference
    for streams in (None, 1, 2, 3, 8, production):
        full, out = R.guarded(R.N_MID, torch.float32)
        ops.mt_uniform(state, consumed, R.N_MID, streams=streams, out=out)
        assert torch.equal(out, want_u) and R.guard_intact(full, R.N_MID), streams
        full, out = R.guarded(R.N_MID, torch.uint8)
        ops.mt_bernoulli(state, consumed, R.N_MID, 0.3, streams=streams, out=out)
        assert torch.equal(out, want_b) and R.guard_intact(full, R.N_MID), streams
    # a skip that lands in the middle of the tensor, through the production cut
    n = R.N_MID // 3
    out = ops.mt_uniform(state, consumed, n, skip=n, streams=production, device="cuda")
    assert torch.equal(out, want_u[n:2 * n])


def _spikes(B, T, N, gen):
    return (torch.randint(0, 6, (B, T, N), generator=gen).float() + torch.rand((B, T, N), generator=gen).round() * 0.25).cuda()


@pytest.mark.parametrize("shape", [(2, 8, 12), (3, 7, 5), (16, 100, 668)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cm_kind", ["BT1", "B1N", "11N", "1T1", "BTN"])
def test_corrupt_is_the_masker_s_host_lines(ops, shape, cm_kind):
    B, T, N = shape
    gen = torch.Generator().manual_seed(B * 1000 + N)
    spikes = _spikes(B, T, N, gen)
    cm = R.cm_of(cm_kind, B, T, N, gen, "cuda")
    production = ops.mt_plan(1024 * 100 * 668)[0]
    for i, (zr, rr) in enumerate(R.RATIOS):
        blob = R.seek((None, 1, 397, 623, 625)[i], seed=11 + i)
        state, consumed = R.position(blob)
        want, zero_idx, rand_idx = R.host_corrupt(spikes, cm, zr, rr)
        if 0 < zr < 1 and rr == 1:
            assert bool(zero_idx.any()) and bool(rand_idx.any()), "the case draws both kinds"
        for streams in ((None, 3) if B * T * N < 10000 else (None, 8, production)):
            full, out = R.guarded(B * T * N, torch.float32)
            got = ops.mt_corrupt(state, consumed, spikes, cm, zr, rr, streams=streams, out=out.view(B, T, N))
            assert torch.equal(got, want) and R.guard_intact(full, B * T * N), (shape, cm_kind, zr, rr, streams)
    # in place, as Masker.forward corrupts the caller's tensor
    own = spikes.clone()
    assert ops.mt_corrupt(state, consumed, own, cm, zr, rr, out=own) is own and torch.equal(own, want)


@pytest.mark.parametrize("streams", [None, 3])
def test_corrupt_nan_follows_torch_max(ops, streams):
    """A NaN that survives the zeroing makes every noise value NaN (torch.max propagates it); a NaN under a zeroed element does not."""
    B, T, N = 3, 7, 5
    gen = torch.Generator().manual_seed(3)
    spikes = _spikes(B, T, N, gen)
    cm = torch.ones(B, T, N, dtype=torch.uint8, device="cuda")
    blob = R.seek(100, seed=21)
    state, consumed = R.position(blob)
    _, zero_idx, rand_idx = R.host_corrupt(spikes, cm, 0.5, 1.0)
    zeroed, kept = zero_idx.nonzero()[0], rand_idx.nonzero()[0]
    # under a zeroed element: finite everywhere, and the oracle's bits
    s1 = spikes.clone()
    s1[tuple(zeroed)] = float("nan")
    torch.set_rng_state(blob)
    want, _, _ = R.host_corrupt(s1, cm, 0.5, 1.0)
    got = ops.mt_corrupt(state, consumed, s1, cm, 0.5, 1.0, streams=streams)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    # surviving (outside the mask, so that nothing overwrites it): every noise element is NaN, the others are the oracle's
    cm2 = cm.clone()
    cm2[tuple(kept)] = 0
    s2 = spikes.clone()
    s2[tuple(kept)] = float("nan")
    torch.set_rng_state(blob)
    want, _, rand2 = R.host_corrupt(s2, cm2, 0.5, 1.0)
    got = ops.mt_corrupt(state, consumed, s2, cm2, 0.5, 1.0, streams=streams)
    assert bool(rand2.any()) and bool(want[rand2].isnan().all()), "the oracle itself: torch.max hands the NaN on"
    assert torch.equal(got.isnan(), want.isnan()) and bool(got[rand2].isnan().all())
    assert torch.equal(got.nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0))
