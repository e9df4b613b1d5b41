"""The masker's device-side corruption draws (MMFM_MASKER_DEVICE, models/masker.py over ops.mt_corrupt / mt_bernoulli) against its own
host path on the MI355X: masks, corrupted spikes and the states of both generators for every mode, then one tiny-model input-masking
step - loss and every gradient bit for bit, eager and under graph replay, fp32 and bf16."""
import random

import numpy as np
import pytest
import torch

import input_masking as IM
import model_checks as MC
from helpers import build_model, tiny_config
from test_oracle_golden import default_masker_cfg

pytestmark = pytest.mark.gpu

B, T, N = 3, 8, 12
REGIONS = np.array([["CA1"] * 5 + ["PO"] * 4 + ["LP"] * 3] * B)
MODES = ["temporal", "random_token", "causal", "neuron", "inter-region", "intra-region", "co-smooth", "forward-pred", "random"]


def masker(mode, **kw):
    from models.masker import Masker
    from utils.config_utils import DictConfig
    cfg = default_masker_cfg(mode=mode, expand_prob=0.5, max_timespan=3, channels=[1, 4, 7], timesteps=[2, 5], causal_zero=True,
                             zero_ratio=0.5, random_ratio=1.0, **kw)
    return Masker(DictConfig(cfg))


def two_calls(mode, fn, seed):
    """Two consecutive calls of one masker from one seed: per call the returned tensors and the states of both generators."""
    torch.manual_seed(seed)
    random.seed(seed)
    m = masker(mode)
    res = []
    for _ in range(2):
        out = fn(m)
        res.append((out, torch.get_rng_state(), random.getstate()))
    return m, res


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_gives_the_host_path_s_bits(mode, monkeypatch):
    x = torch.poisson(torch.full((B, T, N), 1.5), generator=torch.Generator().manual_seed(3)).cuda()
    calls = {"element_masks": lambda m: m.element_masks(x, REGIONS), "forward": lambda m: m(x.clone(), REGIONS)}
    for name, fn in calls.items():
        for seed in (0, 5):
            runs = {}
            for switch in ("1", "0"):
                monkeypatch.setenv("MMFM_MASKER_DEVICE", switch)
                runs[switch] = two_calls(mode, fn, seed)
            (m_dev, dev), (m_host, host) = runs["1"], runs["0"]
            per_call = 2 if mode == "random" else 1              # `random` draws its [B, T, N] mask on the device too
            assert m_dev.device_draws == 2 * per_call and m_host.device_draws == 0, (name, m_dev.device_draws, m_host.device_draws)
            for i, ((out_d, g_d, r_d), (out_h, g_h, r_h)) in enumerate(zip(dev, host)):
                assert len(out_d) == len(out_h)
                for a, b in zip(out_d, out_h):
                    assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (mode, name, seed, i)
                assert torch.equal(g_d, g_h), f"{mode} {name} seed {seed} call {i}: CPU generator blob"
                assert r_d == r_h, f"{mode} {name} seed {seed} call {i}: random.getstate()"
            if name == "element_masks":
                cm, _, corrupted = dev[0][0]
                assert corrupted is not None and not torch.equal(corrupted, x * (cm.expand(B, T, N) == 0)), "noise was drawn somewhere"
    assert torch.equal(x.cpu(), torch.poisson(torch.full((B, T, N), 1.5), generator=torch.Generator().manual_seed(3))), "element_masks reads x only"


def test_switches_and_fallbacks(monkeypatch):
    """MMFM_MASKER_JUMP=0 keeps the host draws too; so do another dtype and a non-contiguous tensor; a pickled masker carries no device
    buffer."""
    x = torch.poisson(torch.full((B, T, N), 1.5), generator=torch.Generator().manual_seed(3)).cuda()
    m = masker("neuron")
    m.element_masks(x, REGIONS)
    assert m.device_draws == 1 and len(m._mt_ws) == 1
    state = m.__getstate__()
    assert state["_mt_ws"] == {} and state["device_draws"] == 0 and state["_ring"] is None
    m.element_masks(x.double(), REGIONS)
    m(x.transpose(0, 1).contiguous().transpose(0, 1), REGIONS[:, :N])
    assert m.device_draws == 1
    monkeypatch.setenv("MMFM_MASKER_JUMP", "0")
    m.element_masks(x, REGIONS)
    assert m.device_draws == 1


def fresh(dtype):
    model = build_model(tiny_config(), IM.TINY["n_ap"], IM.TINY["n_beh"], seed=IM.MODEL_SEED, input_masking=True)
    IM.set_masker(model.masker, "real_draw")
    model.compute_dtype = dtype
    return model.cuda().train()


def three_steps(dtype):
    """The `real_draw` step three times from one seed: eager, captured and replayed, replayed (the masker runs outside the captured plan)."""
    model = fresh(dtype)
    batch = IM.case_batch("real_draw")
    res = []
    for _ in range(3):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(IM.MASKER_SEED)
        random.seed(IM.MASKER_SEED)
        out = model(MC.to_dev(IM.make_mod_dict(batch, IM.CASES["real_draw"]["mode"])))
        out.loss.backward()
        res.append((out.loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, torch.get_rng_state()))
    return model, res


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tiny_model_step_is_bit_equal_between_the_switches(dtype, monkeypatch):
    runs = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MMFM_MASKER_DEVICE", switch)
        runs[switch] = three_steps(dtype)
    (m_dev, dev), (m_host, host) = runs["1"], runs["0"]
    assert m_dev.masker.device_draws == 3 * 2 and m_host.masker.device_draws == 0, "one masker call per modality and step"
    plan = m_dev._engine._last
    assert set(plan["graphs"]) == {"fwd", "bwd"} and plan["runs"]["fwd"] == 3, "the third step replays the captured plan"
    for i, ((loss_d, g_d, s_d), (loss_h, g_h, s_h)) in enumerate(zip(dev, host)):
        assert bool(torch.isfinite(loss_d)) and torch.equal(loss_d, loss_h), (i, loss_d.item(), loss_h.item())
        assert list(g_d) == list(g_h) and all(torch.equal(g_d[k], g_h[k]) for k in g_d), i
        assert torch.equal(s_d, s_h)
    assert all(torch.equal(dev[0][0], l) for l, _, _ in dev[1:]), "the same seed: the replayed steps give the eager step's loss"
