"""CPU checks of the test-support code the dropout-on GPU tests lean on (tests/dropout_refs.py, the oracle's dropout_fn hook): a
reference that ignored the masks it is handed, or a hook that changed the oracle, would let those tests pass for the wrong reason."""
import pytest
import torch
import torch.nn.functional as F

import attn_route_grid as G
import dropout_refs as DR
from helpers import load_config, tiny_config
from multi_modal_foundation_model_amd import ops as K
from oracle import mm_oracle as O

VARIANTS = {"base": {}, "sep": dict(sep=True), "deep": dict(n_enc=2, n_dec=2)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("objective", ["encoding", "token_masking"])
def test_oracle_hook_replays_f_dropout_bit_for_bit(variant, objective):
    """The multipliers F.dropout draws under a fixed torch seed, recorded and replayed through dropout_fn, give the oracle's un-hooked
    dropout-on loss and gradients bit for bit (tiny config, dropout 0.4 / 0.2): the hook sits at the five F.dropout sites, names every
    one of them once, and changes nothing else."""
    mc = tiny_config(dropout=0.4, emb_dropout=0.2, **VARIANTS[variant])
    cfg = O.OracleCfg.from_model_config(mc, {"ap": 12, "behavior": 2})
    sd = O.init_state_dict(cfg, seed=3)
    keys = O.trainable_keys(sd, cfg)
    for k in keys:
        sd[k].requires_grad_(True)
    batch = O.synth_batch(3, 8, 12, 2, seed=4, pad=[0, 3, 1])
    mk = O.OracleMasker(dict(load_config().model.masker))

    def run(fn):
        torch.manual_seed(17)
        out = O.forward(sd, O.make_mod_dict(batch, objective), cfg, training=True, masker=mk, dropout_fn=fn)
        return out["loss"].detach(), torch.autograd.grad(out["loss"], [sd[k] for k in keys])

    loss0, g0 = run(None)
    rec = {}

    def record(key, x):
        assert key not in rec, key
        p = cfg.embed_dropout if "/embdrop/" in key else cfg.dropout
        rec[key] = F.dropout(torch.ones_like(x), p, True)          # the same draw F.dropout(x) makes: one bernoulli_ of x's shape
        return rec[key]

    loss1, g1 = run(record)
    n_layers = 2 if variant == "deep" else 1
    assert len(rec) == 4 + (3 + 5) * n_layers
    assert {k.rsplit("/", 1)[-1] for k in rec} == {"0", "1", "p", "o", "mlpdrop"}
    loss2, g2 = run(DR.oracle_dropout_fn(rec))
    for loss, g in ((loss1, g1), (loss2, g2)):
        assert torch.equal(loss, loss0)
        for k, a, b in zip(keys, g, g0):
            assert torch.equal(a, b), k
    # and the masks matter: other multipliers, another loss
    other = {k: torch.roll(v, 1, -1) for k, v in rec.items()}
    assert not torch.equal(run(DR.oracle_dropout_fn(other))[0], loss0)


def test_oracle_without_hook_and_dropout_off_is_unchanged():
    """Hook given but dropout off (eval mode, or p = 0): never called, same result as without it."""
    cfg = O.OracleCfg.from_model_config(tiny_config(), {"ap": 12, "behavior": 2})
    sd = O.init_state_dict(cfg, seed=3)
    batch = O.synth_batch(2, 8, 12, 2, seed=1)

    def boom(key, x):
        raise AssertionError(key)

    for training in (False, True):
        a = O.forward(sd, O.make_mod_dict(batch, "encoding"), cfg, training=training)["loss"]
        b = O.forward(sd, O.make_mod_dict(batch, "encoding"), cfg, training=training, dropout_fn=boom)["loss"]
        assert torch.equal(a, b)


def test_attention_reference_moves_when_the_two_masks_swap_sites():
    """The fp64 attention reference of tests/test_attention_outdrop_gpu.py on a (2, 4, 48, 16) case: with the drop_p mask and the drop_o
    multiplier taken from each other's (probability, site) - what a swapped threshold, scale or site id in a kernel amounts to - output and
    gradients move by far more than the 2e-2 / 3e-2 of max |ref| the GPU test allows, so that test cannot pass on swapped masks."""
    B, heads, L, dh = 2, 4, 48, 16
    H = heads * dh
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, heads, L, dh, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    d_o = torch.randn(B * L, H, generator=g, dtype=torch.float64)
    kp = torch.ones(B, L, dtype=torch.uint8)
    kp[0, L - 3:] = 0
    kp[B - 1, 5:9] = 0
    allowed = DR.allowed_mask(kp, 1, L)

    def masks(p_att, p_out, seed):
        gg = torch.Generator().manual_seed(seed)
        mp = (torch.rand(B, heads, L, L, generator=gg) >= p_att).double() / (1 - p_att)
        mo = (torch.rand(B * L, H, generator=gg) >= p_out).double() / (1 - p_out)
        return mp, mo

    def run(mp, mo):
        o, lse = DR.attention_dropout_ref(q, k, v, allowed, dh ** -0.5, mp, mo)
        return [o.detach()] + [t.detach() for t in torch.autograd.grad(o, (q, k, v), d_o)]

    right = run(*masks(0.4, 0.25, 1))
    again = run(*masks(0.4, 0.25, 1))
    swapped = run(*masks(0.25, 0.4, 1))                        # the probabilities change places (threshold and scale of the other site)
    other = run(*masks(0.4, 0.25, 2))                          # the same probabilities, other decisions (another site id)
    for name, tol, r, a, s, t in zip(("o", "dq", "dk", "dv"), (2e-2, 3e-2, 3e-2, 3e-2), right, again, swapped, other):
        assert torch.equal(r, a)
        scale = r.abs().max().item()
        for what, w in (("swapped probabilities", s), ("other site", t)):
            err = (w - r).abs().max().item()
            assert err > 10 * tol * scale, f"{name}, {what}: moves by {err:.3e} only (tolerance {tol * scale:.3e})"
    # no masks: plain attention (softmax rows sum to one; padded keys carry no weight)
    o_plain, lse = DR.attention_dropout_ref(q, k, torch.ones_like(v), allowed, dh ** -0.5)
    assert torch.allclose(o_plain, torch.ones_like(o_plain)) and bool(torch.isfinite(lse).all())


def test_survivor_scale_is_the_fp32_quotient():
    assert DR.survivor_scale(0.4) == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.4)))
    assert DR.survivor_scale(0.25) == 4.0 / 3.0 or abs(DR.survivor_scale(0.25) - 4.0 / 3.0) < 1e-7


def test_keepbit_literal_points_under_causal():
    """Which self-attention launches of the engine (bf16, aligned, workspace passed, drop_p on) draw drop_p from the keep-bit workspace,
    at the literal points the read-out of tests/dropout_refs.py was first written for, asked of the library with CAUSAL set: 2656 / 2664 is
    the masked bound of the dh-128 kernels' LDS (tests/test_attn_route_cpu.py has the dense counterparts)."""
    from multi_modal_foundation_model_amd import _lib as Lb

    def keepbit_path(dh, Lq, Lk):
        return DR.on_keepbit_kernels(G.desc(K, Lb, Lb.BF16, dh, Lq, Lk, Lb.ATTN_CAUSAL, workspace=True, drop_p=0.4))

    assert keepbit_path(32, 200, 200) and keepbit_path(64, 600, 600) and not keepbit_path(32, 264, 264) and not keepbit_path(32, 204, 204)
    assert keepbit_path(128, 200, 200) and keepbit_path(128, 2656, 2656) and not keepbit_path(128, 2664, 2664) and not keepbit_path(128, 204, 204)
