"""The du-only front half of the fused MLP backward: mmfm_mlp_bwd with dx == NULL and t1 == NULL && g == NULL (MMFM_MLP_DX_ONLY;
csrc/mlp_fused.hip mlp_bwd_du_kernel<ACT, true>).

The form leaves out the t1 and g stores and nothing else, so its du must be the full front half's bit for bit - on the exact-integer
inputs of tests/rowowner_refs.py (where du is also the reference's, exactly) and on randn inputs (where the full form's g and du are
held to check_mlp_bwd's bounds), with the sentinel-filled guard rows around du untouched.  What can go wrong silently is the count of
stores the weight ring's wait may leave in flight (RINGA_SYNC's EXTRA): too large a count multiplies a weight chunk that has not
landed, now and then.  The largest row count gives some workgroups a second pass, and runs on five seeds."""
import ctypes

import pytest
import torch

import rowowner_refs as RR
from multi_modal_foundation_model_amd import _lib as L

pytestmark = pytest.mark.gpu

BF, FILL, GUARD = torch.bfloat16, -7777.0, 64
ROWS = [33, 129, 1000, 516 * 128 + 37]
ACTS = [L.MLP_GELU, L.MLP_RELU, L.MLP_SIGMOID, L.MLP_GELU_TANH]


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda") * scale


def obuf(R, N):
    return torch.full((R + GUARD, N), FILL, device="cuda", dtype=BF)


def done(buf, R, what):
    RR.assert_written(buf[:R], FILL, what)
    RR.assert_untouched(buf[R:], FILL, f"{what}: guard rows")
    return buf[:R]


def prep_linear(ops, W, gamma=None, beta=None, bias=None):
    N, K = W.shape
    e = dict(W=W, gamma=gamma, beta=beta, bias=bias, Wp=torch.empty(N, K, device="cuda", dtype=BF), WpT=torch.empty(K, N, device="cuda", dtype=BF),
             bp=torch.empty(N, device="cuda"), WpP=torch.empty(N, K, device="cuda", dtype=BF), WpTP=torch.empty(K, N, device="cuda", dtype=BF))
    table, n, tiles = ops.prep_table([e], "cuda")
    ops.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return e


def both_forms(ops, R, xh, dy, up, dn, kind, what, drop=None, rotate=1):
    """The full front half (t1, g, du) and the du-only one on the same operands.  Returns the [R, .] views t1, g, du of the full form;
    asserts that the du-only form wrote the same du, every element of it, and nothing into its guard rows."""
    kw = dict(w_up=up["Wp"], b_up=up["bp"], xhat=xh, dy=dy, w_down_t=dn["WpT"], dx=None, act=kind, rotate=rotate, drop=drop)
    t1, g, du, du2 = obuf(R, 256), obuf(R, 512), obuf(R, 512), obuf(R, 512)
    ops.mlp_bwd(ops.mlp_desc(R, t1=t1, g=g, du=du, **kw))
    ops.mlp_bwd(ops.mlp_desc(R, t1=None, g=None, du=du2, **kw))
    full = done(t1, R, f"{what} t1"), done(g, R, f"{what} g"), done(du, R, f"{what} du")
    RR.check_exact(done(du2, R, f"{what} du (du only)"), full[2], f"{what}: du of the du-only form against the full front half's")
    return full


@pytest.mark.parametrize("R", ROWS)
def test_du_only_on_exact_integers(ops, R):
    for seed in range(5 if R == ROWS[-1] else 1):
        c = RR.exact_mlp(R, "cuda", seed=R + seed)
        up, dn = prep_linear(ops, c["Wu"], bias=c["bu"]), prep_linear(ops, c["Wd"], bias=c["bd"])
        for rotate in (0, 1):
            what = f"mlp du-only exact R={R} seed={seed} rotate={rotate}"
            t1, g, du = both_forms(ops, R, c["xhat"], c["dy"], up, dn, RR.ACT_RELU, what, rotate=rotate)
            RR.check_exact(t1, c["dy"], f"{what} t1")
            RR.check_exact(g, c["g"], f"{what} g")
            RR.check_exact(du, c["du"], f"{what} du")


def randn_case(ops, R, seed):
    x = rnd(R, 256, seed=seed + 1) * 1.5 + rnd(R, 1, seed=seed + 2)
    xh = torch.nn.functional.layer_norm(x, (256,)).to(BF)
    dy = rnd(R, 256, seed=seed + 77).to(BF)
    up = prep_linear(ops, rnd(512, 256, seed=seed + 3, scale=1 / 16), gamma=1 + 0.3 * rnd(256, seed=seed + 7), beta=0.2 * rnd(256, seed=seed + 8),
                     bias=0.1 * rnd(512, seed=seed + 4))
    dn = prep_linear(ops, rnd(256, 512, seed=seed + 5, scale=1 / 22), bias=0.1 * rnd(256, seed=seed + 6))
    return xh, dy, up, dn


@pytest.mark.parametrize("R", ROWS)
def test_du_only_on_randn(ops, R):
    for seed in range(5 if R == ROWS[-1] else 1):
        xh, dy, up, dn = randn_case(ops, R, 100 * seed)
        what = f"mlp du-only randn R={R} seed={seed}"
        t1, g, du = both_forms(ops, R, xh, dy, up, dn, RR.ACT_GELU, what)
        RR.check_exact(t1, dy, f"{what} t1")
        RR.check_mlp_bwd(g, du, xh, up["Wp"], up["bp"], dy, dn["WpT"], RR.ACT_GELU, what)


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("kind", ACTS)
def test_every_activation_with_and_without_dropout(ops, kind, dropout):
    R = 1000
    xh, dy, up, dn = randn_case(ops, R, 7)
    drop = None
    if dropout:
        rng = torch.zeros(2, dtype=torch.int32, device="cuda")
        ops.rng_seed(rng, 5)
        drop = ops.dropout(rng, 3, 0.25)
    what = f"mlp du-only act={kind} dropout={dropout}"
    t1, g, du = both_forms(ops, R, xh, dy, up, dn, kind, what, drop=drop)
    if dropout:         # t1 = dropout'(dy): zero where dropped, dy / 0.75 (rounded once) where kept, and some of each
        kept = t1 != 0
        assert 0.6 < float(kept.float().mean()) < 0.9 and bool((t1[~kept] == 0).all())
        RR.check_exact(t1[kept], (dy.float() / 0.75).to(BF)[kept], f"{what} t1 (kept)")
    else:
        RR.check_exact(t1, dy, f"{what} t1")
    if kind != L.MLP_GELU_TANH:          # (rowowner_refs states the three other activations; the tanh form is held to du's bit-identity alone)
        RR.check_mlp_bwd(g, du, xh, up["Wp"], up["bp"], t1, dn["WpT"], kind, what)


def test_argument_errors_launch_nothing(ops):
    R = 129
    xh, dy, up, dn = randn_case(ops, R, 3)
    kw = dict(w_up=up["Wp"], b_up=up["bp"], xhat=xh, dy=dy, w_down_t=dn["WpT"], act=L.MLP_GELU)
    rs = torch.ones(R, device="cuda")
    bufs = dict(t1=obuf(R, 256), g=obuf(R, 512), du=obuf(R, 512), dx=obuf(R, 256))
    cases = {"t1 alone NULL": dict(t1=None, g=bufs["g"], dx=None), "g alone NULL": dict(t1=bufs["t1"], g=None, dx=None),
             "NULLs with the one-launch kernel": dict(t1=None, g=None, dx=bufs["dx"], rstd=rs, w_up_t=up["WpTP"]),
             "t1 alone NULL, one launch": dict(t1=None, g=bufs["g"], dx=bufs["dx"], rstd=rs, w_up_t=up["WpTP"])}
    for what, args in cases.items():
        d = ops.mlp_desc(R, du=bufs["du"], **kw, **args)
        rc = L.lib().mmfm_mlp_bwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and b"mmfm_mlp_bwd" in L.lib().mmfm_last_error(), what
        with pytest.raises(L.MmfmError):
            ops.mlp_bwd(d)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        RR.assert_untouched(b, FILL, f"argument error: {k}")
