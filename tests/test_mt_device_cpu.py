"""MT19937 on the device, the part that needs no GPU: the header / binding surface (MMFM_MT_DEVICE), ops.mt_plan's cut of [0, n), the
argument refusals of the three entries (they return before any HIP call) and the masker's host path on CPU tensors under either value
of MMFM_MASKER_DEVICE."""
import ctypes as C
import random
import re

import numpy as np
import pytest
import torch

import mt_device_refs as R
from multi_modal_foundation_model_amd import _lib as L, ops
from test_oracle_golden import default_masker_cfg

NAMES = {"mmfm_mt_workspace", "mmfm_mt_uniform", "mmfm_mt_bernoulli", "mmfm_mt_corrupt"}


def test_header_macro_and_exports():
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert re.search(r"^#define MMFM_MT_DEVICE 1$", src, flags=re.M) and re.search(r"^#define MMFM_VERSION 401$", src, flags=re.M)
    assert re.search(r"^#define MMFM_MT_MAX_STREAMS 1024$", src, flags=re.M) and L.MT_MAX_STREAMS == 1024
    names = NAMES | {"mmfm_mt_plan"}
    assert names <= set(L.header_symbols()) and names <= set(L._PROTOS)
    lib = L.lib()
    assert all(hasattr(lib, n) for n in names) and lib.mmfm_version() == 401


@pytest.mark.parametrize("n", [1, 623, 624, 625, 3 * 192, R.N_MID, R.N_BIG])
@pytest.mark.parametrize("streams", [None, 1, 2, 3, 8])
def test_plan_covers_every_output_exactly_once(n, streams):
    S, P = ops.mt_plan(n, streams)
    assert S >= 1 and P >= 1 and (streams is None or S == min(streams, -(-n // 624)))
    runs = [(s * P * 624, min(n, (s + 1) * P * 624)) for s in range(S)]
    runs = [(a, b) for a, b in runs if a < n]                        # trailing runs may be empty
    assert runs[0][0] == 0 and runs[-1][1] == n
    assert all(a < b for a, b in runs) and all(runs[i][1] == runs[i + 1][0] for i in range(len(runs) - 1))
    assert ops.mt_plan(n, streams) == (S, P), "a pure function"
    assert L.lib().mmfm_mt_workspace(n, 0 if streams is None else streams) >= S * (3 * 624 * 4 + 4)


def test_plan_s_own_choice():
    assert ops.mt_plan(1) == (1, 1) and ops.mt_plan(624 * 127) == (1, 127), "short requests step: one run"
    S, P = ops.mt_plan(R.N_BIG)
    assert S == 256 and S & (S - 1) == 0 and P >= 64, "one run per CU at the B = 1024 call"
    for bad in ((0, None), (5, -1), (5, L.MT_MAX_STREAMS + 1)):
        with pytest.raises(L.MmfmError, match="mmfm_mt_plan"):
            ops.mt_plan(*bad)
    assert L.lib().mmfm_mt_workspace(0, 0) < 0


def _err():
    return L.lib().mmfm_last_error()


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """Null pointers, consumed outside 0..624, p outside [0, 1] or NaN, n == 0, streams out of range, a short or misaligned workspace:
    -1 with the error text set.  The pointers are made-up addresses: a call that got past its checks would have to touch them."""
    lib = L.lib()
    st = (C.c_uint32 * 624)(*range(1, 625))
    sp, out, ws = C.addressof(st), 0x7000000, 0x7100000
    need = lib.mmfm_mt_workspace(1000, 0)
    uni = lambda state=sp, consumed=3, skip=0, n=1000, o=out, streams=0, w=ws, wb=need: lib.mmfm_mt_uniform(state, consumed, skip, n, o, streams, w, wb, None)
    ber = lambda state=sp, consumed=3, p=0.5, n=1000, o=out, w=ws, wb=need: lib.mmfm_mt_bernoulli(state, consumed, 0, n, p, o, 0, w, wb, None)
    cor = lambda state=sp, consumed=3, B=2, T=5, N=100, src=out, cm=out, sb=500, st_=100, sn=1, zr=0.5, rr=1.0, dst=out, streams=0, w=ws, wb=need: \
        lib.mmfm_mt_corrupt(state, consumed, B, T, N, src, cm, sb, st_, sn, zr, rr, dst, streams, w, wb, None)
    cases = [(uni, dict(state=None), b"null pointer"), (uni, dict(o=None), b"null pointer"), (uni, dict(w=None), b"null pointer"),
             (uni, dict(consumed=-1), b"outside 0..624"), (uni, dict(consumed=625), b"outside 0..624"), (uni, dict(n=0), b"out of range"),
             (uni, dict(streams=-1), b"streams"), (uni, dict(streams=L.MT_MAX_STREAMS + 1), b"streams"),
             (uni, dict(wb=need - 1), b"workspace"), (uni, dict(wb=0), b"workspace"), (uni, dict(w=ws + 4), b"16-byte"),
             (uni, dict(streams=8, n=624 * 100), b"workspace"),
             (ber, dict(p=-0.1), b"outside [0, 1]"), (ber, dict(p=1.5), b"outside [0, 1]"), (ber, dict(p=float("nan")), b"outside [0, 1]"),
             (ber, dict(state=None), b"null pointer"), (ber, dict(o=None), b"null pointer"), (ber, dict(consumed=700), b"outside 0..624"),
             (ber, dict(wb=16), b"workspace"),
             (cor, dict(state=None), b"null pointer"), (cor, dict(src=None), b"null pointer"), (cor, dict(cm=None), b"null pointer"),
             (cor, dict(dst=None), b"null pointer"), (cor, dict(w=None), b"null pointer"), (cor, dict(consumed=625), b"outside 0..624"),
             (cor, dict(B=0), b"bad shape"), (cor, dict(B=1 << 16, T=1 << 10, N=1 << 5), b"bad shape"), (cor, dict(sb=-1), b"negative mask stride"),
             (cor, dict(zr=1.01), b"outside [0, 1]"), (cor, dict(rr=float("nan")), b"outside [0, 1]"), (cor, dict(zr=-1.0), b"outside [0, 1]"),
             (cor, dict(wb=need - 1), b"workspace")]
    for fn, kw, msg in cases:
        assert fn(**kw) == -1 and msg in _err(), (kw, _err())
    assert list(st) == list(range(1, 625)), "the state array is only read"
    # the wrappers refuse what the library could not: a state that is not 624 CPU int32 words, a missing destination
    with pytest.raises(TypeError, match="624 words"):
        ops.mt_uniform(torch.zeros(623, dtype=torch.int32), 0, 10, device="cpu")
    with pytest.raises(ValueError, match="out"):
        ops.mt_uniform(torch.zeros(624, dtype=torch.int32), 0, 10)
    with pytest.raises(TypeError, match="device"):
        ops.mt_corrupt(torch.zeros(624, dtype=torch.int32), 0, torch.zeros(2, 3, 4), torch.zeros(2, 3, 1, dtype=torch.uint8), 0.5, 1.0)


def test_generator_position_is_what_the_jump_takes():
    from multi_modal_foundation_model_amd import rngjump
    torch.manual_seed(3)
    state, consumed = rngjump.cpu_generator_position()
    assert consumed == 624 and state.dtype == torch.int32 and state.numel() == 624, "freshly seeded: regenerate first"
    torch.rand(5)
    assert rngjump.cpu_generator_position()[1] == 5
    pos = R.position()
    assert pos[1] == 5 and torch.equal(pos[0], rngjump.cpu_generator_position()[0])
    g = torch.Generator().manual_seed(9)
    torch.rand(700, generator=g)
    assert rngjump.cpu_generator_position(g)[1] == 76


# ------------------------------------------------------------------------------------------------------ the masker's host path
B, T, N = 3, 8, 12
REGIONS = np.array([["CA1"] * 5 + ["PO"] * 4 + ["LP"] * 3] * B)
MODES = ["temporal", "random_token", "causal", "neuron", "inter-region", "intra-region", "co-smooth", "forward-pred", "random"]


def masker(mode, **kw):
    from models.masker import Masker
    from utils.config_utils import DictConfig
    cfg = default_masker_cfg(mode=mode, expand_prob=0.5, max_timespan=3, channels=[1, 4, 7], timesteps=[2, 5], **kw)
    return Masker(DictConfig(cfg))


def seeded(fn, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    out = fn()
    return out, torch.get_rng_state(), random.getstate()


@pytest.mark.parametrize("mode", MODES)
def test_cpu_tensors_take_the_host_lines_under_either_switch(mode, monkeypatch):
    """On CPU tensors MMFM_MASKER_DEVICE changes nothing: element_masks and forward give the bits of the host lines replayed from the
    generator position behind the mask draw (forward(token_mask_only=True) stops there), and the states of both generators."""
    x = torch.poisson(torch.full((B, T, N), 1.5), generator=torch.Generator().manual_seed(3))
    kw = dict(zero_ratio=0.5, random_ratio=1.0)
    for seed in (0, 5):
        def oracle():
            _, tmask = masker(mode, **kw)(x.clone(), REGIONS, token_mask_only=True)
            return tmask
        want_tm, _, want_r = seeded(oracle, seed)
        got = {}
        for switch in ("1", "0"):
            monkeypatch.setenv("MMFM_MASKER_DEVICE", switch)
            m = masker(mode, **kw)
            (cm, tm, corrupted), g, r = seeded(lambda: m.element_masks(x, REGIONS), seed)
            f = masker(mode, **kw)
            (sp, tmask), gf, rf = seeded(lambda: f(x.clone(), REGIONS), seed)
            assert m.device_draws == 0 and f.device_draws == 0, "no device path on a CPU tensor"
            assert torch.equal(tm.expand(B, T, N).to(torch.int64), want_tm) and torch.equal(tmask, want_tm)
            assert torch.equal(corrupted, sp) and torch.equal(g, gf) and r == rf == want_r
            got[switch] = (cm, tm, corrupted, g)
        assert all(torch.equal(a, b) for a, b in zip(got["1"], got["0"]))
        # the host lines themselves, from the position behind the mask draw
        seeded(oracle, seed)
        want, _, _ = R.host_corrupt(x, got["1"][0], 0.5, 1.0)
        assert torch.equal(got["1"][2], want) and torch.equal(got["1"][3], torch.get_rng_state())
    assert "_mt_ws" in m.__getstate__() and m.__getstate__()["_mt_ws"] == {} and m.__getstate__()["device_draws"] == 0
