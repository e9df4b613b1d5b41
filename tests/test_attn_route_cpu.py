"""The attention route (attn_route in csrc/attention.hip, asked through mmfm_attn_family) against tests/golden/attn_route.json: the
answers of the chain of launchers the route replaced - mmfm_attn_fast_launch, mmfm_attn_long_launch, mmfm_attn_bf16_launch, each taking
or declining the call, and the fp32-compute kernels for what was left - recorded from a dry-run build of that chain over the grid of
tests/attn_route_grid.py: at the point where a launcher would launch it reported its family, where it would fail the error.  The
thinned grid is recorded again under each environment switch that moves the route.  No GPU: the route reads no tensor.

One place differs from the record, on purpose.  The old bf16 tiled BACKWARD asked only whether its own LDS fits, the forward whether
both do; at dh 128 the forward's need passes 160 KB first (L > 15,064 against 28,632), so there the forward ran the fp32-compute
tiled kernels and the backward the bf16 tiled ones, which draw another drop_p mask.  The route asks one question for both
directions: the backward follows the forward to the fp32-compute tiled kernels, whose backward does not fit at that length and
refuses.  `parent_split` pins those cases: bf16, dh 128, L = 22,496 and 22,528, backward, aligned gradients."""
import os
import subprocess
import sys

import pytest

import attn_route_grid as G
from conftest import ROOT, load_json
from multi_modal_foundation_model_amd import _lib as L, ops

SWITCHES = ["MMFM_ATTN_FAST=0", "MMFM_ATTN_LONG=0", "MMFM_ATTN_FORCE_TILED=1", "MMFM_ATTN_FORCE_TILED=2", "MMFM_ATTN_BWD_SINGLE=0"]


def parent_split(case):
    dtype, dh, Lq, Lk, flags, workspace, drop_p, grads_aligned, backward = case
    return dtype == L.BF16 and dh == 128 and Lq >= 22496 and grads_aligned and backward


def check_against_record(got, want, thin, forced_f32=False):
    cases = list(G.cases(thin))
    assert len(cases) == len(want) == len(got)
    split = 0
    for i, (case, g, w) in enumerate(zip(cases, got, want)):
        if parent_split(case) and not forced_f32:
            # the record's backward (bf16 tiled) left its forward's family (fp32-compute tiled); the route keeps the pair together
            assert (w, want[i - 1], g, got[i - 1]) == ("4", "6", "x", "6"), (case, w, g)
            split += 1
        else:
            assert g == w, f"{case}: family {g}, recorded {w}"
    return split


@pytest.fixture(scope="module")
def record():
    return load_json("attn_route.json")


@pytest.fixture(scope="module")
def codes():
    return G.codes()


def test_route_matches_the_recorded_chain(record, codes):
    assert check_against_record(codes, record["default"], thin=False) == 2 * 6 * 2 * 2      # lengths x flags x workspace x drop_p
    assert set(codes) == set("123456jx"), "the grid reaches every family, the single-pass backward and a refusal"


@pytest.mark.parametrize("switch", SWITCHES)
def test_route_matches_the_recorded_chain_under_a_switch(record, switch):
    """The switches are read once per process: a child process with the switch set prints the thinned grid's codes."""
    name, value = switch.split("=")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]), **{name: value})
    got = subprocess.run([sys.executable, G.__file__], env=env, check=True, capture_output=True, text=True).stdout.strip()
    forced_f32 = switch == "MMFM_ATTN_FORCE_TILED=2"                                        # no bf16 kernel runs: nothing was split
    assert check_against_record(got, record[switch], thin=True, forced_f32=forced_f32) == (0 if forced_f32 else 6 * 2 * 2)
    thin_default = G.codes(True)
    assert got != thin_default, f"{switch} moves no case of the thinned grid"


def test_forward_and_backward_share_a_family(codes):
    """Over the whole grid: the same family wherever the gradients are aligned (or a refusal of one direction: the fp32-compute tiled
    backward needs more LDS than its forward), and with drop_p on never two different families, aligned or not."""
    cases = list(G.cases())
    fam = lambda c: "3" if c == "j" else c
    pairs = 0
    for i in range(0, len(cases), 2):
        (fwd_case, f), (bwd_case, b) = (cases[i], codes[i]), (cases[i + 1], codes[i + 1])
        assert not fwd_case[-1] and bwd_case[-1] and fwd_case[:-1] == bwd_case[:-1]
        grads_aligned, drop_p = fwd_case[7], fwd_case[6]
        if grads_aligned or drop_p > 0:
            assert fam(b) == f or "x" in (f, b), f"{fwd_case[:-1]}: forward {f}, backward {b}"
            pairs += 1
        if grads_aligned and f != "x" and not (f == "6" and b == "x"):
            assert fam(b) == f, f"{fwd_case[:-1]}: forward {f}, backward {b}"
    assert pairs == len(cases) * 3 // 8


def test_keepbit_literal_points_dense(record):
    """The dense counterparts of test_dropout_refs_cpu.py::test_keepbit_literal_points_under_causal (bf16, workspace, drop_p 0.4, forward):
    the record is the authority, and says the dense dh-128 launches stay on the keep-bit kernels past 2656."""
    cases = {c: i for i, c in enumerate(G.cases())}
    keepbit = {}
    for dh, Ln in [(32, 200), (32, 264), (32, 204), (64, 600), (128, 200), (128, 2656), (128, 2664), (128, 204)]:
        case = (L.BF16, dh, Ln, Ln, 0, True, 0.4, True, False)
        want = record["default"][cases[case]]
        assert G.CHARS[ops.attn_family(G.desc(ops, L, *case[:-1]))] == want
        keepbit[(dh, Ln)] = want in "12"
    assert keepbit == {(32, 200): True, (32, 264): False, (32, 204): False, (64, 600): True, (128, 200): True, (128, 2656): True,
                       (128, 2664): True, (128, 204): False}


def test_attn_family_raises_where_the_launch_refuses():
    d = G.desc(ops, L, L.BF16, 64, 200, 200, 0, workspace=True, grads_aligned=False)
    assert ops.attn_family(d) == L.ATTN_FAMILY_KEEPBIT_LONG
    with pytest.raises(L.MmfmError, match="gradient tensors must be 16-byte aligned"):
        ops.attn_family(d, backward=True)
    d = G.desc(ops, L, L.BF16, 16, 72, 72, 0)
    assert ops.attn_family(d, backward=True) == L.ATTN_FAMILY_BF16 | L.ATTN_FAMILY_BWD_SINGLE
