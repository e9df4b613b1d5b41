"""The GEMM route (gemm_route in csrc/gemm.hip, asked through mmfm_gemm_family and mmfm_gemm_pair_fused) against
tests/golden/gemm_route.json: the answers of the chain of launchers the route replaced - mmfm_gemm_big_launch and mmfm_gemm_dw_launch
each taking or declining the call, the 128-tile kernel for what was left, mmfm_gemm_dw_pair_launch in front of two mmfm_gemm calls -
recorded from a dry-run build of that chain over the grid of tests/gemm_route_grid.py: at the point where a launcher would launch (or
opt in to its LDS) it reported its kernel, where it would fail the error.  The thinned grid and the pairs are recorded again under
each environment switch that moves the route.  No GPU: the route reads no tensor.  The route equals the record everywhere."""
import os
import subprocess
import sys

import pytest

import gemm_route_grid as G
from conftest import ROOT, load_json
from multi_modal_foundation_model_amd import _lib as L, ops

SWITCHES = ["MMFM_GEMM_BIG=0", "MMFM_GEMM_DW=0", "MMFM_GEMM_BIG_KMIN=1024", "MMFM_GEMM_BIG_MIN_TILES=1", "MMFM_GEMM_DW_TN=128", "MMFM_GEMM_DW_TN=256"]
BIG, DW = str(L.GEMM_FAMILY_BIG256), (str(L.GEMM_FAMILY_DW128), str(L.GEMM_FAMILY_DW256))


def assert_equal_codes(got, want, cases):
    cases = list(cases)
    assert len(cases) == len(want) == len(got)
    for case, g, w in zip(cases, got, want):
        assert g == w, f"{case}: answer {g}, recorded {w}"


@pytest.fixture(scope="module")
def record():
    return load_json("gemm_route.json")


def under_switch(switch):
    """The switches are read once per process: a child process with the switch set prints the thinned grid's and the pairs' codes."""
    name, value = switch.split("=")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]), **{name: value})
    return subprocess.run([sys.executable, G.__file__], env=env, check=True, capture_output=True, text=True).stdout.split()


def test_route_matches_the_recorded_chain(record):
    codes = G.codes()
    assert_equal_codes(codes, record["default"]["grid"], G.cases())
    assert set(codes) == set("12345x"), "the grid reaches all five families and a refusal"
    pairs = G.pair_codes()
    assert_equal_codes(pairs, record["default"]["pairs"], G.pair_cases())
    assert set(pairs) == set("01x")


@pytest.mark.parametrize("switch", SWITCHES)
def test_route_matches_the_recorded_chain_under_a_switch(record, switch):
    grid, pairs = under_switch(switch)
    assert_equal_codes(grid, record[switch]["grid"], G.cases(thin=True))
    assert_equal_codes(pairs, record[switch]["pairs"], G.pair_cases())
    thin_default = G.codes(thin=True)
    assert grid != thin_default, f"{switch} moves no case of the thinned grid"
    # the two predicates are disjoint, so their order in the route decides nothing: with one of them off, what it took does not go to the other
    if switch in ("MMFM_GEMM_BIG=0", "MMFM_GEMM_DW=0"):
        for case, was, now in zip(G.cases(thin=True), thin_default, grid):
            assert not (was == BIG and now in DW) and not (was in DW and now == BIG), f"{case}: {was} -> {now} under {switch}"


def test_the_thinned_grid_is_the_full_grids_bf16_cases_without_a_record(record):
    full = [c for s, c in zip(G.cases(), record["default"]["grid"]) if s["dtype"] == G.BF16 and not s["live"]]
    assert "".join(full) == G.codes(thin=True)


def test_gemm_family_raises_where_mmfm_gemm_refuses():
    spec = dict(G.AXES[0], **G.BASES["dw"])
    assert (spec["dtype"], spec["live"], spec["c_f32"], spec["splits"]) == (G.BF16, 0, 0, 1)
    d, _ = G.desc(L, dict(spec, c_f32=1))
    assert ops.gemm_family(d) == L.GEMM_FAMILY_DW128 and ops.gemm_pair_fused(d, d) is False
    d, _ = G.desc(L, dict(spec, ak=0, bk=1))
    with pytest.raises(L.MmfmError, match="is not built"):
        ops.gemm_family(d)
    with pytest.raises(L.MmfmError, match="is not built"):
        ops.gemm_pair_fused(d, d)
    d, live = G.desc(L, dict(spec, live=1, dtype=G.F32))
    assert ops.gemm_family(d) == L.GEMM_FAMILY_F32
    with pytest.raises(L.MmfmError, match="mmfm_gemm_live: bf16 only"):
        ops.gemm_family(d, live)
