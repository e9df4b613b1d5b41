"""The step plans are what they were: per row of the matrix in tests/plan_sig.py the plan the engine builds has the signature
recorded in tests/golden/plan_signatures.json (scripts/make_plan_goldens.py) - the same C functions in the same order with the same
arguments, descriptors and device tables, every pointer at the same offset of the same tensor.  A case builds a model and a plan and
launches no kernel of the step.  Runs on the MI355X only (an Engine allocates on the device)."""
import pytest

import plan_sig as S
from conftest import load_json

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.CASES, ids=[c["name"] for c in S.CASES])
def test_plan_signature_is_the_recorded_one(case, monkeypatch):
    for k in S.SWITCHES + S.AUTO:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    golden = load_json("plan_signatures.json")[case["name"]]
    eng, plan, _ = S.build_case(case)
    sig = S.plan_signature(eng, plan)
    assert list(sig) == list(golden), "the plan's units (forward, backward segments in order)"
    for unit, want in golden.items():
        assert sig[unit]["names"] == want["names"], f"{unit}: the launches differ"
        assert sig[unit]["sha256"] == want["sha256"], f"{unit}: same launches, other arguments (diff scripts/make_plan_goldens.py --full)"
