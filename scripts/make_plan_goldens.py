#!/usr/bin/env python3
"""Record the plan signatures of the matrix in tests/plan_sig.py (CASES) into tests/golden/plan_signatures.json.

    python scripts/make_plan_goldens.py [--out FILE] [--full DIR]
    python scripts/make_plan_goldens.py --layout          (no GPU: tests/golden/param_layout.json, the pinned ParamLayouts)

Needs the MI355X (an Engine allocates its buffers on the device) but runs no forward and no kernel of the step: per row it builds the
model, calls `model.engine()` and `engine._plan(B, T, training, grad)` under the row's MMFM_* switches (set and restored per row, the
other plan-time switches and the size-chosen paths' overrides, plan_sig.AUTO, cleared) and hashes what the plan would launch (tests/plan_sig.py).  --full DIR also writes every record of
every row to DIR/<row>.json for diffing two builds; those files are never committed.

The committed file is what the plan builder launched BEFORE a change.  A pull request that means to change a launch regenerates it
and says which rows changed; one that does not must reproduce it byte for byte (tests/test_plan_identity_gpu.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import plan_sig as S  # noqa: E402  (tests/plan_sig.py; its helpers import puts the API mirror on sys.path)


def with_switches(env, fn):
    saved = {k: os.environ.pop(k, None) for k in S.SWITCHES + S.AUTO}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in S.SWITCHES + S.AUTO:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def dump(sigs):
    """One line per unit: the file stays diffable row by row."""
    rows = []
    for name, units in sigs.items():
        lines = ",\n".join(f"  {json.dumps(u)}: {json.dumps(v, separators=(',', ':'))}" for u, v in units.items())
        rows.append(f" {json.dumps(name)}: {{\n{lines}\n }}")
    return "{\n" + ",\n".join(rows) + "\n}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_signatures.json"))
    ap.add_argument("--full", default=None, metavar="DIR")
    ap.add_argument("--layout", action="store_true", help="record the pinned parameter layouts instead (CPU)")
    args = ap.parse_args()
    if args.layout:
        out = os.path.join(ROOT, "tests", "golden", "param_layout.json")
        with open(out, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(S.layout_record(sw), separators=(',', ':'))}"
                                        for k, sw in S.LAYOUTS.items()) + "\n}\n")
        print(f"wrote {out}")
        return
    sigs = {}
    for case in S.CASES:
        def one():
            torch.cuda.reset_peak_memory_stats()
            eng, plan, secs = S.build_case(case)
            return S.plan_signature(eng, plan, full=args.full is not None), secs, torch.cuda.max_memory_allocated()
        sig, secs, nbytes = with_switches(case["env"], one)
        if args.full:
            os.makedirs(args.full, exist_ok=True)
            with open(os.path.join(args.full, case["name"] + ".json"), "w") as f:
                json.dump(sig, f, indent=1, sort_keys=True)
        sigs[case["name"]] = {u: dict(sha256=v["sha256"], names=v["names"]) for u, v in sig.items()}
        print(f"{case['name']}: {sum(len(v['names']) for v in sig.values())} launches, plan built in {secs * 1e3:.1f} ms, "
              f"{nbytes / 2 ** 30:.2f} GiB allocated", flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write(dump(sigs))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
