"""What EngineDDP all-reduces under a freeze pattern (ddp.trainable_spans): per bucket the span from its first to its last trainable
parameter, nothing for a bucket without one, today's buckets with everything trainable.  A pure function of the real ParamLayout of the
YAML model (channels 668 / 2) and the trainable names: no GPU."""
import fnmatch
import math

from helpers import model_config
from multi_modal_foundation_model_amd.ddp import GradBuckets, backward_order, trainable_spans
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout


def setup(bucket_bytes=2 << 20):
    cfg = EngineConfig.from_model_config(model_config(), [("ap", 668), ("behavior", 2)])
    lay = ParamLayout(cfg)
    return cfg, lay, GradBuckets(lay, cfg, bucket_bytes)


def end(lay, k):
    off, shape = lay.entries[k]
    return off + int(math.prod(shape))


def names_in(lay, lo, hi):
    return [k for k, (off, _) in lay.entries.items() if lo <= off < hi]


def test_all_trainable_gives_todays_buckets():
    cfg, lay, gb = setup()
    assert len(gb.buckets) >= 4
    spans = trainable_spans(lay, gb.buckets, list(lay.entries))
    assert spans == gb.trigger and list(spans) == [n for n, _, _ in gb.buckets]
    # the buckets tile the buffer back to front, so the spans do
    assert gb.buckets[0][2] == lay.segments[-1][2] and gb.buckets[-1][1] == 0
    assert all(a[1] == b[2] for a, b in zip(gb.buckets, gb.buckets[1:]))


def test_frozen_encoder_leaves_the_encoder_buckets_without_a_collective():
    cfg, lay, gb = setup()
    live = [k for k in lay.entries if not fnmatch.fnmatchcase(k, "encoder.*") and not fnmatch.fnmatchcase(k, "encoder_embeddings.*")]
    spans = trainable_spans(lay, gb.buckets, live)
    for name, lo, hi in gb.buckets:
        inside = [k for k in names_in(lay, lo, hi) if k in live]
        if not inside:
            assert spans[name] is None
        elif len(inside) == len(names_in(lay, lo, hi)):
            assert spans[name] == (lo, hi)
        else:
            assert spans[name] == (lay.entries[inside[0]][0], end(lay, inside[-1])) and lo <= spans[name][0] < spans[name][1] <= hi
    assert any(v is None for v in spans.values()) and any(v is not None and v != gb.trigger[n] for n, v in spans.items())
    # the last bucket (the tokenisers) keeps the decoder's tokenisers: its span starts behind the encoder's
    last = spans[gb.buckets[-1][0]]
    enc_tok_end = max(end(lay, k) for k in lay.entries if k.startswith("encoder_embeddings."))
    assert last is not None and last[0] >= enc_tok_end


def test_heads_only_issues_one_collective():
    cfg, lay, gb = setup()
    live = [k for k in lay.entries if fnmatch.fnmatchcase(k, "decoder_embeddings.*.out.*")]
    spans = trainable_spans(lay, gb.buckets, live)
    first = gb.buckets[0][0]
    assert [n for n, v in spans.items() if v is not None] == [first]
    assert spans[first] == (lay.entries[live[0]][0], end(lay, live[-1]))
    assert sum(b - a for a, b in (v for v in spans.values() if v)) == sum(int(math.prod(lay.entries[k][1])) for k in live) + \
        sum(lay.entries[b][0] - end(lay, a) for a, b in zip(live, live[1:]))          # (the padding between neighbours rides along)


def test_one_trainable_parameter_in_the_middle_of_a_bucket():
    cfg, lay, gb = setup()
    name, lo, hi = gb.buckets[1]
    inside = names_in(lay, lo, hi)
    k = inside[len(inside) // 2]
    spans = trainable_spans(lay, gb.buckets, [k])
    assert spans[name] == (lay.entries[k][0], end(lay, k)) and lo < spans[name][0] and spans[name][1] < hi
    assert all(v is None for n, v in spans.items() if n != name)
    assert list(spans) == [n for n in backward_order(lay, cfg) if n in gb.trigger]


def test_nothing_trainable_issues_nothing():
    cfg, lay, gb = setup()
    assert set(trainable_spans(lay, gb.buckets, []).values()) == {None}


# ------------------------------------------------------------------------------------------------ training.freeze / --freeze
def test_freeze_parameters_by_fnmatch_patterns():
    import pytest
    import torch
    from multi_modal_foundation_model_amd.optim import freeze_parameters

    class Wrapped(torch.nn.Module):                          # what a data-parallel wrapper looks like: the model under `.module`
        def __init__(self, m):
            super().__init__()
            self.module = m
    net = torch.nn.ModuleDict(dict(encoder=torch.nn.ModuleList([torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)]), head=torch.nn.Linear(2, 1)))
    assert freeze_parameters(net, None) == [] and freeze_parameters(net, []) == [] and all(p.requires_grad for p in net.parameters())
    assert freeze_parameters(Wrapped(net), ["encoder.1.*", "head.bias"]) == ["encoder.1.weight", "encoder.1.bias", "head.bias"]
    assert [k for k, p in net.named_parameters() if p.requires_grad] == ["encoder.0.weight", "encoder.0.bias", "head.weight"]
    with pytest.raises(ValueError, match="matches no parameter"):
        freeze_parameters(net, ["decoder.*"])


def test_entry_script_takes_freeze_patterns_and_the_config_key_is_optional():
    import train_multi_modal as tm
    from helpers import load_config
    assert tm.build_parser().parse_args([]).freeze is None
    assert tm.build_parser().parse_args(["--freeze", "encoder.*", "encoder_embeddings.*"]).freeze == ["encoder.*", "encoder_embeddings.*"]
    assert load_config().training.get("freeze", None) is None          # no key of the reference's YAML: absent = nothing frozen
