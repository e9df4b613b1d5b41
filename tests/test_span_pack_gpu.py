"""mmfm_span_gather / mmfm_span_scatter on the GPU, through the C ABI: copies, so every check is torch.equal against a reference built
by indexing - span lengths around the 16-byte quads and the 4096-element chunk, packed offsets that are and are not multiples of four
(the 16-byte path and the element path), dead spans full of NaN that must never be loaded, sentinels everywhere else, n_spans of 0 and
1, a table at full capacity with n_spans below it, the round trip, and a captured launch replayed with another table."""
import pytest
import torch

from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K

pytestmark = pytest.mark.gpu
LENS = (1, 3, 4, 7, 64, 65, 12 * 8, 1025)
SENT_G, SENT_S = -7.25, 3.5
CAP = 24                             # rows of the static table


def make_case(lens, aligned, dead=(), seed=0, gap=8):
    """G slots on multiples of 8 elements (the layout's alignment) with sentinels between them; packed offsets either rounded up to
    multiples of 4 (the 16-byte path) or a plain running sum started at 1 (the element path for most spans).  Returns the rows."""
    rows, g, s = [], 8, 0 if aligned else 1
    for i, n in enumerate(lens):
        rows.append((g, s, n, int(i not in dead)))
        g = (g + n + gap) // 8 * 8 + (8 if i % 3 == 0 else 0)
        s = (s + n + 3) // 4 * 4 if aligned else s + n
    return rows, g + 8, s + 5


def buffers(rows, gn, sn, seed=0):
    gen = torch.Generator().manual_seed(seed)
    G = torch.full((gn,), SENT_G)
    for g, _, n, live in rows:
        G[g:g + n] = torch.randn(n, generator=gen) if live else float("nan")
    return G.cuda(), torch.full((sn,), SENT_S).cuda()


def table_of(rows, G, stage, cap=CAP, fill=None):
    """The device table at capacity `cap`; rows beyond the spans hold `fill` (a span that would overwrite sentinels if it were read)."""
    t = torch.zeros(cap, 4, dtype=torch.int64) if fill is None else torch.tensor([fill] * cap, dtype=torch.int64)
    K.span_table(rows, G.numel(), stage.numel(), out=t)
    return t.cuda()


def gather_ref(rows, G, stage):
    out = stage.clone()
    for g, s, n, live in rows:
        out[s:s + n] = G[g:g + n] if live else 0.0
    return out


def scatter_ref(rows, stage, G):
    out = G.clone()
    for g, s, n, _ in rows:
        out[g:g + n] = stage[s:s + n]
    return out


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))       # bit for bit, NaN included


def call(fn, a, b, table, n):
    L.check(fn(a.data_ptr(), b.data_ptr(), table.data_ptr(), n, torch.cuda.current_stream().cuda_stream), fn.__name__)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dead", [(), (1, 4, 7), tuple(range(8))])
def test_gather_and_scatter_against_indexing(aligned, dead):
    lib = L.lib()
    rows, gn, sn = make_case(LENS, aligned, dead)
    assert aligned == all(r[1] % 4 == 0 for r in rows)
    G, stage = buffers(rows, gn, sn)
    tab = table_of(rows, G, stage, fill=(0, sn - 4, 4, 1))       # n_spans below the capacity: a row beyond it would move sentinels
    want = gather_ref(rows, G, stage)
    G0 = G.clone()
    call(lib.mmfm_span_gather, G, stage, tab, len(rows))
    torch.cuda.synchronize()
    assert same(stage, want) and same(G, G0)
    assert not torch.isnan(stage).any()                          # dead spans were never loaded: zeros, not NaN * 0
    inside = torch.zeros(sn, dtype=torch.bool)
    for _, s, n, _ in rows:
        inside[s:s + n] = True
    assert bool((stage.cpu()[~inside] == SENT_S).all())          # every byte outside the ranges is still the sentinel
    # the copy back, for every span (dead ones included: they now hold zeros)
    stage2 = torch.randn(sn, generator=torch.Generator().manual_seed(5)).cuda()
    want_g = scatter_ref(rows, stage2, G)
    call(lib.mmfm_span_scatter, stage2, G, tab, len(rows))
    torch.cuda.synchronize()
    assert same(G, want_g)
    outside = torch.ones(gn, dtype=torch.bool)
    for g, _, n, _ in rows:
        outside[g:g + n] = False
    assert same(G.cpu()[outside], G0.cpu()[outside]) and bool((G.cpu()[outside] == SENT_G).all())


def test_round_trip_is_identity_on_live_and_zero_on_dead():
    rows, gn, sn = make_case(LENS + (4097, 9000), True, dead=(2, 8))
    G, stage = buffers(rows, gn, sn)
    tab = table_of(rows, G, stage)
    G0 = G.clone()
    K.span_gather(G, stage, tab, len(rows))
    K.span_scatter(stage, G, tab, len(rows))
    torch.cuda.synchronize()
    for g, _, n, live in rows:
        assert same(G[g:g + n], G0[g:g + n]) if live else bool((G[g:g + n] == 0).all())
    keep = torch.ones(gn, dtype=torch.bool)
    for g, _, n, _ in rows:
        keep[g:g + n] = False
    assert bool((G.cpu()[keep] == SENT_G).all())


@pytest.mark.parametrize("n_spans", [0, 1])
def test_few_spans(n_spans):
    rows, gn, sn = make_case(LENS, False)
    G, stage = buffers(rows, gn, sn)
    tab = table_of(rows, G, stage)
    want = gather_ref(rows[:n_spans], G, stage)
    K.span_gather(G, stage, tab, n_spans)
    torch.cuda.synchronize()
    assert same(stage, want)
    assert n_spans or bool((stage == SENT_S).all())


def test_many_chunks_of_one_span_and_many_short_spans():
    """More (span, chunk) pairs than workgroups: one span of 1100 chunks among 300 short ones."""
    lens = tuple(5 + (i % 9) for i in range(150)) + (1100 * L.SPAN_CHUNK + 3,) + tuple(1 + (i % 5) for i in range(150))
    rows, gn, sn = make_case(lens, True, dead=(7, 200))
    G, stage = buffers(rows, gn, sn)
    tab = table_of(rows, G, stage, cap=len(rows))
    want = gather_ref(rows, G, stage)
    K.span_gather(G, stage, tab, len(rows))
    torch.cuda.synchronize()
    assert same(stage, want)


def test_captured_launch_replayed_with_another_table():
    rows_a, gn, sn = make_case(LENS, True, dead=(1,))
    rows_b, gn_b, sn_b = make_case(LENS[::-1], False, dead=(5,))
    gn, sn = max(gn, gn_b), max(sn, sn_b)
    G, stage = buffers(rows_a, gn, sn)
    tab = table_of(rows_a, G, stage)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.span_gather(G, stage, tab, len(rows_a))                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.span_gather(G, stage, tab, len(rows_a))
    stage.fill_(SENT_S)
    graph.replay()
    torch.cuda.synchronize()
    assert same(stage, gather_ref(rows_a, G, torch.full_like(stage, SENT_S)))
    # another table in the same static buffer: other offsets (the element path now), other lengths per row, another dead span
    G2 = torch.full((gn,), SENT_G)
    gen = torch.Generator().manual_seed(9)
    for g, _, n, live in rows_b:
        G2[g:g + n] = torch.randn(n, generator=gen) if live else float("nan")
    G.copy_(G2.cuda())
    tab.copy_(table_of(rows_b, G, stage))
    stage.fill_(SENT_S)
    graph.replay()
    torch.cuda.synchronize()
    assert same(stage, gather_ref(rows_b, G, torch.full_like(stage, SENT_S)))


def test_refusals_launch_nothing():
    lib = L.lib()
    G, stage = torch.zeros(16).cuda(), torch.zeros(16).cuda()
    tab = torch.zeros(2, 4, dtype=torch.int64).cuda()
    for fn in (lib.mmfm_span_gather, lib.mmfm_span_scatter):
        assert fn(None, stage.data_ptr(), tab.data_ptr(), 1, None) == -1
        assert fn(G.data_ptr(), stage.data_ptr(), tab.data_ptr(), -1, None) == -1
        assert fn(G.data_ptr(), stage.data_ptr(), tab.data_ptr(), L.SPAN_MAX + 1, None) == -1
        assert b"n_spans" in lib.mmfm_last_error()
    with pytest.raises(ValueError):
        K.span_table([(0, 0, 17, 1)], 16, 32)                    # leaves G
    with pytest.raises(ValueError):
        K.span_table([(0, 0, 8, 1), (8, 4, 8, 1)], 16, 32)       # overlap in the staging buffer
