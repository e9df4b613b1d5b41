"""mmfm_adamw_step_ranges / mmfm_grad_sumsq_ranges on the GPU (include/mmfm.h, MMFM_OPTIM_RANGES).

The update is compared BIT FOR BIT with the existing mmfm_adamw_step run on each range's slice with that range's hyper vector, so no
tolerance is invented for it; the sums of squares are compared with the exactly rounded fp64 sum (math.fsum) within the bound that
holds for any summation order, (n - 1) 2^-53 relative (tests/optim_refs.py: sumsq_bound).

The buffer is the smallest that reaches every path: n = 3 * CHUNK + 37 floats with the ranges
    [0, 1)  [1, 8)  [8, CHUNK + 9)  - a gap, a frozen parameter -  [2 * CHUNK + 5, n)
so there are one-element and sub-quad ranges, a chunk boundary crossed at an odd offset (16-byte body, element-wise head and tail),
whole chunks, and more workgroups than one; alternating ranges use two hyper rows."""
import ctypes as C
import math

import pytest
import torch

import edge_refs as E
import optim_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CH = R.CHUNK
N = 3 * CH + 37
RANGES = [(0, 1, 0), (1, 8, 1), (8, CH + 9, 0), (2 * CH + 5, N, 1)]
GAP = (CH + 9, 2 * CH + 5)


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "mmfm_device_check")
    return K


def rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda") * scale


def state(with_bf16, seed=0):
    p, m, v = rnd(N, seed + 1), rnd(N, seed + 2, 0.01), rnd(N, seed + 3, 0.01).abs()
    return p, m, v, (p.to(BF16) if with_bf16 else None)


def hyper_rows(step):
    """Two groups as OneCycleLR leaves them at `step`: own lr, beta1, weight decay and (row 1) a grad_scale other than 1."""
    return [E.adamw_hyper(step, 1e-3 * step, 0.95 - 0.01 * step), E.adamw_hyper(step, 4e-3 / step, 0.85, wd=0.0, grad_scale=0.37)]


def dev_rows(rows):
    return torch.tensor(rows, dtype=torch.float64).to(F32).cuda()


def step_slices(ops, ranges, st, g, rows):
    """The existing kernel on each range's slice with that range's hyper vector."""
    p, m, v, pb = st
    for s, e, row in ranges:
        ops.adamw_step(p[s:e], g[s:e], m[s:e], v[s:e], None if pb is None else pb[s:e], e - s, dev_rows(rows[row]))


def raw(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def assert_same_bits(got, want, what):
    for name, a, b in zip(("p", "m", "v", "p_bf16"), got, want):
        if a is not None:
            E.check_exact(raw(a), raw(b), f"{what}: {name}")


def clone(st):
    return tuple(None if t is None else t.clone() for t in st)


@pytest.mark.parametrize("with_bf16", [False, True], ids=["fp32", "bf16copy"])
def test_ranges_step_equals_the_single_range_kernel_per_slice_and_leaves_the_gap(ops, with_bf16):
    tab = ops.OptimRanges(RANGES, N, 2, device="cuda")
    assert tab.n_chunks == 6
    got, want = state(with_bf16), state(with_bf16)
    before = clone(got)
    for step in (1, 2, 3):
        g = rnd(N, 100 + step, 0.1)
        g[GAP[0]:GAP[1]] = float("nan")                     # a frozen parameter's gradient is never needed
        rows = hyper_rows(step)
        ops.adamw_step_ranges(got[0], g, got[1], got[2], got[3], tab, dev_rows(rows))
        step_slices(ops, RANGES, want, g, rows)
        assert_same_bits(got, want, f"step {step}")
    for name, a, b in zip(("p", "m", "v", "p_bf16"), got, before):
        if a is not None:
            E.check_exact(raw(a)[GAP[0]:GAP[1]], raw(b)[GAP[0]:GAP[1]], f"gap: {name}")
            assert not torch.isnan(a.float()).any(), f"{name}: the gap's NaN gradient leaked"
            assert not torch.equal(raw(a)[:GAP[0]], raw(b)[:GAP[0]]) and not torch.equal(raw(a)[GAP[1]:], raw(b)[GAP[1]:])


@pytest.mark.parametrize("with_bf16", [False, True], ids=["fp32", "bf16copy"])
def test_one_range_over_the_whole_buffer_equals_one_adamw_step(ops, with_bf16):
    tab = ops.OptimRanges([(0, N, 0)], N, 1, device="cuda")
    got, want = state(with_bf16, seed=10), state(with_bf16, seed=10)
    for step in (1, 2, 3):
        g = rnd(N, 200 + step, 0.1)
        h = dev_rows([hyper_rows(step)[1]])
        ops.adamw_step_ranges(got[0], g, got[1], got[2], got[3], tab, h)
        ops.adamw_step(want[0], g, want[1], want[2], want[3], N, h)
        assert_same_bits(got, want, f"whole buffer, step {step}")


def test_unaligned_buffers_take_the_elementwise_path_with_the_same_bits(ops):
    """Views that start 4 bytes into an allocation: no 16-byte access is possible, the results do not change."""
    tab = ops.OptimRanges([(0, 5, 0), (7, CH + 3, 1)], N - 1, 2, device="cuda")
    got, want = state(True, seed=20), state(True, seed=20)
    g = rnd(N, 300, 0.1)
    rows = hyper_rows(2)
    ops.adamw_step_ranges(got[0][1:], g[1:], got[1][1:], got[2][1:], got[3][1:], tab, dev_rows(rows))
    step_slices(ops, [(1, 6, 0), (8, CH + 4, 1)], want, g, rows)
    assert_same_bits(got, want, "offset views")


def write_record(tab, clip_coef, nonfinite=0):
    from multi_modal_foundation_model_amd import _lib as L
    rec = L.OptimRecord(0.0, clip_coef, nonfinite, 0, tab.n_ranges, 0)
    tab.workspace[:C.sizeof(rec)].copy_(torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8))
    return C.c_float(clip_coef).value                       # the float the kernel will read back


@pytest.mark.parametrize("with_bf16", [False, True], ids=["fp32", "bf16copy"])
def test_clipped_step_is_the_plain_step_on_the_scaled_gradient(ops, with_bf16):
    """gi = (g * clip_coef) * grad_scale in that order: G' = G * c is one fp32 multiply by the float in the record, and row 1 has a
    grad_scale other than 1, so the other order would show."""
    tab = ops.OptimRanges(RANGES, N, 2, device="cuda")
    c = write_record(tab, 0.3141592)
    got, want = state(with_bf16, seed=30), state(with_bf16, seed=30)
    g = rnd(N, 400, 0.1)
    rows = hyper_rows(2)
    ops.adamw_step_ranges(got[0], g, got[1], got[2], got[3], tab, dev_rows(rows), clipped=True)
    step_slices(ops, RANGES, want, g * torch.tensor(c, dtype=F32, device="cuda"), rows)
    assert_same_bits(got, want, "clipped")
    assert not torch.equal(g * torch.tensor(c, device="cuda") * 0.37, g * 0.37 * torch.tensor(c, device="cuda")), \
        "the two multiply orders must differ somewhere for this check to mean anything"


SUMSQ_CASES = [pytest.param(1.0, 1.0, id="unit"), pytest.param(1.0, 0.37, id="unit, coef_in 0.37"), pytest.param(1e-20, 1.0, id="1e-20")]


@pytest.mark.parametrize("scale,coef_in", SUMSQ_CASES)
def test_sumsq_against_the_exact_fp64_sum(ops, scale, coef_in):
    tab = ops.OptimRanges(RANGES, N, 2, device="cuda")
    g = rnd(N, 500, 1.0) * scale
    g[GAP[0]:GAP[1]] = float("nan")
    x = (g * torch.tensor(coef_in, dtype=F32, device="cuda")).double().cpu().numpy()      # the fp32 product the update forms, exact in fp64
    want = [math.fsum((x[s:e] * x[s:e]).tolist()) for s, e, _ in RANGES]                    # squares exact in fp64, sums exactly rounded
    want_total = math.fsum(sq for s, e, _ in RANGES for sq in (x[s:e] * x[s:e]).tolist())
    base = math.sqrt(want_total) + 1e-6                     # clip_coef = max_norm / base below 1: one case on either side
    for max_norm in (0.5 * base, 2.0 * base, 0.0, float("inf")):
        ops.grad_sumsq_ranges(g, tab, coef_in=coef_in, max_norm=max_norm)
        first = tab.workspace.clone()
        rec = tab.record()
        ops.grad_sumsq_ranges(g, tab, coef_in=coef_in, max_norm=max_norm)
        assert torch.equal(tab.workspace, first), "two calls on the same inputs must give the same bits"
        assert rec["nonfinite"] == 0 and rec["skipped"] == 0
        for (s, e, _), got, w in zip(RANGES, rec["range_sumsq"], want):
            if max_norm == 0.0:
                print(f"[sumsq] scale {scale} range [{s}, {e}): rel err {abs(got - w) / w:.3e}, bound {R.sumsq_bound(e - s):.3e}")
            assert w > 0 and abs(got - w) <= R.sumsq_bound(e - s) * w
        n_terms = sum(e - s for s, e, _ in RANGES)
        if max_norm == 0.0:
            print(f"[sumsq] scale {scale} total: rel err {abs(rec['total'] - want_total) / want_total:.3e}, bound {R.sumsq_bound(n_terms):.3e}")
        assert abs(rec["total"] - want_total) <= R.sumsq_bound(n_terms) * want_total
        coef = R.clip_coef(rec["total"], max_norm)                                        # torch's formula on the device's own total
        assert abs(rec["clip_coef"] - coef) <= 2.0 ** -23 * coef
        assert (rec["clip_coef"] < 1.0) == (max_norm == 0.5 * base)
    # (scale 1e-20: the squares, about 1e-40, lie below fp32's smallest normal 1.2e-38 - an fp32 accumulation would lose them)


def test_sumsq_closing_phase_beyond_one_group_of_ranges_and_one_tile_of_partials(ops):
    """The closing launch walks the ranges in groups of 256 and stages a group's partials through LDS 512 at a time: 300 three-element
    ranges (two groups) followed by one range of 514 chunks (two tiles, the second one short) reach both loops and their seams."""
    small = [(4 * i, 4 * i + 3, i % 2) for i in range(300)]
    big = (1205, 1205 + 513 * CH)                           # starts and ends inside a chunk: 514 chunks
    ranges = small + [(big[0], big[1], 0)]
    n = big[1] + 11
    tab = ops.OptimRanges(ranges, n, 2, device="cuda")
    assert tab.n_ranges == 301 and tab.n_chunks == 300 + 514
    g = rnd(n, 700, 1.0)
    ops.grad_sumsq_ranges(g, tab, max_norm=1.0)
    first = tab.workspace.clone()
    rec = tab.record()
    ops.grad_sumsq_ranges(g, tab, max_norm=1.0)
    assert torch.equal(tab.workspace, first)
    x = g.double().cpu().numpy()
    sq = x * x
    for (s, e, _), got in zip(ranges, rec["range_sumsq"]):
        w = math.fsum(sq[s:e].tolist())
        assert abs(got - w) <= R.sumsq_bound(e - s) * w, (s, e)
    want_total = math.fsum(v for s, e, _ in ranges for v in sq[s:e].tolist())
    n_terms = sum(e - s for s, e, _ in ranges)
    print(f"[sumsq] 301 ranges / 814 chunks total: rel err {abs(rec['total'] - want_total) / want_total:.3e}, bound {R.sumsq_bound(n_terms):.3e}")
    assert abs(rec["total"] - want_total) <= R.sumsq_bound(n_terms) * want_total
    coef = R.clip_coef(rec["total"], 1.0)
    assert rec["nonfinite"] == 0 and abs(rec["clip_coef"] - coef) <= 2.0 ** -23 * coef and coef < 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_sets_the_flag_and_skips_only_when_asked(ops, bad):
    tab = ops.OptimRanges(RANGES, N, 2, device="cuda")
    g = rnd(N, 600, 0.1)
    g[CH + 3] = bad                                       # inside range 2, second chunk
    rows = hyper_rows(1)
    st = state(True, seed=40)
    before = clone(st)
    ops.grad_sumsq_ranges(g, tab, max_norm=1.0, skip_nonfinite=True)
    ops.adamw_step_ranges(st[0], g, st[1], st[2], st[3], tab, dev_rows(rows), clipped=True, skip_nonfinite=True)
    rec = tab.record()
    assert rec["nonfinite"] == 1 and rec["skipped"] == 1
    assert_same_bits(st, before, "skipped step")
    # not asked to skip: the flag is still set, nothing is counted, the update runs (with the coefficient the record holds)
    ops.grad_sumsq_ranges(g, tab, max_norm=0.0, skip_nonfinite=False)
    rec = tab.record()
    assert rec["nonfinite"] == 1 and rec["skipped"] == 1 and rec["clip_coef"] == 1.0
    ops.adamw_step_ranges(st[0], g, st[1], st[2], st[3], tab, dev_rows(rows), clipped=True, skip_nonfinite=False)
    want = clone(before)
    step_slices(ops, RANGES, want, g, rows)
    for a, b in zip(st, want):                            # the poisoned element: non-finite on both sides (a NaN's payload is not compared)
        assert not bool(torch.isfinite(a[CH + 3].float())) and not bool(torch.isfinite(b[CH + 3].float()))
        a[CH + 3], b[CH + 3] = 0, 0
    assert_same_bits(st, want, "update with a non-finite gradient, skipping off")
    assert not torch.equal(raw(st[0])[:8], raw(before[0])[:8])
