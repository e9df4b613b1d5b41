"""The per-session linear kernels through the C ABI (mmfm_session_reduce / _expand / _dw), fp32 and bf16, against the fp64
references of tests/session_stitch.py: exact-integer cases bit for bit, random cases inside the derived bounds of tests/edge_refs.py,
padding that is never read, spans of absent sessions that keep every byte, repeatability, row permutation and graph replay over
another mix of the same batch shape.  Runs on the MI355X only."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_refs as E
import session_stitch as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
SHAPES = [pytest.param(s, id="B{}T{}P{}N{}".format(*s[:4])) for s in R.SHAPES]
SENTINELS = (float("nan"), -7.25, 3.0e38, float("nan"), 0.5)       # the pattern the gradient buffers and the slabs start from


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def lib():
    from multi_modal_foundation_model_amd import _lib as L
    return L


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def draw(shape, seed, dtype, integer, lim):
    """integer: whole numbers in [-lim, lim] (exact in bf16, and so is every product and every sum of them in fp32); else N(0, 1)."""
    if integer:
        return torch.randint(-lim, lim + 1, shape, generator=gen(seed), device="cuda").to(dtype)
    return torch.randn(shape, generator=gen(seed), device="cuda").to(dtype)


def sentinel(n):
    return torch.tensor(SENTINELS, device="cuda").repeat(n // len(SENTINELS) + 1)[:n].contiguous()


class Case:
    """One batch shape with its session tables on the device.  The flat weight buffer holds NaN between the sessions' slots; every
    session's weights are drawn once, whatever the mix, so that two mixes of one shape share them."""

    def __init__(self, ops, shape, dtype, integer, bias_is_n, pad=float("nan"), ld_extra=0):
        self.K, self.dtype, self.integer, self.bias_is_n = ops, dtype, integer, bias_is_n
        self.B, self.T, self.P, self.N_max, base = shape
        self.n_base = len(base)
        self.sizes = R.session_sizes(self.B, base)
        self.S = len(self.sizes)
        self.ld = self.N_max + ld_extra
        self.w_off, self.b_off, self.w_elems, self.b_elems = R.layout(self.sizes, self.P, bias_is_n)
        self.W = [draw((n, self.P), 100 + k, dtype, integer, 2) for k, n in enumerate(self.sizes)]
        self.bias = [draw((n if bias_is_n else self.P,), 200 + k, F32, integer, 2) for k, n in enumerate(self.sizes)]
        self.w_flat = torch.full((self.w_elems,), float("nan"), device="cuda", dtype=dtype)
        self.b_flat = torch.full((self.b_elems,), float("nan"), device="cuda")
        for k, n in enumerate(self.sizes):
            self.w_flat[self.w_off[k]:self.w_off[k] + n * self.P] = self.W[k].reshape(-1)
            self.b_flat[self.b_off[k]:self.b_off[k] + self.bias[k].numel()] = self.bias[k]
        self.n_dev = torch.tensor(self.sizes, dtype=torch.int32, device="cuda")
        self.w_off_dev = torch.tensor(self.w_off, dtype=torch.int64, device="cuda")
        self.b_off_dev = torch.tensor(self.b_off, dtype=torch.int64, device="cuda")
        self.sid_dev = torch.zeros(self.B, dtype=torch.int32, device="cuda")
        self.pad = pad
        # the padded-side and the P-side operands: drawn once for the shape; the padding of the first is rewritten per mix
        self.x_live = draw((self.B, self.T, self.N_max), 1, dtype, integer, 3)
        self.q = draw((self.B, self.T, self.P), 2, dtype, integer, 3)
        self.x_pad = torch.full((self.B, self.T, self.ld), float("nan"), device="cuda", dtype=dtype)

    def set_mix(self, sid, chunk=None):
        """Overwrites the device tables and the padded operand IN PLACE for another mix (what load_inputs does for a captured plan)."""
        self.sid = list(sid)
        self.sid_dev.copy_(torch.tensor(self.sid, dtype=torch.int32))
        n_b = torch.tensor([self.sizes[k] for k in self.sid], device="cuda")
        live = torch.arange(self.ld, device="cuda")[None, None, :] < n_b[:, None, None]
        xl = torch.nn.functional.pad(self.x_live, (0, self.ld - self.N_max))
        self.x_pad.copy_(torch.where(live, xl, torch.full_like(xl, self.pad)))
        self.chunk = self.K.session_dw_chunk(self.B) if chunk is None else chunk
        runs = torch.from_numpy(self.K.session_runs(self.sid, self.S, self.chunk)).cuda()
        if getattr(self, "runs", None) is not None and self.runs.numel() == runs.numel():
            self.runs.copy_(runs)
        else:
            self.runs = runs
        return self

    def desc(self, bias=True, for_dw=False, ld_p=None):
        L = lib()
        return self.K.session_desc(L.BF16 if self.dtype == BF16 else L.F32, self.B, self.T, self.P, self.N_max, self.S, self.sid_dev, self.n_dev,
                                   self.w_off_dev, ld_pad=self.ld, ld_p=ld_p, b_off=self.b_off_dev, w=None if for_dw else self.w_flat, w_elems=self.w_elems,
                                   bias=self.b_flat if bias and not for_dw else None, b_elems=self.b_elems)

    # the three launches, each into buffers that start from the sentinel pattern / NaN
    def reduce(self, bias=True, out=None, plan=None):
        y = torch.full((self.B, self.T, self.P), float("nan"), device="cuda", dtype=self.dtype) if out is None else out
        self.K.session_reduce(self.desc(bias), self.x_pad, y, plan=plan)
        return y

    def expand(self, bias=True, out=None, plan=None):
        y = torch.full((self.B, self.T, self.ld), -5.0, device="cuda", dtype=self.dtype) if out is None else out
        self.K.session_expand(self.desc(bias), self.q, y, plan=plan)
        return y

    def dw(self, with_db=True, out=None, ws=None, plan=None):
        dw, db = (sentinel(self.w_elems), sentinel(self.b_elems)) if out is None else out
        if ws is None:
            ws = self.K.session_dw_workspace(self.B, self.P, self.N_max, self.S, self.chunk, "cuda")
            ws.copy_(sentinel(ws.numel()))                   # nothing may depend on what the slabs held
        self.K.session_dw(self.desc(for_dw=True), self.x_pad, self.q, self.runs, self.chunk, dw, db if with_db else None, self.bias_is_n, ws, plan=plan)
        return dw, db

    def x(self):
        return self.x_pad[:, :, :self.N_max]


def check_out(out, ref, sum_abs, n, what, exact):
    if exact:
        E.check_exact(out, ref.to(out.dtype), what)
    elif out.dtype == BF16:
        E.check_bf16(out, ref, n * E.U32 * sum_abs, what)
    else:
        E.check_sum(out, ref, n, sum_abs, what)


def check_grads(c, dw, db, exact, what):
    """Present sessions: every element of their spans against the reference.  Everything else - the spans of absent sessions and the
    gaps between the slots - keeps every byte of the sentinel pattern."""
    ref = R.dw_ref(c.x(), c.q, c.sid, c.sizes)
    keep_w, keep_b = np.ones(c.w_elems, dtype=bool), np.ones(c.b_elems, dtype=bool)
    for k, r in ref.items():
        n = c.sizes[k]
        got = dw[c.w_off[k]:c.w_off[k] + n * c.P].view(n, c.P)
        keep_w[c.w_off[k]:c.w_off[k] + n * c.P] = False
        check_out(got, r["dW"], r["abs_W"], r["bound_n"], f"{what}: dW of session {k}", exact)
        if db is not None:
            key, m = ("a", n) if c.bias_is_n else ("q", c.P)
            keep_b[c.b_off[k]:c.b_off[k] + m] = False
            check_out(db[c.b_off[k]:c.b_off[k] + m], r["db_" + key], r["abs_" + key], r["bound_n"], f"{what}: db of session {k}", exact)
    for buf, keep, name in ((dw, keep_w, "dW"), (db, keep_b, "db")):
        if buf is None:
            continue
        want = sentinel(buf.numel()).view(torch.int32).cpu().numpy()
        got = buf.view(torch.int32).cpu().numpy()
        assert np.array_equal(got[keep], want[keep]), f"{what}: {name} written outside the spans of the sessions of this batch"
        if name == "dW":
            assert keep.sum() > 0


# ------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("integer", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("mixname", R.MIXES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_kernels(ops, shape, dtype, mixname, integer):
    """reduce (with and without a bias) and expand: integers bit for bit, random data inside the derived bounds; the padding holds NaN
    throughout, so every output must be finite, and expand's zeros beyond n_s exact."""
    c = Case(ops, shape, dtype, integer, bias_is_n=False, ld_extra=3)
    c.set_mix(R.mix(mixname, c.B, c.n_base))
    for bias in (True, False):
        y = c.reduce(bias)
        ref, sa, n = R.reduce_ref(c.x(), c.sid, c.sizes, c.W, c.bias if bias else None)
        check_out(y, ref, sa, n, f"reduce bias={bias}", integer)
    c = Case(ops, shape, dtype, integer, bias_is_n=True, ld_extra=3)
    c.set_mix(R.mix(mixname, c.B, c.n_base))
    y = c.expand()
    ref, sa, n = R.expand_ref(c.q, c.sid, c.sizes, c.W, c.bias, c.N_max)
    check_out(y[:, :, :c.N_max].contiguous(), ref, sa, n, "expand", integer)
    for b, k in enumerate(c.sid):
        assert bool((y[b, :, c.sizes[k]:c.N_max] == 0).all()) and not bool(torch.signbit(y[b, :, c.sizes[k]:c.N_max].float()).any()), "expand: padding not +0"
    assert bool((y[:, :, c.N_max:] == -5.0).all()), "expand wrote beyond N_max"


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("integer", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("bias_is_n", [False, True], ids=["db_q", "db_a"])
@pytest.mark.parametrize("mixname", R.MIXES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(ops, shape, dtype, mixname, bias_is_n, integer, chunk):
    """dW and both bias-gradient forms, direct writes (one chunk) and slab sums (several); gradient buffers, gaps and slabs start from a
    sentinel pattern with NaN in it: present sessions are fully overwritten, everything else keeps every byte."""
    c = Case(ops, shape, dtype, integer, bias_is_n=bias_is_n).set_mix(R.mix(mixname, shape[0], len(shape[4])), chunk=chunk)
    dw, db = c.dw()
    check_grads(c, dw, db, integer, f"chunk {chunk}")
    dw2, db2 = c.dw(with_db=False)
    check_grads(c, dw2, None, integer, "no bias gradient")
    assert torch.equal(dw2.view(torch.int32), dw.view(torch.int32)) and torch.equal(db2.view(torch.int32), sentinel(c.b_elems).view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_stride_of_the_p_side(ops, dtype):
    """ld_p > P: reduce writes columns [0, P) of its rows and nothing else; expand and dw read theirs from rows of that pitch."""
    c = Case(ops, R.SHAPES[0], dtype, True, bias_is_n=True).set_mix(R.mix("interleaved", 5, 3), chunk=2)
    ld = c.P + 5
    y = torch.full((c.B, c.T, ld), -5.0, device="cuda", dtype=dtype)
    ops.session_reduce(c.desc(bias=False, ld_p=ld), c.x_pad, y)          # (this Case's biases are the read-out's, [n_k]: none for reduce)
    assert torch.equal(y[..., :c.P], c.reduce(bias=False)) and bool((y[..., c.P:] == -5.0).all())
    qw = torch.full((c.B, c.T, ld), float("nan"), device="cuda", dtype=dtype)
    qw[..., :c.P] = c.q
    yp = torch.full((c.B, c.T, c.ld), -5.0, device="cuda", dtype=dtype)
    ops.session_expand(c.desc(ld_p=ld), qw, yp)
    assert torch.equal(yp, c.expand())
    dw, db = sentinel(c.w_elems), sentinel(c.b_elems)
    ws = ops.session_dw_workspace(c.B, c.P, c.N_max, c.S, c.chunk, "cuda")
    ops.session_dw(c.desc(for_dw=True, ld_p=ld), c.x_pad, qw, c.runs, c.chunk, dw, db, True, ws)
    want = c.dw()
    assert torch.equal(dw.view(torch.int32), want[0].view(torch.int32)) and torch.equal(db.view(torch.int32), want[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pad_values_are_never_read(ops, shape, dtype):
    """The padded operand filled with 0, -1, 1e30 and NaN beyond n_s: the same bits out of all three kernels."""
    outs = []
    for pad in (0.0, -1.0, 1e30, float("nan")):
        c = Case(ops, shape, dtype, False, bias_is_n=True, pad=pad).set_mix(R.mix("interleaved", shape[0], len(shape[4])))
        y, (dw, db) = c.reduce(bias=False), c.dw()
        assert bool(torch.isfinite(y.float()).all())
        outs.append((y, dw, db))
    for y, dw, db in outs[1:]:
        for a, b in ((y, outs[0][0]), (dw, outs[0][1]), (db, outs[0][2])):
            assert torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32), b.view(torch.int16 if b.dtype == BF16 else torch.int32))


# ------------------------------------------------------------------------------------------------- repeatability
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_same_bits_twice_and_rows_follow_a_permutation(ops, shape, dtype):
    c = Case(ops, shape, dtype, False, bias_is_n=True).set_mix(R.mix("interleaved", shape[0], len(shape[4])), chunk=2)
    first = (c.reduce(bias=False), c.expand(), *c.dw())
    again = (c.reduce(bias=False), c.expand(), *c.dw())
    for a, b in zip(first, again):
        assert torch.equal(bits(a), bits(b))
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(5)).tolist()
    p = Case(ops, shape, dtype, False, bias_is_n=True)
    p.x_live, p.q = c.x_live[perm].contiguous(), c.q[perm].contiguous()
    p.set_mix([c.sid[i] for i in perm], chunk=2)
    assert torch.equal(bits(p.reduce(bias=False)), bits(first[0][perm]))
    assert torch.equal(bits(p.expand()), bits(first[1][perm]))


# ------------------------------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_graph_replay_serves_another_mix(ops, shape, dtype):
    """The three launches captured once under one mix; tables and inputs overwritten in place with another mix of the same batch shape;
    the replay equals eager launches of that mix bit for bit."""
    c = Case(ops, shape, dtype, False, bias_is_n=True).set_mix(R.mix("one", shape[0], len(shape[4])), chunk=2)
    y = torch.zeros(c.B, c.T, c.P, device="cuda", dtype=dtype)
    yp = torch.zeros(c.B, c.T, c.ld, device="cuda", dtype=dtype)
    grads = (sentinel(c.w_elems), sentinel(c.b_elems))
    ws = ops.session_dw_workspace(c.B, c.P, c.N_max, c.S, c.chunk, "cuda")
    plan = []
    c.reduce(bias=False, out=y, plan=plan), c.expand(out=yp, plan=plan), c.dw(out=grads, ws=ws, plan=plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.run_plan(plan)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.run_plan(plan)
    for name in ("interleaved", "distinct", "absent"):
        c.set_mix(R.mix(name, c.B, c.n_base), chunk=2)
        grads[0].copy_(sentinel(c.w_elems)), grads[1].copy_(sentinel(c.b_elems))
        graph.replay()
        torch.cuda.synchronize()
        eager = (c.reduce(bias=False), c.expand(), *c.dw())
        for a, b in zip((y, yp, *grads), eager):
            assert torch.equal(bits(a), bits(b)), name


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("case", list(R.BAD_DESC) + list(R.BAD_FWD))
def test_bad_arguments_return_before_any_launch(ops, case):
    L = lib()
    kw, msg = (R.BAD_DESC.get(case) or R.BAD_FWD[case])
    d = R.fake_desc(L, **kw)
    for fn in (L.lib().mmfm_session_reduce, L.lib().mmfm_session_expand):
        assert fn(C.byref(d), R.FAKE, R.FAKE, None) == -1
        assert msg in L.lib().mmfm_last_error().decode()
    torch.cuda.synchronize()
