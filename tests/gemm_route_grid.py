"""The descriptor grid of tests/golden/gemm_route.json: every case is a mmfm_gemm_desc with fake, non-null pointers 64 KiB apart (the
route reads pointers only for NULL and alignment), asked of mmfm_gemm_family; every pair case two of them, asked of
mmfm_gemm_pair_fused.  One character per case, in the order of `cases` / `pair_cases`: the family code as a digit (pairs: '1' one
launch, '0' two), 'x' where the launch refuses.

The grid is a "one clause off" sweep: BASES holds descriptors their family takes, FLIPS moves one clause of one `takes` predicate
(or of gemm_check) to a boundary value, and every (base, flip) is asked for both dtypes, with and without a live-row record, with bf16
and fp32 output, whole and split-K.  A flip wins over an axis where both set a field.

Run as a script it prints the codes of the thinned grid and of the pairs, a line each: most of the route's environment switches are
read once per process, so tests/test_gemm_route_cpu.py asks about them in child processes."""
import itertools
import sys

F32, BF16 = 0, 1
CHARS = "0123456789"
OPERANDS = ("A", "B", "C", "bias", "pre_out", "gradmul_pre", "residual", "colsum", "drop", "live")      # fake pointer i at 64 KiB * (i + 1)

# leading dimensions default to the contiguous extent (lda = K or M, ldb = K or N, ldc = ldr = N), kchunk to ceil(K / splits) rounded up to 64
BASES = {
    "big": dict(M=24576, N=256, K=512, ak=1, bk=1),                       # 96 x 1 tiles of 256
    "big_wide": dict(M=1024, N=24576, K=512, ak=1, bk=1),                 # 4 x 96 tiles
    "dw": dict(M=768, N=256, K=4096, ak=0, bk=0),                         # dY^T X
    "dw_long": dict(M=256, N=256, K=65536, ak=0, bk=0, on=("colsum",)),   # ... over >= 32,768 rows: 256-wide tiles
    "tile": dict(M=300, N=200, K=264, ak=1, bk=0),
}

FLIPS = [dict()]
FLIPS += [dict(K=k) for k in (448, 512, 576, 520, 1024, 32767, 32768)]
FLIPS += [dict(M=m) for m in (1023, 1024, 764, 24320, 24576)]
FLIPS += [dict(N=n) for n in (120, 128, 132, 136, 256)]
FLIPS += [dict(N=n, K=k) for n in (128, 136) for k in (32767, 32768)]                       # the streaming width
FLIPS += [dict(pad={ld: 4}) for ld in ("a", "b", "c")] + [dict(on=("residual",), pad={"r": p}) for p in (0, 4)]
FLIPS += [dict(M=764, pad={"a": 4}), dict(N=132, pad={"b": 4})]                             # ragged rows inside a padded leading dimension
FLIPS += [dict(off={op: 8}) for op in ("A", "B", "C")] + [dict(off={"C": 2})]
FLIPS += [dict(on=(op,), off={op: o}) for op in ("bias", "pre_out", "gradmul_pre", "residual") for o in (0, 8)]
FLIPS += [dict(on=("colsum",)), dict(on=()), dict(act=1), dict(on=("drop",)), dict(act=3), dict(act=26)]
FLIPS += [dict(kchunk_add=32), dict(kchunk_add=-64), dict(splits=0), dict(slab_stride=8)]
FLIPS += [dict(ak=a, bk=b) for a in (0, 1) for b in (0, 1)]                                 # (0, 1) is not built
# the 32-bit offset bounds, one step either side: M * max(ldc, ldr) * 2 of the 256-tile kernel, (K + 576) * max(lda, ldb) * 2 of the stream
FLIPS += [dict(M=32768, ldc=ld) for ld in (32760, 32768)] + [dict(M=32768, on=("residual",), ldr=ld) for ld in (32760, 32768)]
FLIPS += [dict(K=k, **{ld: 32768}) for ld in ("lda", "ldb") for k in (32191, 32192)]
FLIPS += [dict(live_rows=-1)]                                                               # a record of another row space

AXES = [dict(dtype=dt, live=lv, c_f32=cf, splits=sp) for dt in (BF16, F32) for lv in (0, 1) for cf in (0, 1) for sp in (1, 4)]


def cases(thin=False):
    """Descriptor specs; thinned: bf16 without a live record."""
    for (name, base), flip, axes in itertools.product(BASES.items(), FLIPS, AXES):
        if thin and (axes["dtype"] != BF16 or axes["live"]):
            continue
        yield dict(axes, **dict(base, **flip))


def cdiv(a, b):
    return -(-a // b)


def desc(L, s):
    """(mmfm_gemm_desc, mmfm_live_rows or None) of a spec."""
    on, off, pad = s.get("on", ()), s.get("off", {}), s.get("pad", {})
    p = lambda op: 0x10000 * (OPERANDS.index(op) + 1) + off.get(op, 0)
    opt = lambda op: p(op) if op in on else None
    d = L.GemmDesc()
    d.dtype, d.c_f32, d.M, d.N, d.K, d.a_kcontig, d.b_kcontig = s["dtype"], s["c_f32"], s["M"], s["N"], s["K"], s["ak"], s["bk"]
    d.A, d.B, d.C = p("A"), p("B"), p("C")
    d.lda = s.get("lda", (d.K if d.a_kcontig else d.M) + pad.get("a", 0))
    d.ldb = s.get("ldb", (d.K if d.b_kcontig else d.N) + pad.get("b", 0))
    d.ldc = s.get("ldc", d.N + pad.get("c", 0))
    d.ldr = s.get("ldr", d.N + pad.get("r", 0)) if "residual" in on else 0
    d.splits = s["splits"]
    d.kchunk = cdiv(cdiv(d.K, max(1, d.splits)), 64) * 64 + s.get("kchunk_add", 0) if d.splits != 1 else 0
    d.slab_stride = s.get("slab_stride", d.M * d.ldc + d.M)
    d.bias, d.pre_out, d.gradmul_pre, d.residual, d.colsum = opt("bias"), opt("pre_out"), opt("gradmul_pre"), opt("residual"), opt("colsum")
    d.act = s.get("act", 3 if "gradmul_pre" in on else 0)
    d.act_scale = 1.0
    d.drop = L.Dropout(p("drop"), 3, 0.25) if "drop" in on else L.NO_DROP
    live = None
    if s.get("live"):
        live = L.LiveRows()
        live.rec, live.B, live.T = p("live"), 1, (d.M if d.a_kcontig else d.K) + s.get("live_rows", 0)
    return d, live


# ------------------------------------------------------------------------------------------------ pairs
# weight gradients over 8,192 rows in 128-wide tiles: [256, 256] makes 4 items a slab, so `splits` 2 / 3 put the first problem's item
# count at 8 / 12 and 64 + 64 / 64 + 66 the sum at 512 / 520
_DW = dict(dtype=BF16, live=0, c_f32=1, M=256, N=256, K=8192, ak=0, bk=0)
PAIR_MEMBERS = [dict(_DW, splits=s) for s in (1, 2, 3, 64, 66)]
PAIR_MEMBERS += [dict(_DW, K=32768, splits=2), dict(_DW, K=32768, splits=3), dict(_DW, K=32768, N=128, splits=2)]    # 256-wide, and N too narrow for it
PAIR_MEMBERS += [dict(_DW, splits=1, on=("bias",)), dict(_DW, splits=2, pad={"a": 4}), dict(_DW, splits=2, off={"B": 8}),     # the stream does not take these
                 dict(_DW, splits=2, ak=1, bk=1), dict(_DW, splits=2, dtype=F32), dict(_DW, splits=2, c_f32=0, on=("colsum",))]
PAIR_MEMBERS += [dict(_DW, splits=2, kchunk_add=32)]                                                                            # refused


def pair_cases():
    return itertools.product(PAIR_MEMBERS, PAIR_MEMBERS)


# ------------------------------------------------------------------------------------------------ asking
def code(answer):
    return "x" if answer < 0 else CHARS[answer]


def codes(thin=False):
    """mmfm_gemm_family's own answers (negative: refused), without ops.gemm_family's exception."""
    from multi_modal_foundation_model_amd import _lib as L
    ask = L.lib().mmfm_gemm_family
    return "".join(code(ask(*desc(L, s))) for s in cases(thin))


def pair_codes():
    from multi_modal_foundation_model_amd import _lib as L
    ask = L.lib().mmfm_gemm_pair_fused
    return "".join(code(ask(desc(L, a)[0], desc(L, b)[0])) for a, b in pair_cases())


if __name__ == "__main__":
    sys.stdout.write(codes(thin=True) + "\n" + pair_codes() + "\n")
