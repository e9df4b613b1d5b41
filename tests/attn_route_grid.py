"""The descriptor grid of tests/golden/attn_route.json: every case is a mmfm_attn_desc with fake, aligned, non-null pointers (the
route reads pointers only for NULL and alignment), asked of mmfm_attn_family.  One character per case, in the order of `cases`:
the family code as a digit, 'j' (3 | 0x10) for the bf16 family's single-pass backward, 'x' where the launch refuses.

Run as a script it prints the codes of the thinned grid: the route's environment switches are read once per process, so
tests/test_attn_route_cpu.py asks about them in child processes."""
import itertools
import sys

DTYPES = (0, 1)                                   # MMFM_F32, MMFM_BF16
DHS = (8, 16, 32, 64, 128)
LENGTHS = (8, 40, 72, 129, 136, 200, 204, 224, 232, 256, 264, 600, 1024, 2656, 2664, 6080, 6112, 9824, 9856, 22496, 22528)
THIN_LENGTHS = (72, 129, 200, 232, 600, 2664, 9856, 22528)
CROSS = ((72, 129), (72, 136), (40, 24), (200, 232), (232, 200))
FLAGS = (0, 1, 2, 4, 5, 7)                        # DIAG 1, CAUSAL 2, SEP 4; masks only where Lq == Lk
WORKSPACE = (False, True)
DROP_P = (0.0, 0.4)
GRADS_ALIGNED = (True, False)                     # leading dims heads * dh, or heads * dh + 4
BACKWARD = (False, True)
B, HEADS = 2, 2
CHARS = "0123456789abcdefghijklmnopqrstuvwxyz"


def shapes(thin=False):
    for L in (THIN_LENGTHS if thin else LENGTHS):
        for fl in FLAGS:
            yield L, L, fl
    for Lq, Lk in CROSS:
        yield Lq, Lk, 0


def cases(thin=False):
    """(dtype, dh, Lq, Lk, flags, workspace, drop_p, grads_aligned, backward), backward fastest."""
    for dtype, dh, (Lq, Lk, fl) in itertools.product(DTYPES, DHS, shapes(thin)):
        for rest in itertools.product(WORKSPACE, DROP_P, GRADS_ALIGNED, BACKWARD):
            yield (dtype, dh, Lq, Lk, fl) + rest


def desc(ops, L, dtype, dh, Lq, Lk, flags, workspace=False, drop_p=0.0, grads_aligned=True):
    hd = HEADS * dh
    ldg = hd if grads_aligned else hd + 4
    p = lambda i: 0x10000 * (i + 1)                # fake device pointers, 64 KiB apart
    d = ops.attn_desc(dtype, B, HEADS, Lq, Lk, dh, p(0), p(1), p(2), hd, hd, hd, p(3), hd, None, None, None, flags, dh ** -0.5,
                      drop_p=L.Dropout(p(7), 3, drop_p) if drop_p > 0 else None,
                      d_o=p(8), lddo=ldg, dq=p(9), dk=p(10), dv=p(11), lddq=ldg, lddk=ldg, lddv=ldg)
    d.lse, d.keypad, d.mod_id = p(4), p(5), p(6)
    d.keepbits = p(12) if workspace else None
    return d


def family(ops, L, case):
    """mmfm_attn_family's own answer for a case (negative: refused), without ops.attn_family's exception."""
    return L.lib().mmfm_attn_family(desc(ops, L, *case[:-1]), int(case[-1]))


def codes(thin=False):
    from multi_modal_foundation_model_amd import _lib as L, ops
    out = []
    for c in cases(thin):
        f = family(ops, L, c)
        out.append("x" if f < 0 else CHARS[f])
    return "".join(out)


if __name__ == "__main__":
    sys.stdout.write(codes(thin=True) + "\n")
