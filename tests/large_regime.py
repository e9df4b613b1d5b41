"""The large-batch regime of the step plan: which side of every size gate a plan stands on ("The large-batch regime").

bench.py times B = 1024 (R = 204,800 rows).  Between the reference's batch of 16 and that size the plan builder and the launchers change
their choices at a dozen thresholds; `regime_record(engine, plan)` writes down, for one built plan, every choice that depends on the
size and nothing that merely scales with it (split counts, grid sizes, buffer sizes), so that two plans of different batch sizes in
the same regime give EQUAL records:

  decisions   what PlanBuilder.workspaces decides for the shape: fm (Engine._fused_mask), batch_red, pair_ok, ctx_group, live rows,
              use_keep per side - read off a PlanBuilder of the plan's own shape, not restated;
  names       the C function names per plan unit (plan_sig.plan_units);
  launches    for every launch whose LAUNCHER chooses by size, the side of each of its gates, computed from the descriptor the plan
              holds.  mmfm_gemm / mmfm_gemm_live / mmfm_gemm_pair: the library's own answer (mmfm_gemm_family: the 256-tile GEMM, the
              streaming weight-gradient kernel with 128- or 256-wide tiles, or the general 128-tile kernel; mmfm_gemm_pair_fused: whether
              a pair leaves in one launch), as mmfm_attn_family answers for the attention launches.  mmfm_reduce_slabs and mmfm_colsum
              (one- or two-stage reduction, which branch of colsum_splits) and every row-owner launch (column blocks on or off, whether
              any workgroup walks a second row pass): restated here ONCE from the launcher's code (source lines at each rule below).

B_BIG is the smallest batch of the default shapes (T = 100, `ap` 668 + `behavior` 2: R = 200 B rows, B T = 100 B tokeniser rows) on the
B = 1024 side of every gate; `host_gates` states the gates as functions of B and tests/test_large_regime_cpu.py proves the minimum.
All gates but one are thresholds, the last of them crossed at B = 328.  The exception is whether mmfm_gemm_pair really leaves as ONE
launch: PlanBuilder.pair_splits asks for slab counts that make the first problem's item count a multiple of 8, but the slab length is
rounded up to 64 rows afterwards and the count that comes out can be smaller - the launcher then issues the two products one after the
other (same sums, other grouping).  At B = 1024 all three pairs of a block leave together; at 328 .. 342 the [256, 256] + [256, 256] pair
(cross-attention out_proj + query) does not.  343 is the first batch from 328 on at which all three do.
No `test_*` module is imported here."""
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops
from multi_modal_foundation_model_amd import plan as P
from plan_sig import plan_units

T, N_AP, N_BEH, MODS = 100, 668, 2, 2
B_BENCH = 1024
# 328 is the first batch beyond every threshold: R = 65,600 > 65,536 (every row-owner grid has more passes than workgroups) and B T = 32,800
# >= 32,768 (the tokenisers' weight gradients stream 256-wide tiles).  343 (R = 68,600 = 535 x 128 + 120, B T = 34,300) is the first from
# there on at which every weight-gradient pair leaves in one launch, as at 1024 (module docstring)
B_BIG = 343
CUS = 256
# the weight-gradient pairs of a block, [N, K] + [N, K]: MLP down + up, attention out_proj + qkv, cross-attention out_proj + query
DW_PAIRS = (((256, 512), (512, 256)), ((256, 256), (768, 256)), ((256, 256), (256, 256)))


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the gates as functions of B
def host_gates(B, T=T, M=MODS):
    """{gate: True on the B = 1024 side} for batch B of the default shapes.  R = B M T rows of the stitched sequence, BT = B T rows of
    one tokeniser.  The thresholds that are named constants come from plan.py; the literals are the ones at the quoted lines, and
    tests/test_large_regime_cpu.py holds each against the function it restates wherever that function runs without a GPU."""
    R, BT = B * M * T, B * T
    return {
        "fused_mask_15": R >= 12288,                                      # engine.py Engine._fused_mask: `if R < 12288 and sw.fused is None: return 11`
        "batch_red_off_pairing_on": R > 8192,                             # plan.py PlanBuilder.workspaces: `self.batch_red = R <= 8192 and ...`, pair_ok = not batch_red
        "dw_split_large_branch": min(R, BT) > 8192,                       # engine.py Engine._dw_split: `if R <= 8192:` (called with R and with BT)
        "ctx_group": R >= P.CTX_GROUP_MIN,                                # plan.py ctx_group_on
        "live_rows": BT >= max(8192, P.LIVE_ROWS_MIN),                    # plan.py live_rows_on
        "rowgemm_column_blocks_off": cdiv(R, 128) >= 128,                 # csrc/rowgemm.hip mmfm_rowgemm / mmfm_rowgemm_groups: `npass < 128`
        "dw_wide_tiles": min(R, BT) >= 32768,                             # csrc/gemm_dw.hip dw_wide: `K >= 32768` (K = R, and B T for the tokenisers)
        "gemm_big_rows": BT >= 1024 and cdiv(BT, 256) >= 96,              # csrc/gemm_big.hip mmfm_gemm_big_takes: `d.M < 1024`, `< 96` tiles (narrowest output: one tile column)
        "reduce_large_branch": min(R, BT) > 8192,                         # csrc/gemm.hip colsum_splits: `R <= 8192 ? ... : min(256, R / 64)`
        # csrc/rowgemm.hip, csrc/mlp_fused.hip grid_for: min(passes, 256 per_cu) workgroups.  128-row passes at two workgroups per CU
        # (the K = 256 forward) and 256-row passes at one (the MLP backward's front half) are the last to get a second pass
        "second_row_pass_everywhere": cdiv(R, 128) > 2 * CUS and cdiv(R, 256) > CUS,
        # plan.py PlanBuilder.pair_splits (the product's own, on the host) into mmfm_gemm_pair_fused
        "dw_pairs_one_launch": all(pair_one_launch(*pair_descs(a, b, R)) for a, b in DW_PAIRS),
    }


def pair_descs(a, b, R):
    """The two descriptors PlanBuilder.dlin_ln hands mmfm_gemm_pair for weight gradients a = [Na, Ka] and b = [Nb, Kb] over R rows."""
    (Na, Ka), (Nb, Kb) = a, b
    Sa, kca, Sb, kcb = P.PlanBuilder.pair_splits(None, Na, Ka, Nb, Kb, R)
    dw = dict(a_kcontig=0, b_kcontig=0, c_f32=1, K=R)
    return (gemm_desc(M=Na, N=Ka, lda=Na, ldb=Ka, ldc=Ka, splits=Sa, kchunk=kca, **dw),
            gemm_desc(M=Nb, N=Kb, lda=Nb, ldb=Kb, ldc=Kb, splits=Sb, kchunk=kcb, **dw))


# ------------------------------------------------------------------------------------------------ the launchers' rules, per descriptor
KERNEL_NAMES = {L.GEMM_FAMILY_F32: "f32", L.GEMM_FAMILY_TILE128: "tile128", L.GEMM_FAMILY_BIG256: "big", L.GEMM_FAMILY_DW128: "dw128",
                L.GEMM_FAMILY_DW256: "dw256"}


def gemm_kernel(d, live=None):
    """Which kernel mmfm_gemm - with `live`, mmfm_gemm_live - gives descriptor `d`: the library's answer (mmfm_gemm_family)."""
    return KERNEL_NAMES[ops.gemm_family(d, live)]


def gemm_gates(d, live=None):
    """The size-free identity of a GEMM descriptor (its two widths: a weight gradient reduces over the rows, K) and its gate sides."""
    widths = (d.N, d.K) if d.a_kcontig else (d.M, d.N)
    return dict(widths=widths, a_kcontig=int(d.a_kcontig), c_f32=int(d.c_f32), split=d.splits > 1, kernel=gemm_kernel(d, live))


def pair_one_launch(a, b):
    """Whether mmfm_gemm_pair issues descriptors `a` and `b` as one launch: the library's answer (mmfm_gemm_pair_fused)."""
    return ops.gemm_pair_fused(a, b)


def two_stage(n, nslabs, stride):
    """mmfm_reduce_slabs (csrc/gemm.hip:445-466): the vector path sums tall-skinny slab sets (>= 16 slabs, < 512 chunks of 256 floats) in
    groups first."""
    chunks = cdiv(n, 256)
    if n % 4 or stride % 4 or nslabs < 16 or chunks >= 512:
        return False
    want = min(nslabs // 4, max(1, 512 // chunks))
    return cdiv(nslabs, cdiv(nslabs, want)) > 1


def colsum_gates(R, N):
    """mmfm_colsum (csrc/gemm.hip:473-501): which branch of colsum_splits, and the stage count of the reduction of its partials."""
    S = max(1, min(15, R // 256)) if R <= 8192 else min(256, R // 64)
    return dict(N=N, large_branch=R > 8192, two_stage=two_stage(N, S, N))


def rowowner_gates(fn, d):
    """Row passes of a row-owner launch: grid_for(R, per_cu, nw) = min(ceil(R / 32 nw), 256 per_cu) workgroups walk ceil(R / 32 nw) passes
    (csrc/rowgemm.hip:769, csrc/mlp_fused.hip:611).  per_cu and the pass height per kernel: mmfm_rowgemm csrc/rowgemm.hip:799-855,
    mmfm_rowgemm_groups :891-927, mmfm_mlp_fwd csrc/mlp_fused.hip:645-657, mmfm_mlp_bwd :664-683.  Column blocks: the K = 256 forward on the
    LDS-DMA ring (no residual, or N = 256 without a norm) with fewer than 128 passes (rowgemm.hip:840-847, :915-919)."""
    per_cu, rows, pairs, kind = 1, 128, 0, (fn,)
    if fn in ("mmfm_rowgemm", "mmfm_rowgemm_groups"):
        groups = d.groups if fn == "mmfm_rowgemm_groups" else 1
        kind = (fn, d.K, d.N, int(d.ln), int(d.ln_bwd), bool(d.residual), groups)
        if not d.ln_bwd and d.K == 256:
            per_cu = 2
            if fn == "mmfm_rowgemm_groups" or not d.residual or (d.N == 256 and not d.ln):
                pairs = (d.N >> 6) * groups
    elif fn == "mmfm_mlp_bwd":
        kind = (fn, "front half" if not d.dx else "one launch")
        rows = 256 if not d.dx else 128
    npass = cdiv(d.R, rows)
    ny = max(1, min(pairs, 512 // npass)) if pairs and npass < 128 else 1
    blocks = ny >= 4 if fn == "mmfm_rowgemm" and d.residual else ny > 1          # with a residual (N = 256): four blocks of one pair, or none
    return dict(kind=kind, column_blocks=blocks, second_pass=npass > CUS * per_cu)


ROW_OWNER = ("mmfm_rowgemm", "mmfm_rowgemm_groups", "mmfm_mlp_fwd", "mmfm_mlp_bwd")


def launch_gates(fn, args, keep):
    """The gate record of one plan entry, or None for a launch whose launcher does not choose by size."""
    name = fn.__name__
    if name in ("mmfm_gemm", "mmfm_gemm_live"):
        return dict(fn=name, **gemm_gates(*keep[:2]))            # keep: the descriptor, and mmfm_gemm_live's record
    if name == "mmfm_gemm_pair":
        return dict(fn=name, a=gemm_gates(keep[0]), b=gemm_gates(keep[1]), one_launch=pair_one_launch(keep[0], keep[1]))
    if name == "mmfm_reduce_slabs":
        _, _, n, nslabs, stride, _ = args
        return dict(fn=name, n=n, two_stage=two_stage(n, nslabs, stride))
    if name == "mmfm_colsum":
        return dict(fn=name, **colsum_gates(args[2], args[3]))
    if name in ROW_OWNER:
        return dict(fn=name, **rowowner_gates(name, keep[0]))
    return None


# ------------------------------------------------------------------------------------------------ the record
def builder_decisions(engine, plan):
    """What PlanBuilder.workspaces decides for the plan's shape and mode, from a builder of that shape (it finds every workspace in the
    shape's pool and allocates nothing new; its launch lists are dropped).  The environment must be the one the plan was built under."""
    engine._select_pool(plan["B"], plan["T"])
    pb = P.PlanBuilder(engine, plan["B"], plan["T"], plan["training"], plan["bwd"] is not None)
    before = set(engine.b)
    pb.workspaces()
    assert set(engine.b) == before, f"the plan was built under other switches: {sorted(set(engine.b) ^ before)}"
    return dict(fm=pb.fm, batch_red=pb.batch_red, pair_ok=pb.pair_ok, ctx_group=pb.ctx_group, live=pb.live,
                use_keep={side: sd.use_keep for side, sd in pb.sides.items()})


def regime_record(engine, plan):
    units = plan_units(plan)
    launches = {}
    for unit, entries in units:
        launches[unit] = [g for g in (launch_gates(fn, args, keep) for fn, args, keep in entries) if g is not None]
    return dict(decisions=builder_decisions(engine, plan), names={unit: [fn.__name__ for fn, _, _ in entries] for unit, entries in units},
                launches=launches)


def record_diff(a, b, path=""):
    """Where two records differ, one line each (for the assertion message)."""
    if isinstance(a, dict) and isinstance(b, dict):
        return [line for k in sorted(set(a) | set(b), key=str) for line in record_diff(a.get(k), b.get(k), f"{path}/{k}")]
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [line for i, (x, y) in enumerate(zip(a, b)) for line in record_diff(x, y, f"{path}[{i}]")]
    return [] if a == b else [f"{path}: {a!r} != {b!r}"]


def gemm_desc(**kw):
    """A mmfm_gemm_desc for the two questions above, no GPU needed: fake, non-null, 16-byte-aligned operands 64 KiB apart (the route
    reads pointers only for NULL and alignment); split-K slabs of M * ldc floats unless `slab_stride` says otherwise."""
    d = L.GemmDesc()
    d.A, d.B, d.C = (0x10000 * (i + 1) for i in range(3))
    for k, v in dict(dict(dtype=L.BF16, a_kcontig=1, b_kcontig=1, splits=1, act_scale=1.0, slab_stride=kw["M"] * kw["ldc"]), **kw).items():
        assert hasattr(L.GemmDesc, k), k
        setattr(d, k, v)
    return d
