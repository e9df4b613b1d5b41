"""The segment references of tests/mod_segments_refs.py, proved on the CPU: against nn.Embedding autograd on a ragged batch,
against the uniform references of tests/edge_refs.py at equal lengths, against the boolean gather upstream de-stitches with -
and a reference with an off-by-one in a slot's offset is told apart by the same comparisons."""
import pytest
import torch

import edge_refs as E
import mod_segments_refs as S

F64 = torch.float64
RAGGED = [(8, 5, 1), (1, 7)]
B, H, MAX_F = 3, 8, 8


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed), dtype=F64)


def slot_inputs(Ts, seed=0):
    """Per slot: tokens [B*T, H], a modality row, a position table, stamps with repeats (distinct per slot); and keep0 [L]."""
    L = sum(Ts)
    toks = [rnd(B * T, H, seed=seed + 10 + j) for j, T in enumerate(Ts)]
    rows = [rnd(H, seed=seed + 20 + j) for j in range(len(Ts))]
    poss = [rnd(MAX_F, H, seed=seed + 30 + j) for j in range(len(Ts))]
    tss = [torch.randint(0, MAX_F, (B, T), generator=gen(seed + 40 + j)) for j, T in enumerate(Ts)]
    keep0 = (torch.rand(L, generator=gen(seed + 50)) > 0.3).to(torch.uint8)
    keep0[0] = 0
    return toks, rows, poss, tss, keep0


def torch_stitch(toks, rows, poss, tss, keep0, Ts):
    """Upstream's way (encoder_embeddings.py:56-61, mm.py:97-149): embed each modality with nn.Embedding, concatenate along the
    token axis, zero the tokens sample 0 masks."""
    xs, leaves = [], []
    for tok, row, pos, ts, T in zip(toks, rows, poss, tss, Ts):
        tok, row = tok.clone().requires_grad_(True), row.clone().requires_grad_(True)
        table = torch.nn.Embedding(MAX_F, H, dtype=F64)
        table.weight.data.copy_(pos)
        leaves.append((tok, row, table.weight))
        xs.append((tok.view(B, T, H), row[None, None, :] + table(ts)))
    keep = keep0.to(F64)[None, :, None]
    x = torch.cat([t for t, _ in xs], 1) * keep + torch.cat([e for _, e in xs], 1)
    return x, torch.cat([e for _, e in xs], 1), leaves


@pytest.mark.parametrize("Ts", RAGGED)
def test_stitch_refs_match_embedding_autograd(Ts, off_error=0):
    toks, rows, poss, tss, keep0 = slot_inputs(Ts)
    x, emb, leaves = torch_stitch(toks, rows, poss, tss, keep0, Ts)
    dx = rnd(B, sum(Ts), H, seed=7)
    x.backward(dx)
    off = S.offsets(Ts)
    for j, T in enumerate(Ts):
        o = off[j] + (off_error if j else 0)
        xr, er, _ = S.stitch_fwd(toks[j], rows[j], poss[j], tss[j], keep0, o, MAX_F)
        torch.testing.assert_close(xr, x[:, off[j]:off[j] + T].detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(er, emb[:, off[j]:off[j] + T].detach(), rtol=1e-12, atol=1e-12)
        r = S.stitch_bwd(dx, None, tss[j], keep0, None, 0.0, o, MAX_F)
        tok, row, table = leaves[j]
        torch.testing.assert_close(r["d_tok"], tok.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(r["d_mod"], row.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(r["d_pos"], table.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Ts", [(8, 5, 1), (5, 7)])
def test_offset_off_by_one_is_rejected(Ts):
    """A slot one position off reads its neighbour's keep0 and gradient rows: the autograd comparison above must fail."""
    with pytest.raises(AssertionError):
        test_stitch_refs_match_embedding_autograd(Ts, off_error=-1)
    perm, good = S.destitch_perm(B * sum(Ts), Ts), S.offsets(Ts)
    bad = list(good)
    bad[1] += 1                                          # slot 1 starts one late: its first row lands in slot 0's block
    y = rnd(B * sum(Ts), H, seed=3)
    out = torch.empty_like(y)
    out[perm] = y
    mm = S.mod_mask(Ts).repeat(B)
    j = 1
    assert torch.equal(out[B * good[j]:B * good[j + 1]], y[mm == j])
    assert not torch.equal(out[B * bad[j]:B * bad[j] + B * Ts[j]], y[mm == j])


def test_refs_reduce_to_uniform_at_equal_lengths():
    T, M = 5, 3
    Ts = (T,) * M
    L = M * T
    toks, rows, poss, _, keep0 = slot_inputs(Ts)
    ts = torch.randint(0, MAX_F, (B, T), generator=gen(1))
    dx, dextra = rnd(B, L, H, seed=2), rnd(B, L, H, seed=3)
    for m in range(M):
        for a, b in zip(S.stitch_fwd(toks[m], rows[m], poss[m], ts, keep0, m * T, MAX_F), E.stitch_fwd(toks[m], rows[m], poss[m], ts, keep0, m, MAX_F)):
            assert torch.equal(a, b)
        ra, rb = S.stitch_bwd(dx, dextra, ts, keep0, None, 0.0, m * T, MAX_F), E.stitch_bwd(dx, dextra, ts, keep0, None, 0.0, m, MAX_F)
        assert ra.keys() == rb.keys()
        for k in ra:
            assert torch.equal(torch.as_tensor(ra[k]), torch.as_tensor(rb[k])), k
    attn = (torch.rand(B, T, generator=gen(4)) > 0.2).long()
    masks = [(torch.rand(B, T, 3, generator=gen(5 + m)) > 0.5).long() for m in range(M)]
    for a, b in zip(S.mask_prep(masks, [3] * M, [attn] * M, [12, 2, 4]), E.mask_prep(masks, [3] * M, attn, [12, 2, 4])):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(S.destitch_perm(B * L, Ts), E.destitch_perm(B * L, L, T, None))
    x, g, bt, dy = rnd(B * L, H, seed=8), rnd(H, seed=9), rnd(H, seed=10), rnd(B * L, H, seed=11)
    for a, b in zip(S.layernorm_fwd(x, g, bt, Ts), E.layernorm_fwd(x, g, bt, 1e-5, L, T)):
        assert torch.equal(a, b)
    ra, rb = S.layernorm_bwd(dy, x, g, None, Ts), E.layernorm_bwd(dy, x, g, None, 1e-5, L, T)
    for k in ra:
        assert torch.equal(torch.as_tensor(ra[k]), torch.as_tensor(rb[k])), k


@pytest.mark.parametrize("Ts", RAGGED + [(3, 3)])
def test_destitch_is_the_boolean_gather(Ts):
    """decoder_embeddings.py:105-107: the head of modality j reads y[decoder_mod_mask == j], rows in (b, t) order."""
    L = sum(Ts)
    y = rnd(B, L, H, seed=1)
    mm = S.mod_mask(Ts)[None, :].expand(B, L)
    out = torch.empty(B * L, H, dtype=F64)
    perm = S.destitch_perm(B * L, Ts)
    assert sorted(perm.tolist()) == list(range(B * L))
    out[perm] = y.reshape(B * L, H)
    off = S.offsets(Ts)
    for j, T in enumerate(Ts):
        assert torch.equal(out[B * off[j]:B * off[j + 1]], y[mm == j])
    x, g, bt = rnd(B * L, H, seed=2), rnd(H, seed=3), rnd(H, seed=4)
    yr, _, _ = S.layernorm_fwd(x, g, bt, Ts)
    ln = torch.nn.functional.layer_norm(x, (H,), g, bt, 1e-5).view(B, L, H)
    for j in range(len(Ts)):
        torch.testing.assert_close(yr[B * off[j]:B * off[j + 1]], ln[mm == j], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Ts", RAGGED)
def test_mask_prep_ref_is_upstreams_concatenation(Ts):
    """mm.py:270 per modality, :152-158 (the key mask is the concatenation of the per-modality masks), :229-233 (n_examples)."""
    chans = [12, 2, 4][:len(Ts)]
    attns = [(torch.rand(B, T, generator=gen(20 + j)) > 0.3).long() for j, T in enumerate(Ts)]
    evals = [(torch.rand(B, T, c, generator=gen(30 + j)) > 0.5).long() for j, (T, c) in enumerate(zip(Ts, chans))]
    tokmask, keypad, keep0, mod_id, count = S.mask_prep(evals, chans, attns, chans)
    per = [e[:, :, 0] & a for e, a in zip(evals, attns)]
    assert torch.equal(tokmask, (torch.cat(per, 1) != 0).to(torch.uint8))
    assert torch.equal(keypad, (torch.cat(attns, 1) != 0).to(torch.uint8))
    assert torch.equal(keep0, (torch.cat(per, 1)[0] != 1).to(torch.uint8))
    assert torch.equal(mod_id, S.mod_mask(Ts).to(torch.uint8))
    assert count.tolist() == [int(p[:, :, None].expand(-1, -1, c).sum()) for p, c in zip(per, chans)]
