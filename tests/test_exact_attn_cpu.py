"""CPU proof of tests/exact_inputs_attn.py for every launch tests/test_gpu_exact_attn.py runs: the
makers' conditions hold, the float64 references are F.scaled_dot_product_attention in float64
(explicit mask, enable_gqa; the int8 variants on the dequantised cache with the current rows
substituted) to 1e-12 and round to the closed-form expected bits, the closed-form split records
are the float64 records' fp32 bits, and each named kernel mistake (a key lost, a key counted
twice, row L admitted, the neighbouring kv head's or the other batch's V read) changes the
expected bf16 output, so the GPU's torch.equal assertions are not vacuous."""

import math

import pytest
import torch
import torch.nn.functional as F

import exact_inputs_attn as xa
from exact_inputs_attn import BF16, B, D


def _sdpa(inp, k, v, counts):
    return F.scaled_dot_product_attention(inp.q.double(), k.double(), v.double(),
                                          attn_mask=counts[0, 0] > 0, scale=xa.f32(inp.scale),
                                          enable_gqa=True)


def _changed(out, ref):
    """bool [B, H, S]: the bf16 output row differs somewhere (a NaN row differs)."""
    return (out.to(BF16) != ref.to(BF16)).any(-1)


def _check_reference(inp, k, v):
    """attn64 == SDPA to 1e-12 and rounds to the expected bits; returns (counts, ref)."""
    H, _ = xa.heads(inp.G)
    counts = xa.causal_counts(inp.pos, inp.T, H)
    ref = xa.attn64(inp.q, k, v, counts, inp.scale)
    c = inp.check
    torch.testing.assert_close(ref[:, :, c], _sdpa(inp, k, v, counts)[:, :, c], rtol=1e-12,
                               atol=1e-12)
    assert torch.equal(xa.out_layout(ref.to(BF16))[:, c], inp.expect[:, c])
    return counts, ref


def _needle_mutations(inp, counts, ref):
    c = inp.check.view(1, 1, -1)
    n = inp.sel.sum(-1)
    order = torch.argsort(inp.sel.int(), dim=-1, descending=True, stable=True)
    for i in range(int(n.max())):
        key = order[..., i:i + 1]
        active = (n > i) & c
        for mult, on in ((0.0, active), (2.0, active & (n > 1))):  # lost; counted twice
            val = torch.where(on.unsqueeze(-1), torch.full_like(key, mult, dtype=torch.float64),
                              counts.gather(-1, key))
            out = xa.attn64(inp.q, inp.k, inp.v, counts.scatter(-1, key, val), inp.scale)
            assert bool(_changed(out, ref)[on].all()), (mult, i)
    for name, v in (("kv head", inp.v.roll(1, 1)), ("batch", inp.v.flip(0))):
        out = xa.attn64(inp.q, inp.k, v, counts, inp.scale)
        assert bool(_changed(out, ref)[c.expand_as(n)].all()), name


def _admit_next_row(inp, k, v, counts, ref):
    """Row pos + 1 of the last checked query admitted: the poison shows."""
    s = int(inp.check.nonzero().max())
    row = int(inp.pos[s]) + 1
    if row >= inp.T:
        return
    c2 = counts.clone()
    c2[:, :, s, row] = 1
    out = xa.attn64(inp.q, k, v, c2, inp.scale)
    assert bool(_changed(out, ref)[:, :, s].all())


def _uniform_mutations(inp):
    G = inp.G
    v = inp.v.double()
    want = inp.expect.view(B, len(inp.pos), -1, D).transpose(1, 2)[:, ::G]  # [B, Hkv, S, D]
    for s, p in enumerate(inp.pos.tolist()):
        L = p + 1
        tot, w = inp.vsum[:, :, s:s + 1], want[:, :, s:s + 1]
        rows = v[:, :, :L]
        lost = ((tot - rows) / (L - 1)).to(BF16)
        twice = ((tot + rows) / (L + 1)).to(BF16)
        assert bool((lost != w).any(-1).all()), (s, L)
        # (the only key of L = 1 counted twice is the same average: no input can show it)
        assert L == 1 or bool((twice != w).any(-1).all()), (s, L)
        if L < inp.T:  # a +-1 row of a later query, or the 2^100 past the last position
            assert bool((((tot + v[:, :, L:L + 1]) / (L + 1)).to(BF16) != w).any(-1).all())
    x = inp.vsum / (inp.pos + 1).double().view(1, 1, -1, 1)
    assert bool((x.roll(1, 1).to(BF16) != want).any(-1).all())
    assert bool((x.flip(0).to(BF16) != want).any(-1).all())


def _check_records(rec, o, m, l):
    """Closed-form records == the float64 records' fp32 bits where a range is determined; a
    needle range without a selected key has a strictly lower m (merge weight exp(-gap) = 0)."""
    has = rec.has
    assert torch.equal(o.float()[has], rec.o[has])
    assert torch.equal(l.float()[has], rec.l[has]) and torch.equal(m.float()[has], rec.m[has])
    low = ~has & ~rec.empty.view(1, -1)
    assert bool((m.float()[low] <= rec.m[low] - xa.GAP_MIN).all())
    e = rec.empty
    assert bool((o[:, e] == 0).all()) and bool((l[:, e] == 0).all())
    assert bool((m[:, e] == -math.inf).all())


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
@pytest.mark.parametrize("route", list(xa.DECODE_CASES))
def test_decode_inputs(route, family, G):
    cases, scales = xa.DECODE_CASES[route]
    for T, L in cases:
        for si, scale in enumerate(scales):
            for inp in xa.decode_inputs(family, G, T, L, T + L, scale):
                counts, ref = _check_reference(inp, inp.k, inp.v)
                if family == "uniform":
                    assert inp.reseeds < 8
                    _uniform_mutations(inp)
                elif family == "poison":
                    _admit_next_row(inp, inp.k, inp.v, counts, ref)
                elif si == 0:  # the expected bits do not depend on the scale
                    _needle_mutations(inp, counts, ref)
                if route not in ("split", "q8"):
                    continue
                q8 = route == "q8"
                k, v = inp.k, inp.v
                if q8:
                    c8 = xa.to_q8(inp, poison=family != "needle")
                    k, v = c8.kd, c8.vd
                    _check_reference(inp, k, v)
                    if family != "needle":
                        _admit_next_row(inp, k, v, counts, ref)
                        # row L - 1 read from the codes, not from k_cur / v_cur
                        out = xa.attn64(inp.q, c8.k_cache.double() * c8.k_cache_scale.double(),
                                        c8.v_cache.double() * c8.v_cache_scale.double(), counts,
                                        inp.scale)
                        assert bool(_changed(out, ref).all())
                for splits in (2, 4):
                    ranges = xa.split_ranges(L, splits, q8)
                    make = xa.uniform_records if family == "uniform" else xa.needle_records
                    _check_records(make(inp, ranges),
                                   *xa.records64(inp.q, k, v, inp.scale, ranges))
            if family == "uniform":
                break  # q = 0: no scale


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
def test_prefill_inputs(family, G):
    for S, p0, T in xa.PREFILL_SPT:
        for inp in xa.prefill_inputs(family, G, S, p0, T, S + p0 + T):
            counts, ref = _check_reference(inp, inp.k, inp.v)
            if family == "uniform":
                _uniform_mutations(inp)
            elif family == "poison":
                _admit_next_row(inp, inp.k, inp.v, counts, ref)
            else:
                _needle_mutations(inp, counts, ref)


def test_placements_cover_what_they_claim():
    for L in (1, 15, 272):
        assert xa.needle_positions(L) == tuple(range(L))
    p = xa.needle_positions(1100)
    assert {0, 1, 1098, 1099, 63, 64, 65, 1087, 1088, 1089} <= set(p) and len(p) < 272
    assert xa.needle_pairs(65) == ((15, 16), (31, 32), (47, 48), (63, 64), (0, 64))
    for G in xa.GROUPS:
        H, Hkv = xa.heads(G)
        for L in (1, 17, 129, 1100):
            seen = set()
            for rows in xa.decode_launches(L, G):
                for b in range(B):
                    for kvh in range(Hkv):
                        grp = [set(rows[b][kvh * G + g][0]) for g in range(G)]
                        assert all(x == y or x.isdisjoint(y) for x in grp for y in grp)
                        seen.update(tuple(r[0]) for r in rows[b][kvh * G:(kvh + 1) * G])
            want = {(p,) for p in xa.needle_positions(L)} | set(xa.needle_pairs(L)) \
                | set(xa.needle_quads(L))
            assert seen == want
        for S, p0, T in xa.PREFILL_SPT:  # diagonal, the key before it, each block's first key
            rows = xa.prefill_launches(S, p0, G)
            assert all(rows[0][0][0][s] == (p0 + s,) for s in range(S))
            assert all(rows[1][0][0][s] == (max(p0 + s - 1, 0),) for s in range(S))
            assert {r[0] for r in rows[2][0][0]} == {(p0 + s) // 32 * 32 for s in range(S)}


def test_tie_zone_and_gap():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -9, 3.0, 0.0],
                     dtype=torch.float64)
    assert xa.tie_zone(x).tolist() == [True, True, False, False, False]
    for scale in xa.SCALES:
        gap = xa.A * xa.A * xa.f32(scale)
        assert gap >= xa.GAP_MIN and math.exp(-gap) < 2.0 ** -150
    with pytest.raises(AssertionError, match="gap"):
        xa.make_needle(1, 64, [3], xa.pack_launches([(1,)], 1)[0], 0, 0.02)
