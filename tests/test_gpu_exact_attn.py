"""Bit-exact tests of the attention kernels on the inputs of tests/exact_inputs_attn.py (families
"needle", "poison", "uniform"; tests/test_exact_attn_cpu.py proves them on the CPU):
tao_attn_decode_bf16 (one pass, and the two-launch 64-key chunk split, forced and routed by
T > 1024), tao_attn_decode_split_bf16 (records) + tao_attn_merge_bf16, tao_attn_decode_q8_bf16
(splits 1, 2, 4) and tao_attn_prefill_bf16 (every waves-per-block choice). Every assertion is
torch.equal or exact field equality against the float64 formulas of
include/torchao_mi355x_llama.h: a key lost or counted twice, a masked row admitted (row L, the
int8 cache's row L - 1, a prefill row past the query's own position), the wrong kv head, batch
or output row, or a wrong (o, m, l) record changes the bits.

tao_int4wo_qkv_attn_bf16 is out of scope: its q is the output of a GEMV and cannot be set
directly, it is off by default, and its attention is attn_decode_step (csrc/tao_attn.h), the
step of the one-pass kernel tested here."""

import contextlib
import math
from types import SimpleNamespace

import pytest
import torch

import exact_inputs_attn as xa
from exact_inputs_attn import B

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(inp):
    return inp.q.to(DEV), inp.k.to(DEV), inp.v.to(DEV), inp.pos.to(DEV)


def _same(route, got, want, check=None):
    got = got.cpu()
    if check is not None:
        got, want = got[:, check], want[:, check]
    assert torch.equal(got, want), xa.describe(route, got, want)


def _check_records(route, part, rec):
    """part [B * H, NS, 132] = o[128], m, l, pad against the closed-form records."""
    part = part.cpu()
    o, m, l = part[..., :128], part[..., 128], part[..., 129]
    has = rec.has
    assert torch.equal(o[has], rec.o[has]), xa.describe(route + " record o", o[has], rec.o[has])
    assert torch.equal(l[has], rec.l[has]), f"{route} record l: {l[has]} != {rec.l[has]}"
    assert torch.equal(m[has], rec.m[has]), f"{route} record m: {m[has]} != {rec.m[has]}"
    low = ~has & ~rec.empty.view(1, -1)  # no selected key: a lower maximum, merged with weight 0
    assert bool((m[low] < rec.m[low]).all()), f"{route} record m of a range without a needle"
    e = rec.empty
    assert bool((o[:, e] == 0).all()) and bool((l[:, e] == 0).all()), f"{route} empty record"
    assert bool((m[:, e] == -math.inf).all()), f"{route} empty record m"


def _decode_cases(route, family, G):
    """(tag, inputs) of every launch of a decode route."""
    cases, scales = xa.DECODE_CASES[route]
    for T, L in cases:
        for scale in scales[:1] if family == "uniform" else scales:
            for i, inp in enumerate(xa.decode_inputs(family, G, T, L, T + L, scale)):
                yield f"{route} {family} G={G} T={T} L={L} scale={inp.scale:.4g} launch {i}", inp


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
def test_one_pass_decode(family, G):
    from torchao._models.llama import kernels

    for tag, inp in _decode_cases("one_pass", family, G):
        q, k, v, pos = _dev(inp)
        _same(tag, kernels.attn_decode(q, k, v, pos, inp.scale), inp.expect)


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
@pytest.mark.parametrize("route", ["chunk_forced", "chunk_routed"])
def test_chunk_split_decode(route, family, G):
    from torchao._models.llama import kernels
    from torchao.kernel.tuning import tuning

    for tag, inp in _decode_cases(route, family, G):
        q, k, v, pos = _dev(inp)
        with tuning(attn=1) if route == "chunk_forced" else contextlib.nullcontext():
            got = kernels.attn_decode(q, k, v, pos, inp.scale)
        _same(tag, got, inp.expect)


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
@pytest.mark.parametrize("splits", [2, 4])
def test_split_records_and_merge(splits, family, G):
    from torchao._models.llama import kernels

    H, _ = xa.heads(G)
    records = xa.uniform_records if family == "uniform" else xa.needle_records
    for tag, inp in _decode_cases("split", family, G):
        tag = f"{tag} splits={splits}"
        q, k, v, pos = _dev(inp)
        L = int(inp.pos[0]) + 1
        scale = xa.SCALES[0]  # 0.125: the record's m is exact
        part = kernels.attn_decode_split(q, k, v, pos, scale, splits)
        _check_records(tag, part, records(inp, xa.split_ranges(L, splits)))
        merged = kernels.attn_merge(part, B, H)
        _same(tag + " merged", merged, inp.expect)
        one = kernels.attn_decode(q, k, v, pos, scale)
        assert torch.equal(merged, one), xa.describe(tag + " merged vs one-pass", merged.cpu(),
                                                     one.cpu())


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
@pytest.mark.parametrize("splits", [1, 2, 4])
def test_q8_decode(splits, family, G):
    from torchao._models.llama import kernels

    H, _ = xa.heads(G)
    records = xa.uniform_records if family == "uniform" else xa.needle_records
    for tag, inp in _decode_cases("q8", family, G):
        tag = f"{tag} splits={splits}"
        c8 = xa.to_q8(inp, poison=family != "needle")
        kv = SimpleNamespace(k_cache=c8.k_cache.to(DEV), v_cache=c8.v_cache.to(DEV),
                             k_cache_scale=c8.k_cache_scale.to(DEV),
                             v_cache_scale=c8.v_cache_scale.to(DEV))
        L = int(inp.pos[0]) + 1
        scale = xa.SCALES[0]
        got = kernels.attn_decode_q8(inp.q.to(DEV), kv, c8.k_cur.to(DEV), c8.v_cur.to(DEV),
                                     inp.pos.to(DEV), scale, splits)
        if splits > 1:
            _check_records(tag, got, records(inp, xa.split_ranges(L, splits, q8=True)))
            got = kernels.attn_merge(got, B, H)
        _same(tag, got, inp.expect)


@pytest.mark.parametrize("G", xa.GROUPS)
@pytest.mark.parametrize("family", xa.FAMILIES)
@pytest.mark.parametrize("nw", xa.PREFILL_NW)
def test_prefill(nw, family, G):
    from torchao._models.llama import kernels
    from torchao.kernel.tuning import tuning

    for S, p0, T in xa.PREFILL_SPT:
        for i, inp in enumerate(xa.prefill_inputs(family, G, S, p0, T, S + p0 + T)):
            q, k, v, pos = _dev(inp)
            with tuning(attn_prefill_nw=nw) if nw else contextlib.nullcontext():
                got = kernels.attn_prefill(q, k, v, pos, inp.scale)
            _same(f"prefill {family} G={G} nw={nw} S={S} p0={p0} T={T} scale={inp.scale:.4g} "
                  f"launch {i}", got, inp.expect, inp.check)
