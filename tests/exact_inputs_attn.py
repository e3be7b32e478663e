"""Inputs on which the attention kernels can be checked BIT FOR BIT.

Same idea as tests/exact_inputs.py: every score, softmax weight and partial sum is an exactly
representable fp32 number whatever the order of the keys, the chunking of the cache and the merges
of partial softmax states, so the kernels (tao_attn_decode_bf16 one-pass and chunk-split,
tao_attn_decode_split_bf16 + tao_attn_merge_bf16, tao_attn_decode_q8_bf16, tao_attn_prefill_bf16)
must give the bits of the float64 formula of include/torchao_mi355x_llama.h. D = 128, bf16.

Key codes. Key row j of every kv head is A * (e[j % 64] + e[64 + (j // 64) % 64]), A = 64 (unique
for j < 4096); the query that selects key j is the same vector. The selected key scores 2 A^2, a
key sharing one index A^2, the others 0: integers below 2^24 in any summation order. For both
scales (0.125 and 1 / sqrt(128)) the gap A^2 * scale is >= 110, so exp(s - m) of every unselected
key is < 2^-150, exactly 0 in fp32, and exp(0) is exactly 1. (Asserted per scale.)

Families:
  "needle"   every (batch, query head, query) selects a set S of keys inside its valid range, |S|
             in {1, 2, 4}: the further members are K rows overwritten with the selected code. Rows
             holding the code PAST the query's position are traps: a prefill mask taken from another
             query of the block admits them and changes the average. V is integer in [-64, 64], rows
             unique over (batch, kv head, row). out = bf16(sum_S v / |S|): exact (|S| a power of
             two), independent of order, chunking and merges. A split's record over a key range is
             o = sum of v over S in range, l = |S in range|, m = 2 A^2 * scale (exact at scale
             0.125); a range without a selected key has a lower m and merges with weight exactly 0.
             Catches: a lost key (the sweep selects every key once), a key counted twice (|S| > 1),
             the wrong kv head or batch, the wrong output row.
  "poison"   needle, plus every cache row at or past `poison_from` (decode: L; prefill: one past a
             victim query's position, later queries unchecked) filled with K = 2 A (score 4 A^2, above
             every valid key) and V = 2^100 (finite: a masked weight 0 times it stays 0). One
             admitted masked key turns the output into 2^100. int8 cache: codes +-127 with scale
             1000 from row L - 1 on (the current key must come from k_cur / v_cur).
  "uniform"  q = 0: every score 0, every weight exactly 1, l = L. V in {-1, +1} (rows past the last
             position 2^100): partial sums are small integers. A record is o = sum of v over the
             range, l = its keys, m = 0; an empty range o = 0, m = -inf, l = 0. out =
             bf16(sum v / L): exact for L a power of two; otherwise the kernels multiply by an fp32
             reciprocal (relative error < 2^-22 for reciprocal and product together), so V is
             reseeded until no expected element lies within 2^-20 relative of a midpoint between
             two bf16 numbers (fewer than 8 reseeds, asserted). Catches a lost, doubled or admitted
             key at EVERY position (each moves sum / L by about 1 / sqrt(L) relative, several bf16
             ulps), and a wrong l.
int8-cache variants (to_q8): codes = the values above with bf16 scale 1 (K in {0, 64}, V its
integers), the current token's rows in k_cur / v_cur; dequantisation is exact however computed.

The makers assert their conditions on the CPU; the references (attn64, records64) are written
from the header formulas in float64 and call no code under test. tests/test_exact_attn_cpu.py
proves, for every launch of tests/test_gpu_exact_attn.py, that the closed forms are the float64
formula's bits and that each named kernel mistake changes them.
"""

import functools
import math
from types import SimpleNamespace

import torch

from exact_inputs import BF16, describe_mismatch  # noqa: F401  (re-exported)

D = 128
A = 64
B = 2
GROUPS = (1, 4, 8)
SCALES = (0.125, 1 / math.sqrt(128))
GAP_MIN = 110.0
POISON_V = 2.0 ** 100
Q8_POISON_CODE, Q8_POISON_SCALE = 127, 1000.0
SWEEP_ALL_L = 272  # needle positions sweep every key up to this length
FAMILIES = ("needle", "poison", "uniform")

# ---- the (T, L) / (S, p0, T) of every GPU case -------------------------------------------------
ONE_PASS_TL = ((64, 1), (64, 15), (64, 16), (64, 17), (272, 127), (272, 128), (272, 129),
               (272, 257), (272, 272), (1024, 1024))
CHUNK_FORCED_TL = ((128, 1), (128, 63), (128, 64), (128, 65), (128, 128))  # tao_tune_attn 1
CHUNK_ROUTED_TL = ((1536, 65), (1536, 1100), (1536, 1536))                 # T > 1024
SPLIT_TL = ((64, 1), (64, 15), (64, 17), (64, 33), (64, 64), (328, 129), (328, 257), (328, 328),
            (1024, 700))
Q8_TL = ((64, 1), (64, 2), (64, 16), (64, 17), (64, 18), (328, 129), (328, 328), (1536, 1100))
PREFILL_SPT = ((1, 0, 64), (7, 0, 64), (16, 0, 64), (17, 31, 64), (33, 37, 160), (48, 95, 160))
PREFILL_NW = (0, 1, 2, 4)  # 0 = the built-in choice
# decode route -> ((T, L) cases, softmax scales of its needle / poison launches); records are
# checked at 0.125 only, where m = 2 A^2 * scale is exact
DECODE_CASES = {
    "one_pass": (ONE_PASS_TL, SCALES),
    "chunk_forced": (CHUNK_FORCED_TL, SCALES[1:]),
    "chunk_routed": (CHUNK_ROUTED_TL, SCALES[1:]),
    "split": (SPLIT_TL, SCALES[:1]),
    "q8": (Q8_TL, SCALES[:1]),
}


def heads(G):
    """(H, Hkv) of a GQA group size, as tests/test_gpu_attn_split.py picks them."""
    Hkv = 8 // G if G < 8 else 2
    return Hkv * G, Hkv


def f32(x):
    """The fp32 value a kernel receives for a Python float, as float64."""
    return float(torch.tensor(x, dtype=torch.float32))


def key_codes(T):
    """float64 [T, D]: the code of every key row."""
    assert T <= 4096, "codes repeat from row 4096"
    j = torch.arange(T)
    k = torch.zeros(T, D, dtype=torch.float64)
    k[j, j % 64] = A
    k[j, 64 + (j // 64) % 64] = A
    return k


def out_layout(x):
    """[B, H, S, D] -> the kernels' [B, S, H * D]."""
    Bb, H, S, _ = x.shape
    return x.transpose(1, 2).reshape(Bb, S, H * D)


def causal_counts(pos, T, H):
    """float64 [B, H, S, T]: 1 where key t <= pos[s]."""
    m = (torch.arange(T)[None, :] <= torch.as_tensor(pos)[:, None]).double()
    return m.expand(B, H, *m.shape).clone()


# ---- float64 references (include/torchao_mi355x_llama.h) ---------------------------------------

def attn64(q, k, v, counts, scale):
    """softmax(q k^T * scale) v per (batch, head, query) over the keys with counts > 0, key t
    taken counts[..., t] times (1 everywhere in range = the header's formula; 0 / 2 model a lost
    / doubled key). q [B, H, S, D], k / v [B, Hkv, T, D], counts [B, H, S, T] -> float64
    [B, H, S, D]."""
    G = q.shape[1] // k.shape[1]
    kk = k.double().repeat_interleave(G, 1)
    vv = v.double().repeat_interleave(G, 1)
    s = torch.einsum("bhsd,bhtd->bhst", q.double(), kk) * f32(scale)
    s = torch.where(counts > 0, s, torch.full_like(s, -math.inf))
    m = s.amax(-1, keepdim=True)
    w = counts * torch.exp(s - m)
    return (w @ vv) / w.sum(-1, keepdim=True)


def records64(q, k, v, scale, ranges):
    """The split record of each key range (a list of key indices per range) for S = 1: float64
    o [B * H, NS, D] = sum exp(s - m) v, m, l [B * H, NS]; an empty range o = 0, m = -inf, l = 0."""
    H = q.shape[1]
    G = H // k.shape[1]
    kk = k.double().repeat_interleave(G, 1)
    vv = v.double().repeat_interleave(G, 1)
    s = torch.einsum("bhsd,bhtd->bhst", q.double(), kk)[:, :, 0] * f32(scale)  # [B, H, T]
    o = torch.zeros(B * H, len(ranges), D, dtype=torch.float64)
    m = torch.full((B * H, len(ranges)), -math.inf, dtype=torch.float64)
    l = torch.zeros(B * H, len(ranges), dtype=torch.float64)
    for i, r in enumerate(ranges):
        if not r:
            continue
        idx = torch.tensor(r)
        sr = s[:, :, idx]
        mr = sr.amax(-1, keepdim=True)
        w = torch.exp(sr - mr)
        m[:, i] = mr.reshape(-1)
        l[:, i] = w.sum(-1).reshape(-1)
        o[:, i] = torch.einsum("bht,bhtd->bhd", w, vv[:, :, idx]).reshape(-1, D)
    return o, m, l


def split_ranges(L, splits, q8=False):
    """Key indices of each range of tao_attn_decode_split_bf16 (ceil(L / splits) keys rounded up
    to 16) or, q8, of tao_attn_decode_q8_bf16 (the L - 1 cached keys split likewise, range 0 also
    taking the current key L - 1)."""
    n = L - 1 if q8 else L
    C = ((n + splits - 1) // splits + 15) // 16 * 16
    out = [list(range(min(s * C, n), min((s + 1) * C, n))) for s in range(splits)]
    if q8:
        out[0].append(L - 1)
    assert sorted(sum(out, [])) == list(range(L))
    return out


# ---- placement lists ----------------------------------------------------------------------------

def needle_positions(L):
    if L <= SWEEP_ALL_L:
        return tuple(range(L))
    p = {0, 1, L - 2, L - 1}
    for m in range(16, L, 16):
        p.update((m - 1, m, m + 1))
    return tuple(sorted(x for x in p if 0 <= x < L))


def needle_pairs(L):
    """Every adjacent pair that straddles a multiple of 16, and (0, L - 1)."""
    p = [(m - 1, m) for m in range(16, L, 16)]
    if L >= 2:
        p.append((0, L - 1))
    return tuple(p)


def needle_quads(L):
    """Four keys around every multiple of 64 (the chunk edge, four waves' steps), and both ends."""
    p = [(m - 2, m - 1, m, m + 1) for m in range(64, L - 1, 64)]
    if L >= 4:
        p.append((0, 1, L - 2, L - 1))
    return tuple(p)


def pack_launches(sets, G):
    """Deal key sets to the B * H (batch, head) slots of as many launches as it takes, so that the
    sets of heads sharing a kv head are disjoint (or the same set, used to fill up a launch).
    Returns a list of rows[b][h][0] = set."""
    H, _ = heads(G)
    n = B * H
    pending, launches = list(sets), []
    while pending:
        slots, rest = [], []
        for s in pending:
            grp = slots[len(slots) // G * G:]
            if len(slots) < n and all(set(s).isdisjoint(o) for o in grp):
                slots.append(tuple(s))
            else:
                rest.append(s)
        while len(slots) < n:
            grp = slots[len(slots) // G * G:]
            slots.append(grp[0] if grp else slots[0])
        launches.append([[[slots[b * H + h]] for h in range(H)] for b in range(B)])
        pending = rest
    return launches


@functools.lru_cache(maxsize=None)
def decode_launches(L, G):
    """Every needle launch of a decode case: singles over needle_positions, then pairs, then
    quads."""
    out = []
    for sets in ([(p,) for p in needle_positions(L)], needle_pairs(L), needle_quads(L)):
        out += pack_launches(sets, G)
    return out


@functools.lru_cache(maxsize=None)
def prefill_launches(S, p0, G):
    """Needle launches of a prefill case, rows[b][h][s]: the diagonal key, the key before it, the
    first key of the diagonal's 32-key block, sweeps in which the last query walks over every key,
    and trap launches: each kv group's queries all select key 0 and a copy of its code at row
    p0 + t, which is in range from query t on and a trap for the queries before."""
    H, Hkv = heads(G)
    n, last = B * H, p0 + S
    pos = [p0 + s for s in range(S)]

    def launch(f):
        return [[[f(b * H + h, s) for s in range(S)] for h in range(H)] for b in range(B)]

    out = [launch(lambda i, s: (pos[s],)),
           launch(lambda i, s: (max(pos[s] - 1, 0),)),
           launch(lambda i, s: (pos[s] // 32 * 32,))]
    for r in range((last + n - 1) // n):
        out.append(launch(lambda i, s, r=r: ((i + n * r + 5 * (S - 1 - s)) % (pos[s] + 1),)))
    ngrp = B * Hkv
    for r in range((S + ngrp - 1) // ngrp):
        def trap(i, s, r=r):
            t = (r * ngrp + i // G) % S
            return (0, p0 + t) if p0 + t else (0,)
        out.append(launch(trap))
    seen = {row for rows in out for b in rows for h in b for s, rs in enumerate(h) for row in rs
            if row <= pos[s]}
    assert seen == set(range(last)), "a key position no query selects"
    return out


def prefill_victims(S):
    """Queries after which the cache is poisoned, one launch each: all of them up to 17 queries,
    else both ends of every 16-query block."""
    if S <= 17:
        return tuple(range(S))
    return tuple(sorted({s for s in (0, 1, 14, 15, 16, 17, 30, 31, 32, 33, S - 2, S - 1) if s < S}))


# ---- makers --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _needle_v(Hkv, T, seed):
    gen = torch.Generator().manual_seed(977 * seed + 13)
    v = torch.randint(-64, 65, (B, Hkv, T, D), generator=gen).double()
    flat = v.view(-1, D)
    assert torch.unique(flat, dim=0).shape[0] == flat.shape[0], "V rows are not unique"
    return v


def _as_bf16(x):
    y = x.to(BF16)
    assert torch.equal(y.double(), x), "a value is not a bf16 number"
    return y


def make_needle(G, T, pos, rows, seed, scale, poison_from=None):
    """rows[b][h][s]: the K rows that hold the code of rows[b][h][s][0], which query (b, h, s)
    selects; the members at or below pos[s] are its set, the others traps. poison_from: the first
    poisoned cache row (family "poison"); queries at or past it are not to be checked.
    Returns q [B, H, S, D], k / v [B, Hkv, T, D] bf16, pos int64 [S], expect [B, S, H * D] bf16,
    sel bool [B, H, S, T] (the in-range set), check bool [S]."""
    H, Hkv = heads(G)
    S = len(pos)
    assert 2 * A * A < 2 ** 24 and A * A * f32(scale) >= GAP_MIN, "softmax gap too small"
    codes = key_codes(T)
    k = codes.expand(B, Hkv, T, D).clone()
    v = _needle_v(Hkv, T, seed).clone()
    q = torch.zeros(B, H, S, D, dtype=torch.float64)
    want = torch.zeros(B, H, S, T, dtype=torch.bool)
    pos_t = torch.as_tensor(pos, dtype=torch.int64)
    assert 0 <= int(pos_t.min()) and int(pos_t.max()) < T
    for b in range(B):
        for h in range(H):
            for s in range(S):
                r = rows[b][h][s]
                assert 0 <= r[0] <= pos[s], "the selected key is out of range"
                q[b, h, s] = codes[r[0]]
                for row in r:
                    k[b, h // G, row] = codes[r[0]]
                    want[b, h, s, row] = row <= pos[s]
    check = torch.ones(S, dtype=torch.bool)
    if poison_from is not None:
        k[:, :, poison_from:] = 2 * A
        v[:, :, poison_from:] = POISON_V
        check = pos_t < poison_from
        assert bool(check.any())
    valid = (torch.arange(T)[None, :] <= pos_t[:, None]) & check[:, None]  # [S, T]
    sc = torch.einsum("bhsd,bhtd->bhst", q, k.repeat_interleave(G, 1))
    ok = (sc == 0) | (sc == A * A) | (sc == 2 * A * A) | ~valid
    assert bool(ok.all()), "a valid key scores outside {0, A^2, 2 A^2}"
    sel = (sc == 2 * A * A) & valid
    assert torch.equal(sel, want & valid), "heads of one kv group select overlapping sets"
    n = sel.sum(-1)
    nc = n[:, :, check]
    assert bool(((nc == 1) | (nc == 2) | (nc == 4)).all()), "|S| must be 1, 2 or 4"
    out = (sel.double() @ v.repeat_interleave(G, 1)) / n.clamp(min=1).unsqueeze(-1).double()
    return SimpleNamespace(G=G, T=T, scale=scale, q=_as_bf16(q), k=_as_bf16(k), v=_as_bf16(v),
                           pos=pos_t, expect=out_layout(out.to(BF16)), sel=sel, check=check)


def needle_records(inp, ranges):
    """Expected records of a decode needle launch: o [B * H, NS, D], l, m [B * H, NS] fp32 and
    has [B * H, NS] (the range holds a selected key: only then are o, l and m determined; without
    one, m is lower and the merge weight exactly 0), empty [NS]."""
    H, Hkv = heads(inp.G)
    sel = inp.sel[:, :, 0].double()  # [B, H, T]
    vv = inp.v.double().repeat_interleave(inp.G, 1)
    NS = len(ranges)
    o = torch.zeros(B * H, NS, D)
    l = torch.zeros(B * H, NS)
    for i, r in enumerate(ranges):
        if r:
            idx = torch.tensor(r)
            l[:, i] = sel[:, :, idx].sum(-1).reshape(-1).float()
            o[:, i] = torch.einsum("bht,bhtd->bhd", sel[:, :, idx], vv[:, :, idx]).reshape(-1, D)
    m = torch.full((B * H, NS), 2 * A * A * f32(inp.scale), dtype=torch.float32)
    assert float(m[0, 0]) == 2 * A * A * inp.scale, "m is exact only for a power-of-two scale"
    return SimpleNamespace(o=o, l=l, m=m, has=l > 0, empty=torch.tensor([not r for r in ranges]))


def tie_zone(x):
    """Whether float64 x lies within 2^-20 relative of a midpoint between two bf16 numbers."""
    mant, _ = torch.frexp(x.abs())
    y = mant * 256  # in [128, 256): bf16 numbers are the integers, midpoints the half-integers
    return (((y - y.floor()) - 0.5).abs() / y < 2.0 ** -20) & (x != 0)


def make_uniform(G, T, pos, seed):
    """q = 0, V in {-1, +1} up to the last position (2^100 past it), expect[s] = bf16(sum of v
    over keys 0..pos[s] / (pos[s] + 1)). Returns make_needle's fields, vsum float64
    [B, Hkv, S, D] and reseeds."""
    H, Hkv = heads(G)
    pos_t = torch.as_tensor(pos, dtype=torch.int64)
    Ls = (pos_t + 1).double().view(1, 1, -1, 1)
    pow2 = ((pos_t + 1) & pos_t) == 0
    for reseeds in range(8):
        gen = torch.Generator().manual_seed(7919 * seed + 31 * reseeds + 5)
        v = (torch.randint(0, 2, (B, Hkv, T, D), generator=gen) * 2 - 1).double()
        vsum = v.cumsum(2)[:, :, pos_t]  # [B, Hkv, S, D]
        x = vsum / Ls
        # L a power of two: the quotient is an fp32 number, rounded to bf16 once on both sides
        if not bool(tie_zone(x)[:, :, ~pow2].any()):
            break
    else:
        raise AssertionError("no V without an expected value next to a bf16 midpoint")
    assert reseeds < 8
    assert float(vsum.abs().max()) < 2 ** 24
    v[:, :, int(pos_t.max()) + 1:] = POISON_V
    k = key_codes(T).expand(B, Hkv, T, D).clone()
    q = torch.zeros(B, H, len(pos), D, dtype=torch.float64)
    expect = out_layout(x.to(BF16).repeat_interleave(G, 1))
    return SimpleNamespace(G=G, T=T, scale=SCALES[1], q=_as_bf16(q), k=_as_bf16(k), v=_as_bf16(v),
                           pos=pos_t, expect=expect, vsum=vsum, reseeds=reseeds,
                           check=torch.ones(len(pos), dtype=torch.bool))


def uniform_records(inp, ranges):
    """Expected records of a decode uniform launch: o = sum of v over the range, l = its keys,
    m = 0; an empty range o = 0, m = -inf, l = 0. Every range is determined (has = all)."""
    H, _ = heads(inp.G)
    vv = inp.v.double().repeat_interleave(inp.G, 1)
    NS = len(ranges)
    o = torch.zeros(B * H, NS, D)
    l = torch.zeros(B * H, NS)
    m = torch.zeros(B * H, NS)
    for i, r in enumerate(ranges):
        if r:
            o[:, i] = vv[:, :, torch.tensor(r)].sum(2).reshape(-1, D).float()
            l[:, i] = len(r)
        else:
            m[:, i] = -math.inf
    return SimpleNamespace(o=o, l=l, m=m, has=torch.ones(B * H, NS, dtype=torch.bool),
                           empty=torch.tensor([not r for r in ranges]))


def to_q8(inp, poison):
    """The int8-cache form of a decode launch (S = 1): codes int8 [B, Hkv, T, D], bf16 scales
    [B, Hkv, T, 1] (all 1), k_cur / v_cur [B, Hkv, 1, D] = row L - 1. poison: rows L - 1 .. T - 1
    of the caches hold codes +127 (K) / -127 (V) with scale 1000. Also kd / vd: the dequantised
    cache with the current rows substituted, float64."""
    L = int(inp.pos[0]) + 1
    k, v = inp.k.double().clone(), inp.v.double().clone()
    k_cur, v_cur = inp.k[:, :, L - 1:L].clone(), inp.v[:, :, L - 1:L].clone()
    ks = torch.ones(*k.shape[:3], 1, dtype=torch.float64)
    vs = ks.clone()
    # rows past L are never valid: bring the bf16 families' poison into the int8 range
    k[:, :, L:] = torch.where(k[:, :, L:] > A, 0.0, k[:, :, L:])
    v[:, :, L:] = torch.where(v[:, :, L:].abs() > A, 0.0, v[:, :, L:])
    if poison:
        k[:, :, L - 1:] = Q8_POISON_CODE
        v[:, :, L - 1:] = -Q8_POISON_CODE
        ks[:, :, L - 1:] = Q8_POISON_SCALE
        vs[:, :, L - 1:] = Q8_POISON_SCALE
    for c in (k, v):
        assert bool((c == c.round()).all()) and float(c.abs().max()) <= 127
    kd, vd = k * ks, v * vs
    kd[:, :, L - 1] = k_cur[:, :, 0].double()
    vd[:, :, L - 1] = v_cur[:, :, 0].double()
    return SimpleNamespace(k_cache=k.to(torch.int8), v_cache=v.to(torch.int8),
                           k_cache_scale=_as_bf16(ks), v_cache_scale=_as_bf16(vs),
                           k_cur=k_cur, v_cur=v_cur, kd=kd, vd=vd)


def decode_inputs(family, G, T, L, seed, scale):
    """Every launch of one decode case of a family: a generator of make_needle / make_uniform
    results."""
    if family == "uniform":
        yield make_uniform(G, T, [L - 1], seed)
        return
    for rows in decode_launches(L, G):
        yield make_needle(G, T, [L - 1], rows, seed, scale,
                          poison_from=L if family == "poison" else None)


def prefill_inputs(family, G, S, p0, T, seed, scales=SCALES):
    """Every launch of one prefill case of a family; the scales alternate over the launches."""
    pos = [p0 + s for s in range(S)]
    if family == "uniform":
        yield make_uniform(G, T, pos, seed)
    elif family == "needle":
        for i, rows in enumerate(prefill_launches(S, p0, G)):
            yield make_needle(G, T, pos, rows, seed, scales[i % len(scales)])
    else:
        rows = prefill_launches(S, p0, G)[0]  # the diagonal key: the needle next to the poison
        for i, s in enumerate(prefill_victims(S)):
            yield make_needle(G, T, pos, rows, seed, scales[i % len(scales)],
                              poison_from=pos[s] + 1)


def describe(route, got, want):
    """describe_mismatch over [rows, H * D] views of attention outputs or records."""
    return describe_mismatch(route, got.reshape(-1, got.shape[-1]).float(),
                             want.reshape(-1, want.shape[-1]).float())
