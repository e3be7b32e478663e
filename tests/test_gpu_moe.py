"""GPU tests of the many-token MoE expert FFN (csrc/moe_gemm.hip, torchao/prototype/moe_quant):
the route against argsort / bincount / cumsum on the CPU, the grouped int4 linear bit for bit on
exact inputs at every row tile, the combine against the same bf16 op sequence on the CPU, the whole
FFN and ``quantize_`` + module against float64 relative to the per-expert loop on the existing
int4 linears, determinism, graph capture, opcheck, and the int8 / float8 base configs."""

import functools

import pytest
import torch
import torch.nn.functional as F

import exact_inputs as X

from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao


def _status():
    from torchao._models.llama import kernels

    kernels.check_decode_status()


# ---- route ---------------------------------------------------------------------------------------

def _route_ref(flat, E):
    """(offsets, order, inverse) of int64 indices on the CPU, indices clamped to [0, E)."""
    flat = flat.clamp(0, E - 1)
    order = flat.argsort(stable=True)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(flat, minlength=E).cumsum(0)])
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel())
    return offsets.int(), order.int(), inverse.int()


def _check_route(flat, E, A):
    got = T.moe_route(flat.to(DEV).view(-1, A), E, A)
    for name, g, w in zip(("offsets", "order", "inverse"), got, _route_ref(flat, E)):
        assert g.dtype is torch.int32 and torch.equal(g.cpu(), w), name
    return got


def _shuffled(values, seed):
    v = torch.tensor(values, dtype=torch.int64)
    return v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(seed))]


def test_route_empty_single_and_straddling_expert():
    """E = 4, A = 2, T = 20: expert 1 empty, expert 3 one row, expert 0 17 rows (one past a 16-row
    tile), expert 2 the other 22."""
    flat = _shuffled([0] * 17 + [2] * 22 + [3], 1)
    offsets, _, _ = _check_route(flat, 4, 2)
    assert offsets.tolist() == [0, 17, 17, 39, 40]
    _status()


def test_route_many_experts_few_tokens():
    gen = torch.Generator().manual_seed(2)
    _check_route(torch.randint(0, 256, (3 * 8,), generator=gen), 256, 8)
    _status()


def test_route_all_on_one_expert_and_several_rounds():
    """600 activations on expert 5 of 8: three 256-entry rounds of the ranking pass, every other
    expert empty; then 1000 random ones."""
    _check_route(torch.full((600,), 5, dtype=torch.int64), 8, 2)
    gen = torch.Generator().manual_seed(3)
    _check_route(torch.randint(0, 8, (1000,), generator=gen), 8, 2)
    _status()


def test_route_bad_index_is_clamped_and_reported():
    flat = torch.tensor([0, 3, 9, 1, -2, 2, 3, 3], dtype=torch.int64)
    _status()
    _check_route(flat, 4, 2)  # against the clamped reference
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="expert index"):
        _status()
    _status()


def test_route_graph_replay_reads_the_indices_at_replay():
    E, A = 8, 2
    idx = torch.zeros(12, A, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.moe_route(idx, E, A)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = T.moe_route(idx, E, A)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (4, 5, 6):
        flat = torch.randint(0, E, (12 * A,), generator=torch.Generator().manual_seed(seed))
        idx.copy_(flat.view(12, A))
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, _route_ref(flat, E)):
            assert torch.equal(got.cpu(), want), seed
    _status()


# ---- grouped linear on exact inputs -------------------------------------------------------------
COUNTS = (17, 0, 33, 1)  # rows of experts 0..3: a straddled 16-row tile, none, 33, one
ROW_DIV = 2
# K = 320 is the K tail (320 = 256 + 64); it has no g = 128 case: K % g == 0 is the format's rule
GROUPED_NKG = [(N, K, g) for N in (64, 80) for K, g in
               ((256, 32), (256, 128), (320, 32), (1024, 32), (1024, 128))]


@functools.lru_cache(maxsize=None)
def _grouped_inputs(N, K, g, family):
    """Per-expert exact weights (a different seed per expert) over shared x rows; made once per
    shape and family, never modified. x [R, K] serves both forms: without src_row sorted row p
    reads x[p], with it x[src_row[p] // ROW_DIV]."""
    R, E = sum(COUNTS), len(COUNTS)
    seed = (N * 7 + K + g) % 1000
    _, _, _, x = X.make_int4_exact(R, N, K, g, seed, family)
    qs, szs, deq = [], [], []
    for e in range(E):
        q, s, z, _ = X.make_int4_exact(1, N, K, g, seed + 10 * (e + 1), family)
        X.check_int4_exact(x, q, s, z, g)  # the shared x against this expert's scales and zeros
        qs.append(q)
        szs.append(torch.stack([s, z], dim=-1))
        deq.append((q, s, z))
    packed = torch.stack([T.int4_pack(q.to(DEV)) for q in qs]).contiguous()
    sz = torch.stack(szs).contiguous().to(DEV)
    offsets = torch.tensor([0] + list(torch.tensor(COUNTS).cumsum(0)), dtype=torch.int32)
    src = torch.randint(0, R * ROW_DIV, (R,), generator=torch.Generator().manual_seed(seed),
                        dtype=torch.int32)
    want, want_src = [], []
    for e in range(E):
        rows = torch.arange(int(offsets[e]), int(offsets[e + 1]))
        if rows.numel():
            q, s, z = deq[e]
            want.append(X.ref_int4(x[rows], q, s, z, g))
            want_src.append(X.ref_int4(x[(src[rows] // ROW_DIV).long()], q, s, z, g))
    return (x.to(DEV), packed, sz, offsets.to(DEV), src.to(DEV), torch.cat(want),
            torch.cat(want_src))


@pytest.mark.parametrize("N,K,g", GROUPED_NKG)
def test_grouped_linear_exact(N, K, g):
    """Every partial sum is exact in fp32, so every row tile, with and without the gather, must give
    the float64 formula rounded once, bit for bit."""
    for family in X.FAMILIES:
        x, packed, sz, offsets, src, want, want_src = _grouped_inputs(N, K, g, family)
        for bm in (16, 32, 64):
            with tuning(moe=(bm, 0)):
                got = T.int4_grouped_linear(x, None, 1, packed, sz, None, None, offsets, g)
                got_src = T.int4_grouped_linear(x, src, ROW_DIV, packed, sz, None, None, offsets, g)
            where = f"N={N} K={K} g={g} {family} bm={bm}"
            assert torch.equal(got.cpu(), want), X.describe_mismatch(where, got.cpu(), want)
            assert torch.equal(got_src.cpu(), want_src), X.describe_mismatch(
                where + " src_row", got_src.cpu(), want_src)


# ---- combine -------------------------------------------------------------------------------------

@pytest.mark.parametrize("A", [1, 2, 3, 8])
def test_combine_matches_the_bf16_op_sequence(A):
    """acc = +0, then acc = bf16(acc + bf16(y2[p] * w)) over the token's positions in ascending
    order: torch's own bf16 mul and add on CPU copies. D = 264: 33 16-B pieces, a ragged block."""
    Tn, D = 5, 264
    R = Tn * A
    gen = torch.Generator().manual_seed(20 + A)
    y2 = torch.randn(R, D, generator=gen).to(torch.bfloat16)
    y2[0, :8] = -0.0
    w = torch.rand(R, generator=gen).to(torch.bfloat16)
    inverse = torch.randperm(R, generator=gen).int()
    want = torch.zeros(Tn, D, dtype=torch.bfloat16)
    for t in range(Tn):
        for p, f in sorted((int(inverse[t * A + a]), t * A + a) for a in range(A)):
            want[t] = want[t] + y2[p] * w[f]
    got = T.moe_combine(y2.to(DEV), w.to(DEV).view(Tn, A), inverse.to(DEV), A)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


# ---- the whole FFN and quantize_ + module -------------------------------------------------------
E_, A_, D_, I_ = 4, 2, 256, 512


@functools.lru_cache(maxsize=None)
def _moe(base="int4"):
    from torchao.prototype.moe_quant import (MOEFeedForwardAOQuantizable, MoEQuantConfig,
                                             cond_ffn_filter)
    from torchao.quantization import (Float8WeightOnlyConfig, Int4WeightOnlyConfig,
                                      Int8WeightOnlyConfig, quantize_)

    gen = torch.Generator().manual_seed(31)
    m = MOEFeedForwardAOQuantizable(D_, I_, E_, A_).to(torch.bfloat16)
    with torch.no_grad():
        m.router.weight.copy_(torch.randn(E_, D_, generator=gen) * 0.5)
        m.experts.w1.copy_(torch.randn(E_, I_, D_, generator=gen) / D_ ** 0.5)
        m.experts.w2.copy_(torch.randn(E_, D_, I_, generator=gen) / I_ ** 0.5)
        m.experts.w3.copy_(torch.randn(E_, I_, D_, generator=gen) / D_ ** 0.5)
    m = m.to(DEV)
    cfg = {"int4": Int4WeightOnlyConfig(group_size=32), "int8": Int8WeightOnlyConfig(),
           "float8": Float8WeightOnlyConfig()}[base]
    quantize_(m, MoEQuantConfig(cfg), cond_ffn_filter)
    return m


def _routing(m, x):
    scores = F.softmax(m.router(x), dim=-1)
    scores, idx = torch.topk(scores, m.top_k, dim=-1)
    scores /= scores.sum(dim=-1, keepdim=True).to(x.dtype)
    return idx, scores


def _x(Tn, seed=0):
    gen = torch.Generator().manual_seed(100 + Tn + seed)
    return torch.randn(Tn, D_, generator=gen).to(torch.bfloat16).to(DEV)


def _ffn_float64(m, x, idx, w):
    """The expert FFN in float64 on the dequantized weights (CPU)."""
    w1, w2, w3 = (getattr(m.experts, n).dequantize().double().cpu() for n in ("w1", "w2", "w3"))
    xd, idx, w = x.double().cpu(), idx.cpu(), w.double().cpu()
    out = torch.zeros(x.shape[0], D_, dtype=torch.float64)
    for t in range(x.shape[0]):
        for a in range(idx.shape[1]):
            e = int(idx[t, a])
            h = F.silu(xd[t] @ w1[e].t()) * (xd[t] @ w3[e].t())
            out[t] += w[t, a] * (h @ w2[e].t())
    return out


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dual", [1, 2])
@pytest.mark.parametrize("Tn", [2, 5, 40])
def test_whole_ffn_against_float64_relative_to_the_per_expert_loop(Tn, dual):
    """rel-L2 against float64 on the dequantized weights, of the grouped path (gate and up in two
    launches, dual = 1, or one, dual = 2) and of the per-expert loop on the existing int4 linears
    (what the module did without the kernels). Both differ from float64 only in summation order
    and the same bf16 rounding points: the grouped path's error must be <= 1.5 x the loop's (the
    factor covers the loop's route changes with M)."""
    m = _moe()
    x = _x(Tn)
    with torch.no_grad():
        idx, w = _routing(m, x)
        with tuning(moe=(0, dual)):
            got = m.experts(x, idx, w, A_)
            again = m.experts(x, idx, w, A_)
        loop = m.experts._many_tokens(x, idx, w, A_)
        ref = _ffn_float64(m, x, idx, w)
    assert got.shape == (Tn, D_) and got.dtype is torch.bfloat16
    assert torch.equal(got, again), "two runs of the same input differ"
    e_grouped, e_loop = _rel_l2(got, ref), _rel_l2(loop, ref)
    print(f"T={Tn} dual={dual}: rel-L2 vs float64: grouped {e_grouped:.4e}, loop {e_loop:.4e}")
    assert e_grouped <= 1.5 * e_loop, (e_grouped, e_loop)
    _status()


def test_quantize_and_module_end_to_end():
    """quantize_(m, MoEQuantConfig(Int4WeightOnlyConfig(32)), cond_ffn_filter), then the module's
    own forward (router, top-k, experts, reshape) at T = 5 and the same bound; T = 1 through the
    module is int4_moe_ffn_decode bit for bit."""
    from torchao._models.llama import kernels
    from torchao.dtypes import AffineQuantizedTensor

    m = _moe()
    for name in ("w1", "w2", "w3"):
        assert isinstance(getattr(m.experts, name), AffineQuantizedTensor)
    x = _x(5, seed=7)
    with torch.no_grad():
        y = m(x.view(5, 1, D_))
        idx, w = _routing(m, x)
        loop = m.experts._many_tokens(x, idx, w, A_)
        ref = _ffn_float64(m, x, idx, w)
    assert y.shape == (5, 1, D_)
    e_grouped, e_loop = _rel_l2(y.view(5, D_), ref), _rel_l2(loop, ref)
    print(f"module T=5: rel-L2 vs float64: grouped {e_grouped:.4e}, loop {e_loop:.4e}")
    assert e_grouped <= 1.5 * e_loop, (e_grouped, e_loop)
    x1 = _x(1)
    with torch.no_grad():
        idx, w = _routing(m, x1)
        got = m.experts(x1, idx, w, A_)
        want = kernels.int4_moe_ffn_decode(x1, m.experts.w1, m.experts.w2, m.experts.w3, idx, w)
    assert got.shape == x1.shape and torch.equal(got.reshape(-1), want.reshape(-1))
    _status()


def test_whole_ffn_in_a_graph_replays_with_new_routing():
    m = _moe()
    Tn = 5
    x, idx, w = _x(Tn), torch.zeros(Tn, A_, dtype=torch.int64, device=DEV), \
        torch.zeros(Tn, A_, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m.experts(x, idx, w, A_)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = m.experts(x, idx, w, A_)
    torch.cuda.current_stream().wait_stream(s)
    for seed in (1, 2):
        xs = _x(Tn, seed=seed)
        with torch.no_grad():
            i2, w2 = _routing(m, xs)
            want = m.experts(xs, i2, w2, A_)
        x.copy_(xs)
        idx.copy_(i2)
        w.copy_(w2)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), seed
    _status()


@pytest.mark.parametrize("base", ["int8", "float8"])
def test_other_base_configs_run_their_per_expert_loop(base):
    """Int8 / float8 expert weights run the reference's loop on the existing linears: the module is
    that loop (the same code), in both branches."""
    m = _moe(base)
    for Tn in (1, 5):
        x = _x(Tn)
        with torch.no_grad():
            idx, w = _routing(m, x)
            got = m.experts(x, idx, w, A_)
            loop = (m.experts._one_token if Tn == 1 else m.experts._many_tokens)(x, idx, w, A_)
        assert got.shape == (Tn, D_) and torch.equal(got, loop)
        assert bool(torch.isfinite(got.float()).all())


# ---- opcheck --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["moe_route", "int4_grouped_linear", "moe_combine"])
def test_opcheck(name):
    x, packed, sz, offsets, src, _, _ = _grouped_inputs(64, 256, 32, "dense")
    R = x.shape[0]
    gen = torch.Generator().manual_seed(9)
    args = {
        "moe_route": (torch.randint(0, 4, (6, 2), generator=gen).to(DEV), 4, 2),
        "int4_grouped_linear": (x, src, ROW_DIV, packed, sz, packed, sz, offsets, 32),
        "moe_combine": (torch.randn(6, 64, generator=gen).to(torch.bfloat16).to(DEV),
                        torch.rand(6, generator=gen).to(torch.bfloat16).to(DEV),
                        torch.randperm(6, generator=gen).int().to(DEV), 2),
    }[name]
    assert R == sum(COUNTS)
    torch.library.opcheck(getattr(T, name).default, args)
