"""The decode-fused float8 GEMVs (tao_fp8wo_decode_bf16, and tao_fp8dq_decode_bf16 for the
dynamic-activation config) against what they replace: RMSNorm kernel -> float8 linear ->
SiLU-mul / RoPE + KV write.

Without the RMSNorm prologue, on the inputs of tests/exact_inputs_fp8.py / exact_inputs_fp8dyn.py
(every product and partial sum an exact fp32 number) the accumulation order cannot matter, so the
outputs must equal the header formulas on the float64 sum BIT FOR BIT, and the epilogues must
equal the project's own unfused kernels (silu_mul, rope_kv) on the linear op's output bit for bit.

With the prologue, x is made of integers in [-8, 8] times a power of two: the sum of squares is
then an exact fp32 number in any order, so r = rsqrt(mean + eps) and the normalised bf16 token are
bit-identical between the prologue and kernels.rmsnorm. What remains is the fp32 order of the dot
products in another launch shape: the project's bar for exactly that, rel-L2 < 2e-3
(tests/test_gpu_decode_fused_int8.py::test_plain_matches_linear).
"""

import functools
import math

import pytest
import torch
import torch.nn as nn

import exact_inputs_fp8 as E8
import exact_inputs_fp8dyn as ED

from torchao import _lib
from torchao.kernel import tuning
from torchao.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    Float8WeightOnlyConfig,
    PerRow,
    quantize_,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
WO, DQ = "fp8wo_decode", "fp8dq_decode"
WO_K = (32, 1056, 8224, 16416)  # exact_inputs.INT8_GEMV_K rounded up to the kernel's 32
EPS = 1e-5


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def test_shape_lists():
    assert tuple(E8.round_up(K, 32) for K in E8.INT8_GEMV_K) == WO_K
    assert ED.GEMV_K == (16, 1024, 1040, 4112)


# ---- inputs, made once and left unchanged -----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wo_inputs(N, K, family):
    """x [1, 1, K] bf16, w [N, K] e4m3fn, scale [N] fp32 on the GPU; the float64-sum reference."""
    codes, scale, _, x = E8.make_fp8wo_exact(1, N, K, (N * 7 + K) % 1000, family)
    want = E8.ref_fp8wo(x, codes, scale)
    return x.view(1, 1, K).to(DEV), codes.view(FP8).to(DEV), scale.to(DEV), want


@functools.lru_cache(maxsize=None)
def _dq_inputs(N, K, seed):
    """The identity token of exact_inputs_fp8dyn (its per-row quantisation reproduces chosen
    codes and a power-of-two scale), weights of the "dense" family; the float64-sum reference."""
    xb, codes, scale, wq, ws, _ = ED.make_identity_token(N, K, seed)
    want = ED.ref_fp8dyn(codes, scale, wq, ws)
    return xb.view(1, 1, K).to(DEV), wq.view(FP8).to(DEV), ws.to(DEV), want


def _wo_check(N, K, tag=""):
    from torchao._models.llama import kernels

    for family in E8.FAMILIES:
        x, w, s, want = _wo_inputs(N, K, family)
        got = kernels.fp8wo_decode(x, w, s)
        assert WO in _last_kernel(), _last_kernel()
        assert got.shape == (1, 1, N)
        got = got.reshape(1, N).cpu()
        assert torch.equal(got, want), E8.describe_mismatch(
            f"fp8wo decode {tag} {family} N={N} K={K}", got, want)


def _dq_check(N, K, seed, tag=""):
    from torchao._models.llama import kernels

    x, w, s, want = _dq_inputs(N, K, seed)
    got = kernels.fp8dq_decode(x, w, s)
    assert DQ in _last_kernel(), _last_kernel()
    op = torch.ops.torchao.fp8_dyn_linear(x.view(1, K), w, s, None)
    assert torch.equal(got.reshape(1, N), op)
    got = got.reshape(1, N).cpu()
    assert torch.equal(got, want), ED.describe_mismatch(
        f"fp8dq decode {tag} N={N} K={K} seed={seed}", got, want)


# ---- bit-exact, no prologue -------------------------------------------------------------------

@pytest.mark.parametrize("K", WO_K)
@pytest.mark.parametrize("N", (1, 37, 330))
def test_fp8wo_plain_is_bit_exact(N, K):
    _wo_check(N, K)


@pytest.mark.parametrize("K", ED.GEMV_K)
@pytest.mark.parametrize("N", (37, 80))
def test_fp8dq_plain_is_bit_exact(N, K):
    for seed in (1, 2, 6):
        _dq_check(N, K, seed + K % 5)


@pytest.mark.parametrize("rpw,wk,rg", ED.GEMV_FORCED)
def test_forced_launch_shapes(rpw, wk, rg):
    with tuning(fp8_gemv=(rpw, wk, rg)):
        for K in WO_K:
            _wo_check(37, K, f"forced rpw={rpw} wk={wk} g={rg}")
        for K in ED.GEMV_K:
            _dq_check(37, K, 3, f"forced rpw={rpw} wk={wk} g={rg}")


def test_fp8dq_eight_pieces_per_thread():
    """One wave per workgroup at K = 4096: the widest token-piece count without the norm."""
    with tuning(fp8_gemv=(4, 1, 1)):
        _dq_check(37, 4096, 4, "npt 8")


@pytest.mark.parametrize("kernel", [WO, DQ])
def test_k_tail_next_to_nan_codes(kernel):
    """Rows of NaN codes (what an all-zero weight row quantises to), one directly after a row
    under test and one last (the row that rows past N clamp to), at a K whose last slice is
    partly empty: the lanes past K skip the math, the finite rows stay bit-exact and only the
    NaN rows' outputs are NaN."""
    from torchao._models.llama import kernels

    N = 37
    if kernel == WO:
        x, w, s, want = _wo_inputs(N, 1056, "dense")
        fn = kernels.fp8wo_decode
    else:
        x, w, s, want = _dq_inputs(N, 1040, 3)
        fn = kernels.fp8dq_decode
    w2 = w.view(torch.uint8).clone()
    w2[5], w2[N - 1] = 0x7F, 0xFF
    want = want.clone()
    want[:, [5, N - 1]] = float("nan")
    for shape in (None, (2, 1, 1), (8, 2, 1), (4, 8, 1)):
        if shape is None:
            got = fn(x, w2.view(FP8), s)
        else:
            with tuning(fp8_gemv=shape):
                got = fn(x, w2.view(FP8), s)
        assert kernel in _last_kernel()
        got = got.reshape(1, N).cpu()
        assert bool(got[:, [5, N - 1]].isnan().all()), shape
        assert not bool(got[:, [n for n in range(N) if n not in (5, N - 1)]].isnan().any()), shape
        assert E8.same_bf16(got, want), shape


def _linear_out(kernel, x, w, s):
    K = x.shape[-1]
    if kernel == WO:
        return torch.ops.torchao.fp8_weight_only_linear(x.view(1, K), w, s, None)
    return torch.ops.torchao.fp8_dyn_linear(x.view(1, K), w, s, None)


def _exact(kernel, N, K):
    from torchao._models.llama import kernels

    if kernel == WO:
        return kernels.fp8wo_decode, _wo_inputs(N, K, "dense")
    return kernels.fp8dq_decode, _dq_inputs(N, K, 5)


@pytest.mark.parametrize("I", (8, 165))
@pytest.mark.parametrize("kernel", [WO, DQ])
def test_swiglu_epilogue_equals_the_unfused_chain(kernel, I):
    """The linear's outputs are order-independent on these inputs, so the fused result equals
    silu_mul of the linear op's output bit for bit (pair_epilogue's documented arithmetic)."""
    from torchao._models.llama import kernels

    fn, (x, w, s, _) = _exact(kernel, 2 * I, 1056)
    lin = _linear_out(kernel, x, w, s)
    if I % 2:  # the unfused kernel takes an even count: one more (gate, up) pair, dropped again
        lin = torch.cat([lin, lin.new_zeros(1, 2)], dim=1)
    ref = kernels.silu_mul(lin)[:, :I]
    for shape in (None, (2, 2, 2), (4, 1, 2)):
        if shape is None:
            got = fn(x, w, s, epilogue="swiglu")
        else:
            with tuning(fp8_gemv=shape):
                got = fn(x, w, s, epilogue="swiglu")
        assert kernel in _last_kernel()
        assert got.shape == (1, 1, I)
        assert torch.equal(got.reshape(-1), ref.reshape(-1)), shape


@functools.lru_cache(maxsize=None)
def _freqs(H, Hkv, T, D=128):
    from torchao._models.llama.model import ModelArgs, _rope_freqs

    cfg = ModelArgs(n_layer=1, n_head=H, n_local_heads=Hkv, dim=H * D, rope_base=500000)
    return _rope_freqs(cfg, T).to(DEV)


def _caches(Hkv, T, D=128, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    kc = torch.randn(1, Hkv, T, D, device=DEV, dtype=BF16, generator=g)
    vc = torch.randn(1, Hkv, T, D, device=DEV, dtype=BF16, generator=g)
    return kc, vc


@pytest.mark.parametrize("pos", (0, 17, 63))
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("kernel", [WO, DQ])
def test_rope_kv_epilogue_equals_the_unfused_chain(kernel, H, Hkv, pos):
    from torchao._models.llama import kernels

    D, T = 128, 64
    N = (H + 2 * Hkv) * D
    fn, (x, w, s, _) = _exact(kernel, N, 1056)
    freqs = _freqs(H, Hkv, T)
    p = torch.tensor([pos], device=DEV)
    kc, vc = _caches(Hkv, T)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    kc0 = kc.clone()
    q = fn(x, w, s, epilogue="rope_kv", rope=(freqs, p, kc, vc, H))
    assert kernel in _last_kernel()
    q_ref = kernels.rope_kv(_linear_out(kernel, x, w, s).view(1, 1, N), freqs, p, kc_ref, vc_ref, H)
    assert q.shape == q_ref.shape == (1, H, 1, D)
    assert torch.equal(q, q_ref)
    assert torch.equal(kc, kc_ref) and torch.equal(vc, vc_ref)  # written and untouched rows
    rows = [t for t in range(T) if t != pos]
    assert torch.equal(kc[:, :, rows], kc0[:, :, rows])
    assert not torch.equal(kc[:, :, pos], kc0[:, :, pos])


# ---- with the RMSNorm prologue -----------------------------------------------------------------

def _uniform_linear(N, K, seed):
    torch.manual_seed(seed)
    lin = nn.Linear(K, N, bias=False, device=DEV, dtype=BF16)
    with torch.no_grad():
        lin.weight.uniform_(-1 / math.sqrt(K), 1 / math.sqrt(K))
    return lin


@functools.lru_cache(maxsize=None)
def _quantized(kernel, N, K, seed=0):
    from torchao._models.llama.model import _fp8dq_parts, _fp8wo_parts

    lin = _uniform_linear(N, K, seed)
    if kernel == DQ and N % 16:
        # the config leaves a weight whose N is no multiple of 16 unquantized (the reference's
        # scaled-mm rule); the kernels have no such rule: the quantizer and linear ops directly
        q, s = torch.ops.torchao.fp8_quantize_rows(lin.weight.detach())
        s = s.reshape(-1)

        def fwd(x):
            y = torch.ops.torchao.fp8_dyn_linear(x.reshape(1, K), q, s, None)
            return y.reshape(*x.shape[:-1], N)

        return fwd, (q, s)
    if kernel == WO:
        quantize_(lin, Float8WeightOnlyConfig())
        parts = _fp8wo_parts(lin)
    else:
        quantize_(lin, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
        parts = _fp8dq_parts(lin)
    assert parts is not None
    assert parts[0].dtype == FP8 and parts[1].dtype == torch.float32
    assert parts[1].data_ptr() == (lin.weight if kernel == WO else
                                   lin.weight.original_weight_tensor).tensor_impl.scale.data_ptr()
    return lin, parts


@functools.lru_cache(maxsize=None)
def _norm_inputs(K, seed=1):
    """x: integers in [-8, 8] times 2^-2 (sum of squares exact in fp32 in any order, asserted);
    norm weight bf16 in [0.5, 1.5)."""
    assert K * 64 < 2 ** 24 and K <= 16384
    g = torch.Generator().manual_seed(seed)
    xi = torch.randint(-8, 9, (K,), generator=g)
    assert int((xi * xi).sum()) < 2 ** 24
    x = (xi.double() * 0.25).to(BF16)
    assert torch.equal(x.double(), xi.double() * 0.25)
    nw = (torch.rand(K, generator=g) + 0.5).to(BF16)
    return x.view(1, 1, K).to(DEV), nw.to(DEV)


def _fn(kernel):
    from torchao._models.llama import kernels

    return kernels.fp8wo_decode if kernel == WO else kernels.fp8dq_decode


@pytest.mark.parametrize("N", (1000, 6144))
@pytest.mark.parametrize("K", (512, 4096, 8192))
@pytest.mark.parametrize("kernel", [WO, DQ])
def test_rmsnorm_prologue(kernel, N, K):
    """Fused norm + linear against linear(kernels.rmsnorm(x)). On these x the normalised bf16
    token is bit-identical on both sides (see the module docstring); for fp8dq that is what makes
    the bar legitimate, because identical normalised tokens give identical codes and an
    identical token scale, so only the fp32 order of the dot products differs."""
    from torchao._models.llama import kernels

    lin, parts = _quantized(kernel, N, K)
    x, nw = _norm_inputs(K)
    got = _fn(kernel)(x, *parts, norm_weight=nw, eps=EPS)
    assert kernel in _last_kernel()
    ref = lin(kernels.rmsnorm(x, nw, EPS))
    assert got.shape == ref.shape
    r = _rel(got, ref)
    print(f"{kernel} prologue N={N} K={K}: rel {r:.3e}")
    assert r < 2e-3


@pytest.mark.parametrize("kernel", [WO, DQ])
def test_rmsnorm_prologue_four_pieces_per_thread(kernel):
    """One wave per workgroup at K = 2048: four pieces of x and of the norm weight per thread."""
    from torchao._models.llama import kernels

    lin, parts = _quantized(kernel, 1000, 2048)
    x, nw = _norm_inputs(2048)
    with tuning(fp8_gemv=(4, 1, 1)):
        got = _fn(kernel)(x, *parts, norm_weight=nw, eps=EPS)
        assert kernel in _last_kernel()
    assert _rel(got, lin(kernels.rmsnorm(x, nw, EPS))) < 2e-3


@pytest.mark.parametrize("kernel", [WO, DQ])
def test_rmsnorm_prologue_with_epilogues(kernel):
    from torchao._models.llama import kernels

    K = 4096
    x, nw = _norm_inputs(K)
    xn = kernels.rmsnorm(x, nw, EPS)
    lin, parts = _quantized(kernel, 2 * 1024, K, seed=2)
    got = _fn(kernel)(x, *parts, norm_weight=nw, eps=EPS, epilogue="swiglu")
    assert kernel in _last_kernel()
    assert got.shape == (1, 1, 1024)
    assert _rel(got, kernels.silu_mul(lin(xn))) < 2e-3
    H, Hkv, D, T, pos = 32, 8, 128, 64, 17
    lin, parts = _quantized(kernel, (H + 2 * Hkv) * D, K, seed=3)
    freqs = _freqs(H, Hkv, T)
    p = torch.tensor([pos], device=DEV)
    kc, vc = _caches(Hkv, T, seed=1)
    kc_ref, vc_ref = kc.clone(), vc.clone()
    q = _fn(kernel)(x, *parts, norm_weight=nw, eps=EPS, epilogue="rope_kv",
                    rope=(freqs, p, kc, vc, H))
    assert kernel in _last_kernel()
    q_ref = kernels.rope_kv(lin(xn), freqs, p, kc_ref, vc_ref, H)
    for a, b in ((q, q_ref), (kc[:, :, pos], kc_ref[:, :, pos]), (vc[:, :, pos], vc_ref[:, :, pos])):
        assert _rel(a, b) < 2e-3
    rows = [t for t in range(T) if t != pos]
    assert torch.equal(kc[:, :, rows], kc_ref[:, :, rows])  # other rows untouched
    assert torch.equal(vc[:, :, rows], vc_ref[:, :, rows])


def _call(entry, x, w, s, N, K, nw, y, epilogue=0):
    _lib.call(entry, x.data_ptr(), w.data_ptr(), s.data_ptr(), N, K,
              None if nw is None else nw.data_ptr(), EPS, epilogue, y.data_ptr(), None, None, None,
              None, 0, 0, 0, 0, None)


@pytest.mark.parametrize("kernel", [WO, DQ])
def test_norm_prologue_k_limit(kernel):
    """K = 16384 with the norm is served; the next multiple of 32 is refused by the entry's host
    check (no kernel runs) with the documented message."""
    from torchao._models.llama import kernels

    K, N = kernels.FP8_NORM_MAX_K, 64
    assert K == 16384
    entry = "tao_fp8wo_decode_bf16" if kernel == WO else "tao_fp8dq_decode_bf16"
    lin, parts = _quantized(kernel, N, K)
    x, nw = _norm_inputs(K)
    y = torch.empty(1, 1, N, device=DEV, dtype=BF16)
    _call(entry, x, *parts, N, K, nw, y)
    assert kernel in _last_kernel()
    assert _rel(y, lin(kernels.rmsnorm(x, nw, EPS))) < 2e-3
    K2 = K + 32
    w2 = torch.zeros(N, K2, device=DEV, dtype=torch.uint8).view(FP8)
    x2 = torch.ones(K2, device=DEV, dtype=BF16)
    nw2 = torch.ones(K2, device=DEV, dtype=BF16)
    torch.cuda.synchronize()
    before = y.clone()
    with pytest.raises(RuntimeError, match="<= 16384 with norm_weight"):
        _call(entry, x2, w2, parts[1], N, K2, nw2, y)
    _call(entry, x2, w2, parts[1], N, K2, None, y)  # without the norm the same K is served
    torch.cuda.synchronize()
    assert not torch.equal(y, before)  # (zero codes: y is now all zero)
    assert not y.any()


# ---- errors, graph capture, the KV guard ---------------------------------------------------------

@pytest.mark.parametrize("kernel", [WO, DQ])
def test_graph_capture_errors_and_kv_guard(kernel):
    from torchao._models.llama import kernels

    N, K = 6144, 4096
    entry = "tao_fp8wo_decode_bf16" if kernel == WO else "tao_fp8dq_decode_bf16"
    fn = _fn(kernel)
    lin, parts = _quantized(kernel, N, K, seed=3)
    x, nw = _norm_inputs(K)
    eager = fn(x, *parts, norm_weight=nw, eps=EPS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(x, *parts, norm_weight=nw, eps=EPS)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = fn(x, *parts, norm_weight=nw, eps=EPS)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    with pytest.raises(RuntimeError, match="one token"):
        fn(torch.zeros(2, K, device=DEV, dtype=BF16), *parts)
    with pytest.raises(RuntimeError, match="epilogue"):
        _call(entry, x, *parts, N, K, None, eager, epilogue=7)
    if kernel == WO:
        w3 = torch.zeros(N, 1040, device=DEV, dtype=torch.uint8).view(FP8)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            fn(torch.zeros(1, 1040, device=DEV, dtype=BF16), w3, parts[1])
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        fn(x, parts[0].view(torch.int8), parts[1])
    with pytest.raises(RuntimeError, match="float32"):
        fn(x, parts[0], parts[1].to(BF16))
    with pytest.raises(RuntimeError, match="scales for"):
        fn(x, parts[0], parts[1][:-1].contiguous())
    with pytest.raises(RuntimeError, match="norm_weight"):
        fn(x, *parts, norm_weight=nw.float(), eps=EPS)
    # a KV position past the cache: no row written, reported once by tao_decode_status
    H, Hkv, D, T = 32, 8, 128, 16
    freqs = _freqs(H, Hkv, 64)
    kc = torch.zeros(1, Hkv, T, D, device=DEV, dtype=BF16)
    vc = torch.zeros_like(kc)
    kernels.check_decode_status()  # clear
    fn(x, *parts, epilogue="rope_kv", rope=(freqs, torch.tensor([T], device=DEV), kc, vc, H))
    assert kernel in _last_kernel()
    torch.cuda.synchronize()
    assert not kc.any() and not vc.any()
    with pytest.raises(RuntimeError, match="past the KV cache"):
        kernels.check_decode_status()
    kernels.check_decode_status()  # read and cleared: clean afterwards


@pytest.mark.parametrize("kernel", [WO, DQ])
def test_parts_on_the_gpu(kernel):
    """The weight criteria with the device test satisfied: a bias, or a scale cast to bf16 (a
    per-call cast would be needed), sends the linear to the regular path."""
    from torchao._models.llama.model import (_fp8dq_parts, _fp8wo_parts, _int4_parts,
                                              _int8dq_parts, _int8wo_parts)

    parts_fn, other = (_fp8wo_parts, _fp8dq_parts) if kernel == WO else (_fp8dq_parts, _fp8wo_parts)
    cfg = (Float8WeightOnlyConfig() if kernel == WO else
           Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
    lin = _uniform_linear(64, 128, 0)
    quantize_(lin, cfg)
    assert parts_fn(lin) is not None and other(lin) is None
    assert _int4_parts(lin) is None and _int8wo_parts(lin) is None and _int8dq_parts(lin) is None
    biased = nn.Linear(128, 64, bias=True, device=DEV, dtype=BF16)
    quantize_(biased, cfg)
    assert parts_fn(biased) is None
    inner = lin.weight if kernel == WO else lin.weight.original_weight_tensor
    inner.tensor_impl.scale = inner.tensor_impl.scale.to(BF16)
    assert parts_fn(lin) is None


# ---- in the harness ---------------------------------------------------------------------------------

def _tiny_model(quant):
    from torchao._models.llama.generate import apply_quantization
    from torchao._models.llama.model import ModelArgs, Transformer

    torch.manual_seed(2)
    model = Transformer(ModelArgs(dim=512, n_layer=2, n_head=4, n_local_heads=2, vocab_size=1000,
                                  block_size=256)).to(DEV).to(BF16)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, nn.Linear):
                b = 1 / math.sqrt(mod.in_features)
                mod.weight.uniform_(-b, b)
        for blk in model.layers:
            blk.attention_norm.weight.uniform_(0.5, 1.5)
            blk.ffn_norm.weight.uniform_(0.5, 1.5)
    model.eval().fuse_w13()
    return apply_quantization(model, quant)


def _step(model, prompt, P, T, fused):
    """Prefill, then the logits of one decode step at position P."""
    pos = torch.arange(P, device=DEV)
    model.setup_caches(1, P + T)
    assert model.enable_fused_kernels(fused) == fused
    with torch.no_grad():
        model(prompt, pos)
        return model(prompt[:, -1:], torch.tensor([P], device=DEV))


@pytest.mark.parametrize("quant", ["float8wo", "float8dq-row"])
def test_fused_fp8_decode_in_the_harness(quant, monkeypatch):
    """A tiny Llama on the float8 configs through apply_quantization: the one-token step is
    routed to the fused float8 kernels (norms, RoPE + KV write and SwiGLU inside the GEMVs), a
    HIP-graph decode equals the eager one, and the fused logits track the torch-op step's.

    float8wo: only summation order differs between the two steps: rel-L2 < 2e-2, the bar of
    the int8 harness test. float8dq-row: a real-valued hidden state can move a bf16 ulp through
    the norm's sum order, which can move the token's scale and a few percent of its codes, so both
    steps are compared with the unquantised bf16 model of the same seed instead:
    d_fused <= 1.25 d_ops (the two paths differ in rounding order inside one quantisation grid,
    which perturbs the quantisation error by a fraction of itself)."""
    from torchao._models.llama import kernels, model as M
    from torchao._models.llama.generate import GraphDecoder, generate, prefill

    kernel = WO if quant == "float8wo" else DQ
    name = "fp8wo_decode" if quant == "float8wo" else "fp8dq_decode"
    model = _tiny_model(quant)
    parts_fn = M._fp8wo_parts if quant == "float8wo" else M._fp8dq_parts
    fusable = [blk.attention.wqkv for blk in model.layers]
    fusable += [blk.feed_forward.w13 for blk in model.layers] + [model.output]
    expected = sum(parts_fn(lin) is not None for lin in fusable)
    # (vocab 1000 is no multiple of 16: the float8dq config leaves the head unquantized)
    assert expected == (5 if quant == "float8wo" else 4)
    P, T = 9, 12
    torch.manual_seed(5)
    prompt = torch.randint(0, 1000, (1, P), device=DEV)
    ops = _step(model, prompt, P, T, fused=False)
    seen = []
    real = getattr(kernels, name)

    def spy(*a, **k):
        y = real(*a, **k)
        seen.append(_last_kernel())
        return y

    model.setup_caches(1, P + T)
    assert model.enable_fused_kernels()
    with torch.no_grad():
        model(prompt, torch.arange(P, device=DEV))
        monkeypatch.setattr(kernels, name, spy)
        got = model(prompt[:, -1:], torch.tensor([P], device=DEV))
        monkeypatch.setattr(kernels, name, real)
    assert len(seen) == expected and all(kernel in k for k in seen), seen
    if quant == "float8wo":
        assert kernel in _last_kernel()  # the head GEMV, the step's last launch
        r = _rel(got, ops)
        print(f"float8wo fused vs torch-op step: rel {r:.3e}")
        assert r < 2e-2
    else:
        ref = _step(_tiny_model(None), prompt, P, T, fused=False)
        d_fused, d_ops = _rel(got, ref), _rel(ops, ref)
        print(f"float8dq-row vs bf16 model: d_fused {d_fused:.4e} d_ops {d_ops:.4e} "
              f"ratio {d_fused / d_ops:.3f}")
        assert d_fused <= 1.25 * d_ops
    pos = torch.arange(P, device=DEV)
    eager, _, _ = generate(model, prompt, T, None)
    dec = GraphDecoder(model, 1, P + T, DEV)
    dec.reset(prompt, prefill(model, prompt, pos))
    dec.capture()
    graphed, _, _ = generate(model, prompt, T, dec)
    assert torch.equal(graphed, eager)
    kernels.check_decode_status()
