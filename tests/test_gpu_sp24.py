"""Bit-exact GPU tests of the 2:4 sparse int8 linear (Int8DynamicActivationInt8WeightConfig with
SemiSparseLayout): the compress / decompress kernels, torch.ops.torchao.int8_sp24_scaled_mm on both
routes (the sparse GEMV and the sparse MFMA GEMM), the fused one-token int8_sp24_dyn_linear, and
quantize_ end to end.

The references are the ops' plain-torch definitions on the CPU (an exact integer product, then
bf16(bf16(bf16(acc) * xs) * ws) (+ bias) in torch bf16 ops) and the dense int8_scaled_mm on the
decompressed weight. Every partial sum on the GPU is an integer, so no route, reduction order or
split can change a bit: every check is torch.equal, there is no tolerance anywhere."""

import copy
import functools

import pytest
import torch

from torchao import _lib
from torchao.dtypes import SemiSparseAQTTensorImpl, SemiSparseLayout
from torchao.kernel import tuning
from torchao.quantization import Int8DynamicActivationInt8WeightConfig, quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
GEMV, GEMM = 1, 2


def _prune(w):
    """pre_process's rule on int8 codes."""
    return SemiSparseLayout().pre_process(w.float()).to(torch.int8)


@functools.lru_cache(maxsize=None)
def _weight(N, K):
    """Random codes in [-127, 127] pruned 2:4, with the edge groups: empty, one nonzero at every
    position, all six position pairs."""
    g = torch.Generator().manual_seed(100 * N + K)
    w = _prune(torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8))
    edge = [[0, 0, 0, 0], [5, 0, 0, 0], [0, -6, 0, 0], [0, 0, 7, 0], [0, 0, 0, -127],
            [1, 2, 0, 0], [1, 0, 2, 0], [1, 0, 0, 2], [0, 1, 2, 0], [0, 1, 0, 2], [0, 0, 1, 2]]
    w[N - 1, :44] = torch.tensor(edge, dtype=torch.int8).reshape(-1)
    ws = (torch.rand(N, generator=g) * 0.02 + 0.001).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    values, meta, err = T.int8_sp24_compress(w)
    assert int(err) == 0
    return w, values, meta, ws, bias


@functools.lru_cache(maxsize=None)
def _acts(M, K):
    g = torch.Generator().manual_seed(7 * M + K)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    xs = (torch.rand(M, 1, generator=g) * 0.05 + 0.001).to(torch.bfloat16)
    return xq, xs


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("N", [5, 80])
def test_compress_decompress_kernels_equal_the_definitions(N, K):
    w, values, meta, _, _ = _weight(N, K)
    v, m, err = T.int8_sp24_compress(w.to(DEV))
    assert torch.equal(v.cpu(), values) and torch.equal(m.cpu(), meta) and int(err) == 0
    assert torch.equal(T.int8_sp24_decompress(v, m).cpu(), w)
    bad = w.clone()
    bad[N // 2, K - 4:] = torch.tensor([1, 0, 2, 3], dtype=torch.int8)
    assert int(T.int8_sp24_compress(bad.to(DEV))[2]) == 1
    with pytest.raises(ValueError, match="2:4"):
        SemiSparseAQTTensorImpl.from_plain(bad.to(DEV), torch.ones(N), None, SemiSparseLayout())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M", [1, 2, 4, 5, 16, 17, 33])
@pytest.mark.parametrize("K", [128, 384, 2176])
@pytest.mark.parametrize("N", [16, 80])
def test_scaled_mm_equals_definition_and_dense_op_on_both_routes(N, K, M, with_bias):
    w, values, meta, ws, bias = _weight(N, K)
    xq, xs = _acts(M, K)
    b = bias if with_bias else None
    ref = T.int8_sp24_scaled_mm(xq, xs, values, meta, ws, b)  # the CPU definition
    d = [t.to(DEV) for t in (xq, xs, values, meta, ws)]
    bd = None if b is None else b.to(DEV)
    dense = T.int8_scaled_mm(d[0], d[1], T.int8_sp24_decompress(d[2], d[3]), d[4], bd)
    assert torch.equal(dense.cpu(), ref)
    auto = GEMV if M <= 2 else GEMM
    assert _lib.lib().tao_int8_sp24_route(M, N, K) == auto
    for route in (GEMV, GEMM):
        with tuning(sp24=(route, 0, 0, 0, 0)):
            y = T.int8_sp24_scaled_mm(*d, bd)
            kernel = _lib.lib().tao_last_kernel().decode()
        assert kernel == ("sp24_gemv_kernel" if route == GEMV else "sp24_gemm_kernel")
        assert torch.equal(y.cpu(), ref), f"route {route}"
    assert torch.equal(T.int8_sp24_scaled_mm(*d, bd).cpu(), ref)


# (bm, waves of 16 features per k-group, most k-groups): every NWV with every BM, one and several
# k-groups; N = 80 leaves a partial workgroup at NWV = 2 and 4, M = 33 a row tail at every BM
@pytest.mark.parametrize("shape", [(16, 2, 0), (16, 4, 2), (32, 1, 8), (32, 2, 3), (32, 4, 1),
                                   (64, 1, 3), (64, 2, 4), (64, 4, 2)])
def test_gemm_forced_launch_shapes(shape):
    N, K, M = 80, 2176, 33
    _, values, meta, ws, bias = _weight(N, K)
    xq, xs = _acts(M, K)
    ref = T.int8_sp24_scaled_mm(xq, xs, values, meta, ws, bias)
    with tuning(sp24=(GEMM, 0, 0, 0, 0), sp24_gemm=shape):
        y = T.int8_sp24_scaled_mm(*[t.to(DEV) for t in (xq, xs, values, meta, ws, bias)])
    assert torch.equal(y.cpu(), ref)


# (tokens, rows per wave, waves along K, row groups): the tuned one-token tiles, and fewer waves
# along K than slices (2176 k is two slices, 4224 three) with several row groups
@pytest.mark.parametrize("M, rpw, wk, g", [(1, 2, 0, 0), (1, 8, 1, 4), (2, 0, 1, 2), (4, 0, 2, 4),
                                           (8, 0, 1, 8)])
def test_gemv_forced_launch_shapes(M, rpw, wk, g):
    N, K = 80, 2176
    _, values, meta, ws, bias = _weight(N, K)
    xq, xs = _acts(M, K)
    ref = T.int8_sp24_scaled_mm(xq, xs, values, meta, ws, bias)
    with tuning(sp24=(GEMV, 0, rpw, wk, g)):
        y = T.int8_sp24_scaled_mm(*[t.to(DEV) for t in (xq, xs, values, meta, ws, bias)])
    assert torch.equal(y.cpu(), ref)
    if M == 1:  # the fused launch on the same tuned tile
        _, dv, dm, dws, db = [t.to(DEV) for t in _weight(N, 4224)]
        x = torch.randn(1, 4224, generator=torch.Generator().manual_seed(rpw)).to(torch.bfloat16)
        q, s = T.int8_quantize_per_token(x.to(DEV))
        with tuning(sp24=(0, 0, rpw, wk, g)):
            assert torch.equal(T.int8_sp24_dyn_linear(x.to(DEV), dv, dm, dws, db),
                               T.int8_sp24_scaled_mm(q, s, dv, dm, dws, db))


def test_gemv_tokens_up_to_the_lds_limit_then_the_gemm():
    """Two tokens of K = 32256 are the most the GEMV stages (63 KiB + partials inside the 64 KiB
    of dynamic LDS); K = 32768 goes to the GEMM, and a forced GEMV is refused, not launched."""
    N, M = 16, 2
    for K, kernel in ((32256, "sp24_gemv_kernel"), (32768, "sp24_gemm_kernel")):
        _, values, meta, ws, bias = _weight(N, K)
        xq, xs = _acts(M, K)
        ref = T.int8_sp24_scaled_mm(xq, xs, values, meta, ws, bias)
        d = [t.to(DEV) for t in (xq, xs, values, meta, ws, bias)]
        y = T.int8_sp24_scaled_mm(*d)
        assert _lib.lib().tao_last_kernel().decode() == kernel
        assert torch.equal(y.cpu(), ref)
    with tuning(sp24=(GEMV, 0, 0, 0, 0)), pytest.raises(RuntimeError, match="tokens in LDS"):
        T.int8_sp24_scaled_mm(*d)


@pytest.mark.parametrize("route", [GEMV, GEMM])
def test_k_map_in_one_shot(route):
    """xq = 127 I with unit scales: acc[m][n] = 127 w[n][m], so a misplaced value, index bit or x
    byte is a wrong element."""
    N, K = 80, 128
    w, values, meta, _, _ = _weight(N, K)
    xq = 127 * torch.eye(K, dtype=torch.int8)
    one_m, one_n = torch.ones(K, 1, dtype=torch.bfloat16), torch.ones(N, dtype=torch.bfloat16)
    ref = (127 * w.t().to(torch.int32)).to(torch.bfloat16)
    with tuning(sp24=(route, 0, 0, 0, 0)):
        y = T.int8_sp24_scaled_mm(*[t.to(DEV) for t in (xq, one_m, values, meta, one_n)])
    assert torch.equal(y.cpu(), ref)


@pytest.mark.parametrize("K", [128, 4224])
def test_dyn_linear_one_launch_equals_quantizer_then_scaled_mm(K):
    N = 80
    _, values, meta, ws, bias = [t.to(DEV) for t in _weight(N, K)]
    x = torch.randn(1, K, generator=torch.Generator().manual_seed(K)).to(torch.bfloat16).to(DEV)
    q, s = T.int8_quantize_per_token(x)
    ref = T.int8_sp24_scaled_mm(q, s, values, meta, ws, bias)
    y = T.int8_sp24_dyn_linear(x, values, meta, ws, bias)
    assert _lib.lib().tao_last_kernel().decode() == "sp24_gemv_fq_kernel"
    assert torch.equal(y, ref)


def test_quantize_stack_equals_plain_config_on_pruned_weights_and_graph_replays():
    torch.manual_seed(3)
    base = torch.nn.Sequential(torch.nn.Linear(128, 80), torch.nn.ReLU(),
                               torch.nn.ConstantPad1d((0, 48), 0.0), torch.nn.Linear(128, 80))
    base = base.to(torch.bfloat16).to(DEV)
    sparse, plain = copy.deepcopy(base), copy.deepcopy(base)
    for lin in (plain[0], plain[3]):
        lin.weight.data = SemiSparseLayout().pre_process(lin.weight.data)
    quantize_(sparse, Int8DynamicActivationInt8WeightConfig(layout=SemiSparseLayout()))
    quantize_(plain, Int8DynamicActivationInt8WeightConfig())
    x1 = torch.randn(1, 128, device=DEV).to(torch.bfloat16)
    x16 = torch.randn(16, 128, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        y1 = sparse(x1)
        assert _lib.lib().tao_last_kernel().decode() == "sp24_gemv_fq_kernel"
        assert torch.equal(y1, plain(x1))
        eager = sparse(x16)
        assert torch.equal(eager, plain(x16))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = sparse(x16)
        for _ in range(3):
            y.zero_()
            graph.replay()
            assert torch.equal(y, eager)


def test_opcheck():
    w, values, meta, ws, bias = [t.to(DEV) for t in _weight(16, 128)]
    xq, xs = [t.to(DEV) for t in _acts(5, 128)]
    x = torch.randn(1, 128, device=DEV).to(torch.bfloat16)
    torch.library.opcheck(T.int8_sp24_compress.default, (w,))
    torch.library.opcheck(T.int8_sp24_decompress.default, (values, meta))
    torch.library.opcheck(T.int8_sp24_scaled_mm.default, (xq, xs, values, meta, ws, bias))
    torch.library.opcheck(T.int8_sp24_dyn_linear.default, (x, values, meta, ws, bias))
