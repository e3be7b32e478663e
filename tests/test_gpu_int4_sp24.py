"""GPU tests of the 2:4 sparse int4 weight-only linear (Int4WeightOnlyConfig with
MarlinSparseLayout): the compress / decompress kernels against their plain-torch definitions, the
linear on both routes (the sparse GEMV and the GEMM on v_smfmac_f32_16x16x64_bf16) against the
float64 formula

    y[m][n] = bf16( sum_g s[g][n] * sum_{k in g} x[m][k] (q[n][k] - 8) + bias[n] )

bit for bit on exact inputs (small-integer x, power-of-two scales, integer bias: every fp32 partial
sum is exact in any order) and within the project's rel-L2 bar on random data, and quantize_ end to
end under a captured graph."""

import copy
import functools

import pytest
import torch

from exact_inputs import describe_mismatch, make_q, round_bf16_once
from torchao import _lib
from torchao.dtypes import MarlinSparseAQTTensorImpl, MarlinSparseLayout
from torchao.kernel import tuning
from torchao.quantization import Int4WeightOnlyConfig, quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
GEMV, GEMM = 1, 2
KERNEL = {GEMV: "int4_sp24_gemv_kernel", GEMM: "int4_sp24_gemm_kernel"}
BOUNDARY = 4  # kI4Sp24GemvDefaultMaxM, the measured GEMV / GEMM boundary
BAR = 4e-3    # rel-L2 against float64 on the same codes (tests/test_gpu_mxfp4.py)
# groups with 0, 1 and 2 kept codes, every position and every position pair
EDGE = [[8, 8, 8, 8], [5, 8, 8, 8], [8, 0, 8, 8], [8, 8, 15, 8], [8, 8, 8, 7],
        [1, 2, 8, 8], [1, 8, 2, 8], [1, 8, 8, 2], [8, 1, 2, 8], [8, 1, 8, 2], [8, 8, 1, 2]]


@functools.lru_cache(maxsize=None)
def _weight(N, K, g):
    """Uniform codes pruned 2:4 (code 8 = zero) with the edge groups, compressed on the CPU;
    power-of-two scales [K/g, N], integer bias."""
    gen = torch.Generator().manual_seed(100 * N + K + g)
    q = (MarlinSparseLayout().pre_process((make_q(N, K, 5) - 8).float()) + 8).to(torch.int32)
    q[N - 1, :44] = torch.tensor(EDGE, dtype=torch.int32).reshape(-1)
    values, meta, err = T.int4_sp24_compress(q)
    assert int(err) == 0
    scale = (2.0 ** torch.randint(-3, 2, (K // g, N), generator=gen)).to(torch.bfloat16)
    bias = torch.randint(-8, 9, (N,), generator=gen).to(torch.bfloat16)
    return q, values, meta, scale, bias


@functools.lru_cache(maxsize=None)
def _x(M, K):
    gen = torch.Generator().manual_seed(7 * M + K)
    return torch.randint(-4, 5, (M, K), generator=gen).to(torch.bfloat16)


def _formula(x, q, scale, g, bias):
    """The float64 formula, [M, N], before the one rounding."""
    w = (q - 8).double() * scale.t().double().repeat_interleave(g, 1)
    y = x.double() @ w.t()
    return y if bias is None else y + bias.double()


@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("N", [5, 40])
def test_compress_decompress_kernels_equal_the_definitions(N, K):
    q, values, meta, _, _ = _weight(N, K, 128)
    v, m, err = T.int4_sp24_compress(q.to(DEV))
    assert torch.equal(v.cpu(), values) and torch.equal(m.cpu(), meta) and int(err) == 0
    assert torch.equal(T.int4_sp24_decompress(v, m).cpu(), q)
    bad = q.clone()
    bad[N // 2, K - 4:] = torch.tensor([1, 8, 2, 3], dtype=torch.int32)
    assert int(T.int4_sp24_compress(bad.to(DEV))[2]) == 1
    with pytest.raises(ValueError, match="2:4"):
        MarlinSparseAQTTensorImpl.from_plain(
            bad.to(DEV), torch.ones(N, 1), torch.full((N, 1), 8.0), MarlinSparseLayout())


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("M", [1, 2, BOUNDARY, BOUNDARY + 1, 16, 17, 33])
@pytest.mark.parametrize("K", [128, 384, 4224])
@pytest.mark.parametrize("N", [16, 40])
def test_linear_is_the_formula_bit_for_bit_on_exact_inputs(N, K, M, per_channel, with_bias):
    g = K if per_channel else 128
    q, values, meta, scale, bias = _weight(N, K, g)
    b = bias if with_bias else None
    ref = round_bf16_once(_formula(_x(M, K), q, scale, g, b))
    route = GEMV if M <= BOUNDARY else GEMM
    assert _lib.lib().tao_int4_sp24_route(M, N, K) == route
    y = T.int4_sp24_weight_only_linear(
        _x(M, K).to(DEV), values.to(DEV), meta.to(DEV), scale.to(DEV), g,
        None if b is None else b.to(DEV))
    assert _lib.lib().tao_last_kernel().decode() == KERNEL[route]
    assert torch.equal(y.cpu(), ref), describe_mismatch(KERNEL[route], y.cpu(), ref)


# route, then (tokens per tile, waves of 16 features per k-group, most k-groups) of the GEMM: both
# routes at M = 2, every BM with NWV > 1 (N = 40 leaves a partial workgroup) and several k-groups
@pytest.mark.parametrize("M, route, shape", [(2, GEMV, (0, 0, 0)), (2, GEMM, (0, 0, 0)),
                                             (33, GEMM, (16, 4, 2)), (33, GEMM, (32, 2, 3)),
                                             (33, GEMM, (64, 4, 2))])
def test_forced_routes_and_gemm_shapes_agree(M, route, shape):
    N, K, g = 40, 4224, 128
    q, values, meta, scale, bias = _weight(N, K, g)
    ref = round_bf16_once(_formula(_x(M, K), q, scale, g, bias))
    with tuning(int4_sp24=(route, 0, 0, 0, 0) + shape):
        y = T.int4_sp24_weight_only_linear(
            *[t.to(DEV) for t in (_x(M, K), values, meta, scale)], g, bias.to(DEV))
        assert _lib.lib().tao_last_kernel().decode() == KERNEL[route]
    assert torch.equal(y.cpu(), ref), describe_mismatch(KERNEL[route], y.cpu(), ref)


@functools.lru_cache(maxsize=None)
def _random_module():
    torch.manual_seed(11)
    m = torch.nn.Linear(512, 48).to(torch.bfloat16).to(DEV)
    quantize_(m, Int4WeightOnlyConfig(group_size=128, layout=MarlinSparseLayout()))
    return m, copy.deepcopy(m).to("cpu")


@pytest.mark.parametrize("M", [1, 5, 40])
def test_random_data_within_the_bar_of_float64_and_of_the_cpu_path(M):
    m, m_cpu = _random_module()
    x = torch.randn(M, 512, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu().double()
        oracle = m_cpu(x).double()
    q, scale, _ = m_cpu.weight.tensor_impl.get_plain()
    ref = _formula(x, q, scale.t(), 128, m_cpu.bias.detach())
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print(f"M={M}: rel-L2 vs float64 {rel(y, ref):.3e}, vs the CPU path {rel(y, oracle):.3e}")
    assert rel(y, ref) <= BAR and rel(y, oracle) <= BAR


def test_quantized_stack_replays_under_a_captured_graph():
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.ReLU(),
                                torch.nn.Linear(128, 40)).to(torch.bfloat16).to(DEV)
    quantize_(model, Int4WeightOnlyConfig(group_size=128, layout=MarlinSparseLayout()))
    assert isinstance(model[0].weight.tensor_impl, MarlinSparseAQTTensorImpl)
    for M in (1, 16):  # the GEMV and the GEMM
        x = torch.randn(M, 256, device=DEV).to(torch.bfloat16)
        with torch.no_grad():
            eager = model(x)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y = model(x)
            for _ in range(3):
                y.zero_()
                graph.replay()
                assert torch.equal(y, eager)


def test_opcheck():
    q, values, meta, scale, bias = [t.to(DEV) for t in _weight(16, 128, 128)]
    torch.library.opcheck(T.int4_sp24_compress.default, (q,))
    torch.library.opcheck(T.int4_sp24_decompress.default, (values, meta))
    torch.library.opcheck(T.int4_sp24_weight_only_linear.default,
                          (_x(5, 128).to(DEV), values, meta, scale, 128, bias))
