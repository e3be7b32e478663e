"""What the dispatcher ops of the NF4, FP6 and uintx weight-only linears refuse around their weight
checks (x, bias), message for message, which of two faults is reported, the empty call, and the
bias on the GEMV route and on the dequantize + matmul route. Bit-exactness against the formulas
is the job of the test_gpu_exact_* suites; here the smallest weight each format accepts is enough."""

import pytest
import torch

from torchao import _lib
from torchao.kernel.tuning import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
N = 16
SAME_DEVICE = "bias is on cpu but x is on cuda:0: all operands must be on the same device"


def _weights():
    """op name -> (K, call(x, bias), tuning knob, its arguments after the route, GEMV kernel)."""
    torch.manual_seed(0)
    bf = torch.bfloat16
    # NF4, N = 16, K = 64: 512 code bytes, 16 block scalers, one factor, the mean, 16 levels
    nf4 = (torch.randint(0, 256, (512,), dtype=torch.uint8).to(DEV),
           torch.randint(-127, 128, (16,), dtype=torch.int8).to(DEV),
           torch.rand(1).to(bf).to(DEV), torch.rand(1).to(bf).to(DEV),
           torch.linspace(-1, 1, 16).to(bf).to(DEV))
    # FP6 (e3m2), N = 16, K = 64: two 32-code groups of 6 dwords per row
    fp6 = (torch.randint(-2 ** 31, 2 ** 31, (N, 12), dtype=torch.int64).to(torch.int32).to(DEV),
           (0.5 + torch.rand(N)).to(bf).to(DEV))
    # uint3, N = 16, K = 128, group 32: the 2-bit and the 1-bit shard, 64 (scale, zero point) pairs
    u3 = (torch.randint(0, 256, (N, 32), dtype=torch.uint8).to(DEV),
          torch.randint(0, 256, (N, 16), dtype=torch.uint8).to(DEV),
          (0.5 + torch.rand(64)).to(bf).to(DEV),
          torch.randint(0, 8, (64,), dtype=torch.int32).to(DEV))
    return {
        "nf4_linear": (64, lambda x, b: T.nf4_linear(x, *nf4, N, b), "nf4", (0, 0, 0, 0),
                       "nf4_gemv_kernel", "nf4_dequant_kernel"),
        "fp6_weight_only_linear": (64, lambda x, b: T.fp6_weight_only_linear(x, *fp6, 3, 2, b),
                                   "fp6", (0, 0, 0, 0, 0), "fp6wo_gemv_kernel",
                                   "fp6_dequant_kernel"),
        "uintx_weight_only_linear": (
            128, lambda x, b: T.uintx_weight_only_linear(x, None, u3[0], u3[1], u3[2], u3[3], 3, 32,
                                                         b),
            "uintx", (0, 0, 0, 0, 0, 0), "uintx_gemv_kernel", "uintx_dequant_kernel"),
    }


@pytest.fixture(scope="module")
def weights():
    return _weights()


OPS = ("nf4_linear", "fp6_weight_only_linear", "uintx_weight_only_linear")


def _message(call, x, bias):
    with pytest.raises(RuntimeError) as e:
        call(x, bias)
    return str(e.value).splitlines()[0]


@pytest.mark.parametrize("op", OPS)
def test_refusals(weights, op):
    K, call = weights[op][:2]
    x = torch.randn(3, K, dtype=torch.bfloat16, device=DEV)
    ok_bias = torch.randn(N, dtype=torch.bfloat16, device=DEV)
    long_bias = torch.randn(N + 1, dtype=torch.bfloat16, device=DEV)
    wide = torch.randn(3, K + 64, dtype=torch.bfloat16, device=DEV)
    assert _message(call, x.half(), None) == f"{op} (HIP) needs bf16 x, got Half"
    if op != "nf4_linear":  # NF4 takes K from x: a wider x is another weight
        assert _message(call, wide, None) == f"x last dim {K + 64} != K {K}"
    assert _message(call, x, long_bias) == f"{op}: bias must have N = {N} elements"
    assert _message(call, x, ok_bias.cpu()) == SAME_DEVICE
    # two faults at once: the one that is reported
    assert _message(call, x.half(), ok_bias.cpu()) == f"{op} (HIP) needs bf16 x, got Half"
    assert _message(call, x, long_bias.cpu()) == f"{op}: bias must have N = {N} elements"
    if op != "nf4_linear":
        assert _message(call, wide, long_bias) == f"x last dim {K + 64} != K {K}"
        assert _message(call, wide.half(), None) == f"{op} (HIP) needs bf16 x, got Half"
    # no rows: an empty result of the right shape, with and without a bias
    for b in (None, ok_bias):
        y = call(x[:0], b)
        assert y.shape == (0, N) and y.dtype == torch.bfloat16 and y.device == x.device
    assert call(x.reshape(3, 1, K)[:0], None).shape == (0, 1, N)


@pytest.mark.parametrize("op", OPS)
def test_bias_on_both_routes(weights, op):
    K, call, knob, rest, gemv, dequant = weights[op]
    x = torch.randn(3, K, dtype=torch.bfloat16, device=DEV)
    bias = (1 + torch.rand(N, device=DEV)).to(torch.bfloat16)
    last = _lib.lib().tao_last_kernel
    for route, kernel in ((1, gemv), (2, dequant)):
        with tuning(**{knob: (route, *rest)}):
            y = call(x, bias)
            assert last().decode() == kernel  # the route's own launch (2: the matmul is torch's)
            again = call(x, bias)
            plain = call(x, None)
        assert y.shape == (3, N) and torch.equal(y, again)
        assert not torch.equal(y, plain)  # the bias was added
        assert torch.isfinite(y.float()).all()
