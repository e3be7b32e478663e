"""GPU tests of the NVFP4 linear's MFMA route: the Nvfp4WO policy of gemm_mfma_kernel, reached with
tuning(nvfp4_mfma=1) through torch.ops.torchao.nvfp4_linear and F.linear on an NVFP4Tensor.

Exact inputs (``_exact``): arbitrary code bytes, scale bytes of the e4m3 values k/8 * 2^e (k = 8..15,
e = 0, 1), integer x in [-4, 4] and bias in [-8, 8], per-tensor scale absent or 2^-3. Every product is
a multiple of 1/16 of magnitude at most 90, so for K <= 8256 every partial sum in any order is exact
in fp32 and the output must equal the float64 result, rounded once to bf16, bit for bit: no tolerance.
M = 5, 17, 65: a partial 16-row tile, a tile plus a row, a second 64-row block; N = 48, 144: a partial
workgroup, across a 128-row tile of the swizzled scales; K = 64, 320, 2112, 8256: less than a 256-k
step, a step plus a tail, eight steps plus a tail, split-K."""

import functools

import numpy as np
import pytest
import torch

from conftest import bf16, golden_files, load_golden

from torchao import _lib
from torchao.kernel.tuning import tuning
from torchao.prototype.mx_formats import NVFP4InferenceConfig, NVFP4MMConfig
from torchao.prototype.mx_formats.utils import to_blocked
from torchao.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
BAR64 = 4e-3  # tests/test_gpu_nvfp4.py's bar for this linear against float64
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                    dtype=torch.float64)
LAYOUTS = pytest.mark.parametrize("swizzled", [False, True], ids=["rowmajor", "swizzled"])


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=32)
def _exact(M, N, K):
    """Device inputs and, per (bias, per-tensor scale) choice, the expected bf16 output."""
    g = torch.Generator().manual_seed((M * 31 + N * 7 + K) % 1000)
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    sb = (56 + torch.randint(0, 16, (N, K // 16), generator=g)).to(torch.uint8)  # (1 + m/8) 2^e
    x = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
    bias = torch.randint(-8, 9, (N,), generator=g).to(torch.bfloat16)
    codes = torch.stack([q >> 4, q & 0xF], -1).reshape(N, K).long()  # element 2 j: the high nibble
    scale = sb.view(torch.float8_e4m3fn).double()
    assert scale.min() >= 1 and scale.max() <= 3.75
    assert 4 * 6 * 3.75 * 16 * K < 2 ** 24  # every partial sum, in any order, is exact in fp32
    acc = x.double() @ (E2M1[codes] * scale.repeat_interleave(16, 1)).t()
    want = {}
    for has_bias in (False, True):
        for alpha in (None, 0.125):
            r = acc * (alpha or 1.0) + (bias.double() if has_bias else 0.0)
            assert torch.equal(r.float().double(), r)  # fp32 holds it: bf16 is the one rounding
            want[has_bias, alpha] = r.float().to(torch.bfloat16)
    scales = {False: sb.reshape(-1).to(DEV), True: to_blocked(sb).reshape(-1).to(DEV)}
    return x.to(DEV), q.to(DEV), scales, bias.to(DEV), want


def check(what, M, N, K, swizzled):
    """With and without bias and per-tensor scale, under the tuning the caller has set."""
    x, q, scales, bias, want = _exact(M, N, K)
    for (has_bias, alpha), ref in want.items():
        pts = None if alpha is None else torch.tensor([alpha], device=DEV)
        got = T.nvfp4_linear(x, q, scales[swizzled], pts, bias if has_bias else None, swizzled,
                             False, None).cpu()
        assert _last_kernel() == "gemm_mfma_kernel", (what, _last_kernel())
        assert torch.equal(got, ref), (what, M, N, K, swizzled, has_bias, alpha,
                                       (got != ref).nonzero()[:4].tolist())


@LAYOUTS
@pytest.mark.parametrize("N,K", [(48, 64), (48, 320), (144, 2112), (48, 8256)])
@pytest.mark.parametrize("M", (5, 17, 65))
def test_mfma_route_exact(M, N, K, swizzled):
    with tuning(nvfp4_mfma=1):
        check("nvfp4 mfma", M, N, K, swizzled)


@pytest.mark.parametrize("nw", (1, 2))
@pytest.mark.parametrize("splits", (1, 3))
@pytest.mark.parametrize("bm,kg", [(16, 1), (16, 2), (16, 4), (32, 2), (64, 1)])
def test_forced_launch_shapes(bm, kg, splits, nw):
    # the policy is built for every shape the launcher names: none of these is refused
    with tuning(gemm=(bm, kg, splits), gemm_nw=nw, nvfp4_mfma=1):
        for swizzled in (False, True):
            check(f"nvfp4 mfma forced {bm}x{kg}x{splits} nw {nw}", 65, 144, 2112, swizzled)


@LAYOUTS
@pytest.mark.parametrize("M", (2, 4))
def test_below_the_gemv_boundary(M, swizzled):
    with tuning(nvfp4=(0, 1, 0, 0, 0), nvfp4_mfma=1):  # the GEMV keeps one token only
        check("nvfp4 mfma, boundary 1", M, 144, 2112, swizzled)


@LAYOUTS
@pytest.mark.parametrize("M", (5, 11))
@pytest.mark.parametrize("name", golden_files("nvfp4_N144"))
def test_dynamic(name, M, swizzled):
    rec = load_golden(name)
    dev = lambda k: torch.from_numpy(rec[k]).to(DEV) if k in rec.files else None  # noqa: E731
    s = torch.from_numpy(rec["scales_swizzled" if swizzled else "scales_rowmajor"]).reshape(-1)
    q, s, bias = dev("qdata"), s.to(DEV), bf16(rec["bias"]).to(DEV)
    pts, apts = dev("per_tensor_scale"), dev("act_per_tensor_scale")
    rows = np.arange(M) % rec["x"].shape[0]  # the fixture's 5 rows, wrapped around
    x = bf16(rec["x"][rows]).to(DEV)
    with tuning(nvfp4_mfma=1):
        y = T.nvfp4_linear(x, q, s, pts, bias, swizzled, True, apts)
        assert _last_kernel() == "gemm_mfma_kernel"
        ref = torch.from_numpy(rec["y64_dyn"][rows])
        err = float(torch.linalg.norm(y.cpu().double() - ref) / torch.linalg.norm(ref))
        assert err <= BAR64, err
        if apts is None:  # DYNAMIC is "snap x, then the same product"
            two = T.nvfp4_linear(T.nvfp4_act_qdq(x, None), q, s, pts, bias, swizzled, False, None)
            assert _last_kernel() == "gemm_mfma_kernel"
            assert torch.equal(y, two)


def test_quantized_module():
    gen = torch.Generator().manual_seed(4)
    lin = torch.nn.Linear(2112, 256, bias=False, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(256, 2112, generator=gen) * 0.02).to(torch.bfloat16))
    lin = lin.to(DEV)
    quantize_(lin, NVFP4InferenceConfig(NVFP4MMConfig.WEIGHT_ONLY, use_triton_kernel=False))
    x = torch.randn(48, 2112, generator=gen).to(torch.bfloat16).to(DEV)
    ref = x.double().cpu() @ lin.weight.to_dtype(torch.bfloat16).double().cpu().t()
    with torch.no_grad(), tuning(nvfp4_mfma=1):
        y = lin(x)
        assert _last_kernel() == "gemm_mfma_kernel"
    err = float(torch.linalg.norm(y.double().cpu() - ref) / torch.linalg.norm(ref))
    assert err <= BAR64, err
    with torch.no_grad():  # hook off: the built-in route and its kernel
        lin(x)
    assert _last_kernel() == "nvfp4_dequant_kernel"


def test_hook_argument_check():
    assert _lib.lib().tao_tune_nvfp4_mfma(2) != 0
    assert "tune: nvfp4 mfma" in _lib.lib().tao_last_error().decode()
