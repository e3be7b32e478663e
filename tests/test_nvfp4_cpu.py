"""CPU tests of the NVFP4 workflow (torchao.prototype.mx_formats, NVFP4InferenceConfig): the
plain-torch quantizer, scale layouts and dequantizer against the reference fixtures bit for bit
(tests/golden/nvfp4_*, written by experiments/gen_golden_nvfp4.py), checkpoint interchange, the CPU
linear of both modes, slicing and the refusals. No GPU compute is invoked."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao.prototype.mx_formats import NVFP4InferenceConfig, NVFP4MMConfig, NVFP4Tensor
from torchao.prototype.mx_formats.nvfp4_tensor import QuantizeTensorToNVFP4Kwargs, nvfp4_quantize
from torchao.prototype.mx_formats.utils import from_blocked, to_blocked
from torchao.quantization import quantize_

E4 = torch.float8_e4m3fn
FIXTURES = golden_files("nvfp4_N")
CKPT = "nvfp4_refckpt_N32_K64"
BAR = 4e-3  # the project's bar against float64 on the same codes (tests/test_gpu_float8.py)
WO = dict(mm_config=NVFP4MMConfig.WEIGHT_ONLY, use_triton_kernel=False)
DYN = dict(mm_config=NVFP4MMConfig.DYNAMIC, use_triton_kernel=False)


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def u8(t):
    return t.detach().contiguous().view(torch.uint8).numpy()


def rel_l2(y, ref):
    y, ref = y.detach().double(), ref.double()
    return float(torch.linalg.norm(y - ref) / torch.linalg.norm(ref))


def scale_of(rec, key):
    return torch.from_numpy(rec[key]) if key in rec.files else None


def _linear(rec, **config):
    N, K = rec["w"].shape
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    quantize_(lin, NVFP4InferenceConfig(**config))
    return lin


def test_fixture_set():
    assert len(FIXTURES) == 6


@pytest.mark.parametrize("name", FIXTURES)
def test_quantizer_layouts_and_dequantizer_equal_the_fixture(name):
    rec = load_golden(name)
    w, pts = bf16(rec["w"]), scale_of(rec, "per_tensor_scale")
    N, K = w.shape
    scales, codes = nvfp4_quantize(w, 16, pts)
    assert np.array_equal(codes.numpy(), rec["qdata"])
    assert np.array_equal(u8(scales), rec["scales_rowmajor"])
    blocked = to_blocked(scales)
    assert blocked.dtype is E4 and np.array_equal(u8(blocked), rec["scales_swizzled"])
    assert torch.equal(from_blocked(blocked, N, K // 16).view(torch.uint8), scales.view(torch.uint8))
    for swizzled in (False, True):
        t = NVFP4Tensor.to_nvfp4(w, per_tensor_scale=pts, is_swizzled_scales=swizzled)
        assert t.shape == (N, K) and t.dtype is torch.bfloat16
        assert np.array_equal(u8(t._scale_e4m3).reshape(-1),
                              rec["scales_swizzled" if swizzled else "scales_rowmajor"].reshape(-1))
        assert np.array_equal(bits(t.to_dtype(torch.bfloat16)), rec["w_hat"])
        assert np.array_equal(bits(t.t().to_dtype(torch.bfloat16)), rec["w_hat"].T)
    xs, xq = nvfp4_quantize(bf16(rec["x"]), 16, scale_of(rec, "act_per_tensor_scale"))
    assert np.array_equal(xq.numpy(), rec["xq_codes"]) and np.array_equal(u8(xs), rec["x_scales"])


@pytest.mark.parametrize("tag", ["", "_pts"])
def test_quantizer_edges(tag):
    rec = load_golden("nvfp4_quant_edges.npz")
    pts = torch.from_numpy(rec["per_tensor_scale"]) if tag else None
    for swizzled in (False, True):
        t = NVFP4Tensor.to_nvfp4(bf16(rec["x"]), per_tensor_scale=pts, is_swizzled_scales=swizzled)
        assert np.array_equal(t.qdata.numpy(), rec["qdata" + tag])
        key = ("scales_swizzled" if swizzled else "scales_rowmajor") + tag
        assert np.array_equal(u8(t._scale_e4m3).reshape(-1), rec[key].reshape(-1))
        assert np.array_equal(bits(t.to_dtype(torch.bfloat16)), rec["w_hat" + tag])


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    w = sd["weight"]
    assert isinstance(w, NVFP4Tensor) and w.shape == (32, 64) and w._is_swizzled_scales
    assert w.act_quant_kwargs is None and w._per_tensor_scale is None and w._block_size == 16
    assert np.array_equal(w.qdata.numpy(), rec["qdata"])
    assert np.array_equal(u8(w._scale_e4m3), rec["scales_swizzled"])
    assert np.array_equal(bits(w.to_dtype(torch.bfloat16)), rec["w_hat"])
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    quantize_(lin, NVFP4InferenceConfig(**WO))
    lin.load_state_dict(sd)
    assert np.array_equal(bits(lin.weight.to_dtype(torch.bfloat16)), rec["w_hat"])


@pytest.mark.parametrize("name", FIXTURES)
def test_quantize_and_cpu_linear(name):
    rec = load_golden(name)
    x = bf16(rec["x"])
    pts, apts = scale_of(rec, "per_tensor_scale"), scale_of(rec, "act_per_tensor_scale")
    for config, key in ((WO, "y64_wo"), (DYN, "y64_dyn")):
        lin = _linear(rec, **config)
        w = lin.weight
        assert isinstance(w, NVFP4Tensor) and not w.requires_grad and w._is_swizzled_scales
        assert (w.act_quant_kwargs == QuantizeTensorToNVFP4Kwargs()) == (config is DYN)
        # quantize_ takes no per-tensor scale; rebuild the weight with the fixture's
        lin.weight = torch.nn.Parameter(NVFP4Tensor.to_nvfp4(
            bf16(rec["w"]), per_tensor_scale=pts, act_per_tensor_scale=apts,
            is_swizzled_scales=True, act_quant_kwargs=w.act_quant_kwargs), requires_grad=False)
        y = lin(x)
        assert y.dtype is torch.bfloat16 and rel_l2(y, torch.from_numpy(rec[key])) <= BAR
        if config is WO:
            assert np.array_equal(bits(y), rec["y_ref"])
            assert torch.equal(torch.addmm(lin.bias, x, lin.weight.t()), y)


def test_slicing():
    w = torch.randn(256, 128).to(torch.bfloat16)
    for swizzled in (False, True):
        t = NVFP4Tensor.to_nvfp4(w, is_swizzled_scales=swizzled)
        full = t.to_dtype(torch.bfloat16)
        assert torch.equal(t[128:].to_dtype(torch.bfloat16), full[128:])
        assert torch.equal(t[:, 64:].to_dtype(torch.bfloat16), full[:, 64:])
        assert torch.equal(t[:128, :64].to_dtype(torch.bfloat16), full[:128, :64])
    with pytest.raises(RuntimeError, match="start index to be a multiple of 128, got 64"):
        t[64:]
    with pytest.raises(RuntimeError, match="multiple of 64 or equal to tensor size 128, got 32"):
        t[:, :32]
    with pytest.raises(AssertionError, match="multiple of block_size 16"):
        NVFP4Tensor.to_nvfp4(w)[:, 8:]


@pytest.mark.parametrize("make,error,text", [
    (lambda: torch.nn.Linear(64, 32, dtype=torch.bfloat16), NotImplementedError,
     "use_triton_kernel=False.*MXFP8 inference is served"),
    (lambda: torch.nn.Linear(72, 32, dtype=torch.bfloat16), RuntimeError, "divisible by 16"),
    (lambda: torch.nn.Linear(64, 24, dtype=torch.bfloat16), RuntimeError, "divisible by 16"),
    (lambda: torch.nn.Linear(64, 32), RuntimeError, "Bias is not supported"),
], ids=["triton", "K72", "N24", "fp32-bias"])
def test_refusals_leave_the_module_untouched(make, error, text):
    lin = make()
    w0, before = lin.weight, lin.weight.detach().clone()
    config = NVFP4InferenceConfig(**WO)
    if error is NotImplementedError:
        with pytest.raises(error, match=text):
            NVFP4InferenceConfig()
        config.use_triton_kernel = True  # changed after construction: the handler refuses
    with pytest.raises(error, match=text):
        quantize_(lin, config)
    assert lin.weight is w0 and torch.equal(lin.weight.detach(), before)
    assert "extra_repr" not in lin.__dict__
