"""CPU tests of the MXFP8 inference workflow (torchao.prototype.mx_formats, MXFPInferenceConfig):
the plain-torch to_mx / to_dtype against the reference fixtures byte for byte
(tests/golden/mxfp8_*.npz, mx_quant_edges.npz, written by experiments/gen_golden_mx.py), the
quantized structure, the refusals, checkpoint interchange with the reference, the op registration,
the C-ABI argument validation and the formula's float32 evaluation. No GPU compute is invoked."""

import ctypes
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao import _lib, ops
from torchao.prototype.mx_formats import MXFPInferenceConfig, MXGemmKernelChoice
from torchao.prototype.mx_formats.config import MXLinearConfig, ScaleCalculationMode
from torchao.prototype.mx_formats.inference_workflow import NVFP4InferenceConfig
from torchao.prototype.mx_formats.mx_tensor import (
    MXTensor,
    QuantizeTensorToMXKwargs,
    get_fp_scale,
    to_dtype,
    to_mx,
)
from torchao.quantization import quantize_

E4 = torch.float8_e4m3fn
E8 = torch.float8_e8m0fnu
FIXTURES = golden_files("mxfp8_N")
CKPT = "mxfp8_refckpt_N32_K64"
BAR = 4e-3  # the project's bar against float64 on the same codes (tests/test_float8_dyn_cpu.py)


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _linear(rec, bias=True):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=bias, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if bias:
            lin.bias.copy_(bf16(rec["bias"]))
    return lin


def test_fixture_files_present():
    assert FIXTURES == ["mxfp8_N40_K352.npz", "mxfp8_N64_K256.npz", "mxfp8_N96_K1024.npz"]
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if f.startswith("float8"))
    for f in os.listdir(GOLDEN):
        if f.startswith("mx"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= largest, f


@pytest.mark.parametrize("fname", FIXTURES)
def test_to_mx_and_to_dtype_match_the_reference(fname):
    rec = load_golden(fname)
    for a, q, s in (("w", "wq", "ws"), ("x", "xq", "xs")):
        scale, codes = to_mx(bf16(rec[a]), E4, 32)
        assert scale.dtype is E8 and codes.dtype is E4
        assert scale.shape == rec[s].shape and codes.shape == rec[q].shape
        assert np.array_equal(_u8(codes).numpy(), rec[q]), (fname, a)
        assert np.array_equal(_u8(scale).numpy(), rec[s]), (fname, a)
    zt = int(rec["zero_token"])
    assert not rec["xs"][zt].any() and not rec["xq"][zt].any()
    assert rec["xs"][int(rec["subnormal_token"]), int(rec["subnormal_block"])] == 0
    if "w_deq" in rec:
        deq = to_dtype(torch.from_numpy(rec["wq"]).view(E4), torch.from_numpy(rec["ws"]).view(E8),
                       E4, 32, torch.bfloat16)
        assert torch.equal(_bits(deq), _bits(bf16(rec["w_deq"])))


def test_quantizer_edge_blocks_match_the_reference():
    rec = load_golden("mx_quant_edges.npz")
    x = bf16(rec["x"])
    scale, codes = to_mx(x, E4, 32)
    assert np.array_equal(_u8(scale).numpy(), rec["s"])
    assert np.array_equal(_u8(codes).numpy(), rec["q"])
    s = rec["s"]
    assert s[0, 0] == 255 and s[5, 1] == 255      # NaN blocks (NaN wins over inf)
    assert s[0, 1] == 247                          # +inf: exponent field 255 - 8
    assert s[1, 0] == 0 and s[1, 1] == 0           # all zero, all subnormal
    assert s[2, 0] == 122 and s[2, 1] == 121       # amax 8.0 and the number just below it
    assert not rec["q"][1, :32].any() and rec["q"][1, 32:].any()
    assert rec["q"][3, 1] == 0x7E and rec["q"][3, 33] == 0xFE and rec["q"][3, 34] == 0x7E
    deq = to_dtype(codes, scale, E4, 32, torch.bfloat16)
    assert torch.equal(_bits(deq), _bits(bf16(rec["deq"])))
    # fp32 input takes the same path
    s32, c32 = to_mx(x.float(), E4, 32)
    assert torch.equal(_u8(s32), _u8(scale)) and torch.equal(_u8(c32), _u8(codes))


def test_scale_decode():
    f = get_fp_scale(torch.tensor([0, 1, 127, 254, 255], dtype=torch.uint8).view(E8))
    assert f[0].item() == 2.0 ** -127 and f[1].item() == 2.0 ** -126 and f[2].item() == 1.0
    assert f[3].item() == 2.0 ** 127 and f[4].isnan()


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_gives_an_mxtensor_with_the_fixture_bytes(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _linear(rec)
    quantize_(lin, MXFPInferenceConfig())
    w = lin.weight
    assert isinstance(w, torch.nn.Parameter) and isinstance(w, MXTensor) and not w.requires_grad
    assert w.shape == (N, K) and w.dtype is torch.bfloat16
    assert w.qdata.dtype is E4 and w.qdata.shape == (N, K)
    assert w._scale_e8m0.dtype is E8 and w._scale_e8m0.shape == (N, K // 32)
    assert w._elem_dtype is E4 and w._block_size == 32 and w._orig_dtype is torch.bfloat16
    assert w._gemm_kernel_choice is MXGemmKernelChoice.CUBLAS and w._pack_fp6 is False
    assert w.act_quant_kwargs == QuantizeTensorToMXKwargs(
        elem_dtype=E4, block_size=32, gemm_kernel_choice=MXGemmKernelChoice.CUBLAS)
    assert np.array_equal(_u8(w.qdata).numpy(), rec["wq"])
    assert np.array_equal(_u8(w._scale_e8m0).numpy(), rec["ws"])
    assert "MXTensor" in repr(lin) and f"in_features={K}" in repr(lin)
    assert torch.equal(_bits(w.dequantize()), _bits(w.to_dtype(torch.bfloat16)))
    for t in (w.detach(), w.clone(), w.to("cpu")):
        assert isinstance(t, MXTensor) and torch.equal(_u8(t.qdata), _u8(w.qdata))
        assert torch.equal(_u8(t._scale_e8m0), _u8(w._scale_e8m0))
        assert t.act_quant_kwargs == w.act_quant_kwargs
    assert w.clone().qdata.data_ptr() != w.qdata.data_ptr()
    # gemm_kernel_choice round-trips and picks nothing
    lin2 = _linear(rec)
    quantize_(lin2, MXFPInferenceConfig(gemm_kernel_choice=MXGemmKernelChoice.EMULATED))
    assert lin2.weight._gemm_kernel_choice is MXGemmKernelChoice.EMULATED
    assert torch.equal(_u8(lin2.weight.qdata), _u8(w.qdata))


@pytest.mark.parametrize("kwargs", [
    dict(activation_dtype=torch.float8_e5m2, weight_dtype=torch.float8_e5m2),
    dict(activation_dtype=torch.float4_e2m1fn_x2, weight_dtype=torch.float4_e2m1fn_x2),
    dict(activation_dtype="fp6_e2m3", weight_dtype="fp6_e2m3"),
    dict(activation_dtype="fp6_e3m2", weight_dtype="fp6_e3m2"),
    dict(block_size=64),
])
def test_refusals_leave_the_weight_untouched(kwargs):
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    w0 = lin.weight
    before = w0.detach().clone()
    with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
        quantize_(lin, MXFPInferenceConfig(**kwargs))
    # a config whose fields were changed after construction is refused by the handler
    cfg = MXFPInferenceConfig()
    for k, v in kwargs.items():
        setattr(cfg, k, v)
    with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
        quantize_(lin, cfg)
    assert lin.weight is w0 and type(lin.weight) is torch.nn.Parameter
    assert torch.equal(lin.weight.detach(), before) and "extra_repr" not in lin.__dict__


def test_other_refusals():
    for make in (NVFP4InferenceConfig, MXLinearConfig):
        with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
            make()
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    for mode in (ScaleCalculationMode.EVEN, ScaleCalculationMode.CEIL, ScaleCalculationMode.RCEIL):
        with pytest.raises(NotImplementedError, match="FLOOR"):
            to_mx(x, E4, 32, mode)
    with pytest.raises(NotImplementedError):
        to_mx(x, E4, 32, pack_fp6=True)
    with pytest.raises(AssertionError, match="divisible"):
        to_mx(torch.zeros(2, 40, dtype=torch.bfloat16), E4, 32)
    lin = torch.nn.Linear(64, 32)  # fp32 weight: the reference's assertion
    with pytest.raises(AssertionError, match="bf16"):
        quantize_(lin, MXFPInferenceConfig())
    assert type(lin.weight.data) is torch.Tensor


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    N, K = int(rec["N"]), int(rec["K"])
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    w = sd["weight"]
    assert isinstance(w, MXTensor) and w.shape == (N, K) and w.dtype is torch.bfloat16
    assert np.array_equal(_u8(w.qdata).numpy(), rec["wq"])
    assert np.array_equal(_u8(w._scale_e8m0).numpy().reshape(N, K // 32), rec["ws"])
    assert w._gemm_kernel_choice is MXGemmKernelChoice(str(rec["gemm_kernel_choice"]))
    assert isinstance(w.act_quant_kwargs, QuantizeTensorToMXKwargs)
    assert w.act_quant_kwargs.elem_dtype is E4 and w.act_quant_kwargs.block_size == 32
    assert w.act_quant_kwargs.scaling_mode is ScaleCalculationMode.FLOOR
    # assign=True
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    lin.load_state_dict(sd, assign=True)
    assert isinstance(lin.weight, MXTensor)
    assert np.array_equal(_u8(lin.weight.qdata).numpy(), rec["wq"])
    assert torch.equal(_bits(lin.bias.detach()), _bits(bf16(rec["bias"])))
    # copy into a module quantized here
    lin2 = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    quantize_(lin2, MXFPInferenceConfig())
    lin2.load_state_dict(sd)
    assert np.array_equal(_u8(lin2.weight.qdata).numpy(), rec["wq"])
    assert np.array_equal(_u8(lin2.weight._scale_e8m0).numpy(), rec["ws"])


def test_own_state_dict_round_trips():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, MXFPInferenceConfig())
    buf = io.BytesIO()
    torch.save(lin.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    w = sd["weight"]
    assert isinstance(w, MXTensor) and w.act_quant_kwargs == lin.weight.act_quant_kwargs
    assert w._gemm_kernel_choice is MXGemmKernelChoice.CUBLAS
    assert torch.equal(_u8(w.qdata), _u8(lin.weight.qdata))
    assert torch.equal(_u8(w._scale_e8m0), _u8(lin.weight._scale_e8m0))
    fresh = torch.nn.Linear(int(rec["K"]), int(rec["N"]), dtype=torch.bfloat16)
    fresh.load_state_dict(sd, assign=True)
    assert torch.equal(_u8(fresh.weight.qdata), _u8(lin.weight.qdata))
    with pytest.raises(ValueError, match="metadata mismatch"):
        lin.weight.copy_(torch.zeros(lin.weight.shape, dtype=torch.bfloat16))


def test_cpu_forward_and_cpu_ops_raise():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, MXFPInferenceConfig())
    x = bf16(rec["x"])
    with pytest.raises(NotImplementedError, match="GPU only"):
        lin(x)
    xq, xs = torch.from_numpy(rec["xq"]).view(E4), torch.from_numpy(rec["xs"])
    wq, ws = torch.from_numpy(rec["wq"]).view(E4), torch.from_numpy(rec["ws"])
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mx_quantize_rows(x)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mx_scaled_mm(xq, xs, wq, ws, None)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mx_dyn_linear(x, wq, ws, None)


def test_op_sets():
    want = {"mx_quantize_rows", "mx_scaled_mm", "mx_dyn_linear"}
    for name in want:
        assert hasattr(torch.ops.torchao, name)
    assert ops.native_dispatch_mx() == want, ops._native_error
    assert ops.native_dispatch() == {
        "int4_weight_only_linear", "int8_weight_only_linear", "int8_quantize_per_token",
        "int8_scaled_mm", "int8_dyn_linear"}, ops._native_error
    assert ops.native_dispatch_float8() == {
        "fp8_weight_only_linear", "fp8_quantize_rows", "fp8_dequantize"}, ops._native_error
    assert ops.native_dispatch_float8_dyn() == {"fp8_scaled_mm",
                                                "fp8_dyn_linear"}, ops._native_error
    assert not any("mx_" in d for d in ops.lib._op_defs)
    assert {d.split("::")[-1] for d in ops.lib_mx._op_defs} == want


def test_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(2, 3, 352, dtype=torch.bfloat16)
        wq = torch.empty(40, 352, dtype=E4)
        ws = torch.empty(40, 11, dtype=torch.uint8)
        q, s = torch.ops.torchao.mx_quantize_rows(x)
        assert q.shape == (2, 3, 352) and q.dtype is E4
        assert s.shape == (2, 3, 11) and s.dtype is torch.uint8
        y = torch.ops.torchao.mx_scaled_mm(q, s, wq, ws, None)
        assert y.shape == (2, 3, 40) and y.dtype is torch.bfloat16
        y = torch.ops.torchao.mx_dyn_linear(x, wq, ws, torch.empty(40, dtype=torch.bfloat16))
        assert y.shape == (2, 3, 40) and y.dtype is torch.bfloat16


def _call(name, *args):
    fn = getattr(_lib.lib(), name)
    return fn(*args), _lib.lib().tao_last_error().decode()


def test_c_abi_validates_before_device_work():
    """Bad arguments return 1 with tao_last_error set; the pointers are never dereferenced (they
    are host buffers here)."""
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc, msg = _call("tao_mx_quantize_rows_bf16", p, p, p, 1, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mx_scaled_mm_bf16", p, p, p, p, None, p, 1, 8, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mx_dyn_linear_bf16", p, p, p, None, p, 1, 8, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mx_dyn_linear_bf16", p, p, p, None, p, 2, 8, 64, None)
    assert rc == 1 and "one token" in msg
    rc, msg = _call("tao_mx_scaled_mm_bf16", p, p, p, p, None, p, -1, 8, 64, None)
    assert rc == 1 and "negative" in msg
    rc, msg = _call("tao_mx_dyn_linear_bf16", p, p, p, None, p, 1, 8, 65536 + 32, None)
    assert rc == 1 and "65536" in msg
    odd = ctypes.c_void_p(p.value + 1)
    rc, msg = _call("tao_mx_scaled_mm_bf16", odd, p, p, p, None, p, 1, 8, 64, None)
    assert rc == 1 and "xq" in msg
    # K % 256 == 0: the scale arrays are read in 8-B words
    rc, msg = _call("tao_mx_scaled_mm_bf16", p, odd, p, p, None, p, 1, 8, 256, None)
    assert rc == 1 and "xs" in msg
    rc, msg = _call("tao_mx_scaled_mm_bf16", p, p, p, odd, None, p, 1, 8, 256, None)
    assert rc == 1 and "ws" in msg
    # M == 0 is a no-op
    for name, args in (("tao_mx_quantize_rows_bf16", (p, p, p, 0, 64, None)),
                       ("tao_mx_scaled_mm_bf16", (p, p, p, p, None, p, 0, 8, 64, None)),
                       ("tao_mx_dyn_linear_bf16", (p, p, p, None, p, 0, 8, 64, None))):
        assert _call(name, *args)[0] == 0
    rc, msg = _call("tao_tune_mx_mfma", 2)
    assert rc == 1 and "mx mfma" in msg
    assert _call("tao_tune_mx_mfma", 1)[0] == 0 and _call("tao_tune_reset")[0] == 0


@pytest.mark.parametrize("fname", FIXTURES)
def test_float32_formula_is_within_the_bar(fname):
    """The formula of csrc/mx_fp8.hip evaluated with float32 sums, block by block, and rounded to
    bf16 once, against y64 on the same codes; and the reference's emulated output, for scale.
    Measured here: 1.6e-3 .. 1.9e-3 for both (the bf16 rounding of the output)."""
    rec = load_golden(fname)
    K = int(rec["K"])
    xq = torch.from_numpy(rec["xq"]).view(E4).float().reshape(5, 1, K // 32, 32)
    wq = torch.from_numpy(rec["wq"]).view(E4).float().reshape(1, -1, K // 32, 32)
    fx = get_fp_scale(torch.from_numpy(rec["xs"]).view(E8)).reshape(5, 1, K // 32)
    fw = get_fp_scale(torch.from_numpy(rec["ws"]).view(E8)).reshape(1, -1, K // 32)
    acc = (((xq * wq).sum(-1) * fx) * fw).sum(-1)
    y = (acc + bf16(rec["bias"]).float()[None, :]).to(torch.bfloat16)
    y64 = torch.from_numpy(rec["y64"])
    assert bool(y64.isfinite().all())
    e = float((y.double() - y64).norm() / y64.norm())
    e_ref = float((bf16(rec["y_ref"]).double() - y64).norm() / y64.norm())
    print(f"{fname}: float32 formula {e:.3e}, reference emulated {e_ref:.3e}")
    assert e <= BAR and e_ref <= BAR
    zt = int(rec["zero_token"])
    assert torch.equal(_bits(y[zt]), _bits(bf16(rec["bias"])))
