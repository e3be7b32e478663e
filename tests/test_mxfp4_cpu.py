"""CPU tests of the MXFP4-weight inference workflow (MXFPInferenceConfig with e4m3fn activations
and float4_e2m1fn_x2 weights): the plain-torch to_mx / to_dtype against the reference fixtures byte
for byte (tests/golden/mxfp4w_*.npz, mxfp4_quant_edges.npz, written by
experiments/gen_golden_mxfp4.py), the quantized structure, the refusals, checkpoint interchange with
the reference, the op registration, the C-ABI argument validation and the formula's float32
evaluation. No GPU compute is invoked.

NaN-sign exemption: the nibble written for a NaN *input* element is compared without its sign bit
(3 elements of the edge fixture, listed in its ``nan_elems``); nothing else is exempt."""

import ctypes
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao import _lib, ops
from torchao.prototype.mx_formats import MXFPInferenceConfig, MXGemmKernelChoice
from torchao.prototype.mx_formats.config import ScaleCalculationMode
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
F4 = torch.float4_e2m1fn_x2
FIXTURES = golden_files("mxfp4w_N")
CKPT = "mxfp4w_refckpt_N32_K64"
BAR = 4e-3  # the project's bar against float64 on the same codes (tests/test_mx_cpu.py)
F4_VALUES = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _config(**kw):
    return MXFPInferenceConfig(activation_dtype=E4, weight_dtype=F4, **kw)


def _linear(rec, bias=True):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=bias, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if bias:
            lin.bias.copy_(bf16(rec["bias"]))
    return lin


def nan_sign_mask(rec):
    """uint8 [R, K/2]: 0xFF, with the sign bit cleared on the nibbles of NaN input elements."""
    mask = np.full(rec["q"].shape, 0xFF, dtype=np.uint8)
    for r, k in rec["nan_elems"]:
        mask[r, k // 2] &= 0x7F if k % 2 == 0 else 0xF7
    return mask


def test_fixture_files_present():
    assert FIXTURES == ["mxfp4w_N40_K352.npz", "mxfp4w_N64_K256.npz", "mxfp4w_N96_K1024.npz"]
    rec = load_golden("mxfp4_quant_edges.npz")
    assert len(rec["nan_elems"]) == 3


def test_nibble_order_of_the_stored_bytes():
    """Element 2 j sits in the HIGH nibble of byte j (the reference's pack_uint4)."""
    x = torch.zeros(1, 32, dtype=torch.bfloat16)
    x[0, :8] = torch.tensor([0.5, 1, 1.5, 2, 3, 4, 6, -6], dtype=torch.bfloat16)
    scale, q = to_mx(x, F4, 32)
    assert _u8(scale).item() == 127
    assert q.dtype is torch.uint8 and q.shape == (1, 16)
    assert q[0, :4].tolist() == [0x12, 0x34, 0x56, 0x7F] and not q[0, 4:].any()
    deq = to_dtype(q, scale, F4, 32, torch.bfloat16)
    assert torch.equal(_bits(deq), _bits(x))


@pytest.mark.parametrize("fname", FIXTURES)
def test_to_mx_and_to_dtype_match_the_reference(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    scale, codes = to_mx(bf16(rec["w"]), F4, 32)
    assert scale.dtype is E8 and codes.dtype is torch.uint8
    assert codes.shape == (N, K // 2) == rec["wq"].shape and scale.shape == rec["ws"].shape
    assert np.array_equal(codes.numpy(), rec["wq"]), fname
    assert np.array_equal(_u8(scale).numpy(), rec["ws"]), fname
    s32, c32 = to_mx(bf16(rec["w"]).float(), F4, 32)
    assert torch.equal(_u8(s32), _u8(scale)) and torch.equal(c32, codes)
    # the activation side is the MXFP8 quantizer
    xs, xq = to_mx(bf16(rec["x"]), E4, 32)
    assert np.array_equal(_u8(xq).numpy(), rec["xq"]) and np.array_equal(_u8(xs).numpy(), rec["xs"])
    zt = int(rec["zero_token"])
    assert not rec["xs"][zt].any() and not rec["xq"][zt].any()
    if "w_deq" in rec:
        deq = to_dtype(torch.from_numpy(rec["wq"]), torch.from_numpy(rec["ws"]).view(E8), F4, 32,
                       torch.bfloat16)
        assert deq.shape == (N, K)
        assert torch.equal(_bits(deq), _bits(bf16(rec["w_deq"])))


def test_quantizer_edge_blocks_match_the_reference():
    rec = load_golden("mxfp4_quant_edges.npz")
    x = bf16(rec["x"])
    mask = nan_sign_mask(rec)
    assert int((mask != 0xFF).sum()) == 3
    scale, codes = to_mx(x, F4, 32)
    assert np.array_equal(_u8(scale).numpy(), rec["s"])
    assert np.array_equal(codes.numpy() & mask, rec["q"] & mask)
    s, q = rec["s"], rec["q"]
    assert s[0, 0] == 255 and s[7, 1] == 255 and s[8, 1] == 255   # NaN blocks (NaN beside inf too)
    assert s[0, 1] == 253 and s[8, 0] == 253                       # +-inf: exponent field 255 - 2
    assert q[0, (32 + 9) // 2] & 0x0F == 0x7 and q[8, 0] & 0x0F == 0xF   # inf -> +-6
    assert q[0, 2] & 0x07 == 0x3                                   # the NaN element's own nibble
    assert s[1, 0] == 0 and s[1, 1] == 0                           # all zero, all subnormal
    assert not q[1, :16].any() and q[1, 16:].any()
    assert s[2, 0] == 128 and s[2, 1] == 127       # amax 8.0 and the number just below it
    # the ties, in units of the block scale: 0.25->0 0.75->1 1.25->1 1.75->2 2.5->2 3.5->4 5->4 7->6
    assert q[3, :4].tolist() == [0x02, 0x24, 0x46, 0x67]
    assert q[3, 8:12].tolist() == [0x8A, 0xAC, 0xCE, 0xEF]          # and in the other sign
    assert q[3, 16 + 1] == 0x88                                     # -0.0 and a tiny negative
    assert s[4, 0] == 127 and s[4, 1] == 131 and q[4, 0] >> 4 == 0x6 and q[4, 16] & 0xF == 0xF
    assert q[5, 1] == 0x7F and q[5, 16 + 3] == 0xF7                 # 7 and 7.5 saturate at 6
    assert s[6, 0] == 252 and s[9, 0] == 0
    deq = to_dtype(codes, scale, F4, 32, torch.bfloat16)
    ref = bf16(rec["deq"])
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(deq), nan)
    assert torch.equal(_bits(deq)[~nan], _bits(ref)[~nan])
    # fp32 input takes the same path
    s32, c32 = to_mx(x.float(), F4, 32)
    assert torch.equal(_u8(s32), _u8(scale)) and torch.equal(c32, codes)


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_gives_an_mxtensor_with_the_fixture_bytes(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _linear(rec)
    quantize_(lin, _config())
    w = lin.weight
    assert isinstance(w, torch.nn.Parameter) and isinstance(w, MXTensor) and not w.requires_grad
    assert w.shape == (N, K) and w.dtype is torch.bfloat16
    assert w.qdata.dtype is torch.uint8 and w.qdata.shape == (N, K // 2)
    assert w._scale_e8m0.dtype is E8 and w._scale_e8m0.shape == (N, K // 32)
    assert w._scale_e8m0.numel() * 32 == 2 * w.qdata.numel()
    assert w._elem_dtype is F4 and w._block_size == 32 and w._orig_dtype is torch.bfloat16
    assert w._gemm_kernel_choice is MXGemmKernelChoice.CUBLAS and w._pack_fp6 is False
    assert w._use_fp4_custom_triton_dequant_kernel is False
    assert w.act_quant_kwargs == QuantizeTensorToMXKwargs(
        elem_dtype=E4, block_size=32, gemm_kernel_choice=MXGemmKernelChoice.CUBLAS)
    assert np.array_equal(w.qdata.numpy(), rec["wq"])
    assert np.array_equal(_u8(w._scale_e8m0).numpy(), rec["ws"])
    assert "MXTensor" in repr(lin) and f"in_features={K}" in repr(lin)
    assert "float4_e2m1fn_x2" in repr(w) and f"shape=({N}, {K})" in repr(w)
    deq = w.dequantize()
    assert deq.shape == (N, K) and deq.dtype is torch.bfloat16
    assert torch.equal(_bits(deq), _bits(w.to_dtype(torch.bfloat16)))
    if "w_deq" in rec:
        assert torch.equal(_bits(deq), _bits(bf16(rec["w_deq"])))
    for t in (w.detach(), w.clone(), w.to("cpu")):
        assert isinstance(t, MXTensor) and t.shape == (N, K) and t._elem_dtype is F4
        assert torch.equal(t.qdata, w.qdata)
        assert torch.equal(_u8(t._scale_e8m0), _u8(w._scale_e8m0))
        assert t.act_quant_kwargs == w.act_quant_kwargs
    assert w.clone().qdata.data_ptr() != w.qdata.data_ptr()
    # gemm_kernel_choice and use_fp4_custom_triton_dequant_kernel round-trip and pick nothing
    lin2 = _linear(rec)
    quantize_(lin2, _config(gemm_kernel_choice=MXGemmKernelChoice.EMULATED))
    assert lin2.weight._gemm_kernel_choice is MXGemmKernelChoice.EMULATED
    assert torch.equal(lin2.weight.qdata, w.qdata)
    t = MXTensor.to_mx(bf16(rec["w"]), F4, use_fp4_custom_triton_dequant_kernel=True)
    assert t._use_fp4_custom_triton_dequant_kernel is True and torch.equal(t.qdata, w.qdata)
    assert t.detach()._use_fp4_custom_triton_dequant_kernel is True
    assert torch.equal(_bits(t.dequantize()), _bits(deq))


def test_copy_needs_matching_metadata():
    rec = load_golden(FIXTURES[0])
    w4 = MXTensor.to_mx(bf16(rec["w"]), F4)
    w8 = MXTensor.to_mx(bf16(rec["w"]), E4)
    assert w4.shape == w8.shape
    other = MXTensor.to_mx(bf16(rec["w"]) * 2, F4)
    other.copy_(w4)
    assert torch.equal(other.qdata, w4.qdata)
    assert torch.equal(_u8(other._scale_e8m0), _u8(w4._scale_e8m0))
    for dst, src in ((w4, w8), (w8, w4)):
        with pytest.raises(ValueError, match="metadata mismatch"):
            dst.copy_(src)
    with pytest.raises(ValueError, match="metadata mismatch"):
        w4.copy_(torch.zeros(w4.shape, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        MXTensor(w8.qdata, w8._scale_e8m0, F4, 32, torch.bfloat16, False,
                 MXGemmKernelChoice.EMULATED, False, None)
    with pytest.raises(ValueError, match="do not cover"):
        MXTensor(w4.qdata[:, :8], w4._scale_e8m0, F4, 32, torch.bfloat16, False,
                 MXGemmKernelChoice.EMULATED, False, None)


@pytest.mark.parametrize("kwargs", [
    dict(activation_dtype=F4, weight_dtype=F4),
    dict(activation_dtype=F4, weight_dtype=E4),
    dict(activation_dtype=torch.float8_e5m2, weight_dtype=F4),
    dict(activation_dtype=E4, weight_dtype=torch.float8_e5m2),
    dict(activation_dtype=E4, weight_dtype=F4, block_size=64),
])
def test_refusals_leave_the_weight_untouched(kwargs):
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    w0 = lin.weight
    before = w0.detach().clone()
    with pytest.raises(NotImplementedError, match="MXFP8 inference is served.*MXFP4 weights"):
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
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    for mode in (ScaleCalculationMode.EVEN, ScaleCalculationMode.CEIL, ScaleCalculationMode.RCEIL):
        with pytest.raises(NotImplementedError, match="FLOOR"):
            to_mx(x, F4, 32, mode)
    with pytest.raises(AssertionError, match="divisible"):
        to_mx(torch.zeros(2, 48, dtype=torch.bfloat16), F4, 32)
    with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
        to_mx(x, F4, 16)


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    N, K = int(rec["N"]), int(rec["K"])
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    w = sd["weight"]
    assert isinstance(w, MXTensor) and w.shape == (N, K) and w.dtype is torch.bfloat16
    assert w._elem_dtype is F4 and w.qdata.dtype is torch.uint8 and w.qdata.shape == (N, K // 2)
    assert np.array_equal(w.qdata.numpy(), rec["wq"])
    assert np.array_equal(_u8(w._scale_e8m0).numpy().reshape(N, K // 32), rec["ws"])
    assert w._gemm_kernel_choice is MXGemmKernelChoice(str(rec["gemm_kernel_choice"]))
    assert isinstance(w.act_quant_kwargs, QuantizeTensorToMXKwargs)
    assert w.act_quant_kwargs.elem_dtype is E4 and w.act_quant_kwargs.block_size == 32
    assert w.act_quant_kwargs.scaling_mode is ScaleCalculationMode.FLOOR
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    lin.load_state_dict(sd, assign=True)
    assert isinstance(lin.weight, MXTensor) and np.array_equal(lin.weight.qdata.numpy(), rec["wq"])
    assert torch.equal(_bits(lin.bias.detach()), _bits(bf16(rec["bias"])))
    # copy into a module quantized here
    lin2 = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    quantize_(lin2, _config())
    lin2.load_state_dict(sd)
    assert np.array_equal(lin2.weight.qdata.numpy(), rec["wq"])
    assert np.array_equal(_u8(lin2.weight._scale_e8m0).numpy(), rec["ws"])
    # ... but not into an MXFP8 module (from a state dict read afresh, which no module has
    # adopted with assign=True)
    lin3 = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    quantize_(lin3, MXFPInferenceConfig())
    fresh = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    with pytest.raises((ValueError, RuntimeError), match="metadata mismatch"):
        lin3.load_state_dict(fresh)
    assert lin3.weight._elem_dtype is E4


def test_own_state_dict_round_trips():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, _config())
    buf = io.BytesIO()
    torch.save(lin.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    w = sd["weight"]
    assert isinstance(w, MXTensor) and w.act_quant_kwargs == lin.weight.act_quant_kwargs
    assert w._elem_dtype is F4 and w.shape == lin.weight.shape
    assert torch.equal(w.qdata, lin.weight.qdata)
    assert torch.equal(_u8(w._scale_e8m0), _u8(lin.weight._scale_e8m0))
    fresh = torch.nn.Linear(int(rec["K"]), int(rec["N"]), dtype=torch.bfloat16)
    fresh.load_state_dict(sd, assign=True)
    assert torch.equal(fresh.weight.qdata, lin.weight.qdata)


def test_cpu_forward_and_cpu_ops_raise():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, _config())
    x = bf16(rec["x"])
    with pytest.raises(NotImplementedError, match="GPU only"):
        lin(x)
    with pytest.raises(NotImplementedError, match="GPU only"):
        torch.nn.functional.linear(MXTensor.to_mx(x, E4), lin.weight)
    xq, xs = torch.from_numpy(rec["xq"]).view(E4), torch.from_numpy(rec["xs"])
    wq, ws = torch.from_numpy(rec["wq"]), torch.from_numpy(rec["ws"])
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mxfp4_quantize_rows(x)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mxfp4w_scaled_mm(xq, xs, wq, ws, None)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.mxfp4w_dyn_linear(x, wq, ws, None)


def test_op_sets():
    want = {"mxfp4_quantize_rows", "mxfp4w_scaled_mm", "mxfp4w_dyn_linear"}
    for name in want:
        assert hasattr(torch.ops.torchao, name)
    assert ops.native_dispatch_mxfp4() == want, ops._native_error
    assert {d.split("::")[-1] for d in ops.lib_mxfp4._op_defs} == want
    assert not any("mxfp4" in d for d in ops.lib._op_defs)
    assert not any("mxfp4" in d for d in ops.lib_mx._op_defs)


def test_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(2, 3, 352, dtype=torch.bfloat16)
        xq = torch.empty(2, 3, 352, dtype=E4)
        xs = torch.empty(2, 3, 11, dtype=torch.uint8)
        wq = torch.empty(40, 176, dtype=torch.uint8)
        ws = torch.empty(40, 11, dtype=torch.uint8)
        q, s = torch.ops.torchao.mxfp4_quantize_rows(x)
        assert q.shape == (2, 3, 176) and q.dtype is torch.uint8
        assert s.shape == (2, 3, 11) and s.dtype is torch.uint8
        y = torch.ops.torchao.mxfp4w_scaled_mm(xq, xs, wq, ws, None)
        assert y.shape == (2, 3, 40) and y.dtype is torch.bfloat16
        y = torch.ops.torchao.mxfp4w_dyn_linear(x, wq, ws, torch.empty(40, dtype=torch.bfloat16))
        assert y.shape == (2, 3, 40) and y.dtype is torch.bfloat16


def _call(name, *args):
    fn = getattr(_lib.lib(), name)
    return fn(*args), _lib.lib().tao_last_error().decode()


def test_c_abi_validates_before_device_work():
    """Bad arguments return 1 with tao_last_error set; the pointers are never dereferenced (they
    are host buffers or null here)."""
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc, msg = _call("tao_mxfp4_quantize_rows_bf16", p, p, p, 1, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", p, p, p, p, None, p, 1, 8, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mxfp4w_dyn_linear_bf16", p, p, p, None, p, 1, 8, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_mxfp4w_dyn_linear_bf16", p, p, p, None, p, 2, 8, 64, None)
    assert rc == 1 and "one token" in msg
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", p, p, p, p, None, p, -1, 8, 64, None)
    assert rc == 1 and "negative" in msg
    rc, msg = _call("tao_mxfp4w_dyn_linear_bf16", p, p, p, None, p, 1, 8, 65536 + 32, None)
    assert rc == 1 and "65536" in msg
    odd = ctypes.c_void_p(p.value + 1)
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", odd, p, p, p, None, p, 1, 8, 64, None)
    assert rc == 1 and "xq" in msg
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", p, p, odd, p, None, p, 1, 8, 64, None)
    assert rc == 1 and "wq" in msg
    rc, msg = _call("tao_mxfp4_quantize_rows_bf16", p, odd, p, 1, 64, None)
    assert rc == 1 and "q" in msg
    # K % 256 == 0: the scale arrays are 8-B aligned
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", p, odd, p, p, None, p, 1, 8, 256, None)
    assert rc == 1 and "xs" in msg
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", p, p, p, odd, None, p, 1, 8, 256, None)
    assert rc == 1 and "ws" in msg
    # null pointers
    rc, msg = _call("tao_mxfp4w_scaled_mm_bf16", None, p, p, p, None, p, 1, 8, 40, None)
    assert rc == 1 and "multiple of 32" in msg
    # M == 0 is a no-op, null pointers and all
    for name, args in (("tao_mxfp4_quantize_rows_bf16", (None, None, None, 0, 64, None)),
                       ("tao_mxfp4w_scaled_mm_bf16", (None, None, None, None, None, None, 0, 8,
                                                      64, None)),
                       ("tao_mxfp4w_dyn_linear_bf16", (None, None, None, None, None, 0, 8, 64,
                                                       None))):
        assert _call(name, *args)[0] == 0


@pytest.mark.parametrize("fname", FIXTURES)
def test_float32_formula_is_within_the_bar(fname):
    """The formula of csrc/mx_fp4.hip evaluated with float32 sums, block by block, and rounded to
    bf16 once, against y64 on the same codes; and the reference's emulated output, for scale.
    Measured here: 1.6e-3 .. 2.2e-3 for both (the bf16 rounding of the output)."""
    rec = load_golden(fname)
    K = int(rec["K"])
    wq = torch.from_numpy(rec["wq"])
    wf = F4_VALUES[torch.stack([wq >> 4, wq & 0xF], -1).reshape(wq.shape[0], -1).long()]
    xq = torch.from_numpy(rec["xq"]).view(E4).float().reshape(5, 1, K // 32, 32)
    wf = wf.reshape(1, -1, K // 32, 32)
    fx = get_fp_scale(torch.from_numpy(rec["xs"]).view(E8)).reshape(5, 1, K // 32)
    fw = get_fp_scale(torch.from_numpy(rec["ws"]).view(E8)).reshape(1, -1, K // 32)
    acc = (((xq * wf).sum(-1) * fx) * fw).sum(-1)
    y = (acc + bf16(rec["bias"]).float()[None, :]).to(torch.bfloat16)
    y64 = torch.from_numpy(rec["y64"])
    assert bool(y64.isfinite().all())
    e = float((y.double() - y64).norm() / y64.norm())
    e_ref = float((bf16(rec["y_ref"]).double() - y64).norm() / y64.norm())
    print(f"{fname}: float32 formula {e:.3e}, reference emulated {e_ref:.3e}")
    assert e <= BAR and e_ref <= BAR
    zt = int(rec["zero_token"])
    assert torch.equal(_bits(y[zt]), _bits(bf16(rec["bias"])))
