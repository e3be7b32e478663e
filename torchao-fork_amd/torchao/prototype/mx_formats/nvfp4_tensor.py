"""``NVFP4Tensor``: e2m1 codes two per byte, one float8_e4m3fn scale per 16 elements of the last
dimension, and an optional fp32 per-tensor scale on top.

Reference: torchao/prototype/mx_formats/nvfp4_tensor.py (``NVFP4Tensor`` :64-279, its aten ops
:282-707, ``nvfp4_quantize`` :726-799). Names, fields and stored bytes are the reference's, so a
``state_dict`` it saved loads here. ``nvfp4_quantize`` / ``to_dtype`` below are the plain-torch
statement of the arithmetic; they run anywhere and equal the reference bit for bit on the CPU. On
the GPU, for bf16 tensors, ``to_nvfp4`` is the fused quantizer (``torch.ops.torchao.nvfp4_quantize``),
``to_dtype(bfloat16)`` the HIP dequantizer and ``F.linear`` on an ``NVFP4Tensor`` weight
``torch.ops.torchao.nvfp4_linear`` (csrc/nvfp4.hip), in both modes:

    y[m][n] = bf16(alpha * sum_k xq[m][k] * (e2m1(wq[n][k]) * e4m3(ws[n][k / 16])) + fp32(bias[n]))

with fp32 sums and one rounding; ``alpha`` is the weight's per-tensor scale (1 if absent) times, in
DYNAMIC mode, the activation's; ``xq`` is x (WEIGHT_ONLY) or x snapped to its NVFP4 grid (DYNAMIC).
The reference's DYNAMIC mode is ``torch._scaled_mm`` on sm100; its WEIGHT_ONLY mode rounds the
dequantized weight, the product and the bias sum to bf16 in turn. Everything the kernels do not
serve (CPU, fp32 / fp16, N % 16 or K % 64 != 0, transposed codes) runs plain torch ops: WEIGHT_ONLY
as the reference, DYNAMIC as the formula above in fp32.
"""

import sys
from dataclasses import dataclass
from enum import Enum
from typing import Optional

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.prototype.mx_formats.mx_tensor import (
    F4_E2M1_VALUES,
    _f32_to_e2m1_codes,
    _pack_e2m1,
    _unpack_e2m1,
)
from torchao.prototype.mx_formats.utils import ceil_div, from_blocked, to_blocked
from torchao.utils import TorchAOBaseTensor, fill_defaults

aten = torch.ops.aten

F4_E2M1_MAX = 6.0
F8E4M3_MAX = 448.0
E4M3_EPS = torch.finfo(torch.float8_e4m3fn).tiny  # 2^-6

NO_TRITON = ("the Triton NVFP4 quantizer (use_triton_kernel=True) is not built: pass "
             "use_triton_kernel=False")


class NVFP4MMConfig(Enum):
    DYNAMIC = "dynamic"
    WEIGHT_ONLY = "weight_only"


@dataclass
class QuantizeTensorToNVFP4Kwargs:
    """How the activation of a DYNAMIC NVFP4 linear is quantized (the reference's fields)."""

    block_size: int = 16
    is_swizzled_scales: bool = False
    use_triton_kernel: bool = False


def per_tensor_amax_to_scale(amax: torch.Tensor) -> torch.Tensor:
    """amax / (448 * 6): with it the largest block scale of the tensor reaches the top of e4m3."""
    return amax.to(torch.float32) / (F8E4M3_MAX * F4_E2M1_MAX)


def nvfp4_quantize(data_hp: torch.Tensor, block_size: int = 16,
                   per_tensor_scale: Optional[torch.Tensor] = None):
    """bf16 / fp32 [rows, ..., K] -> (float8_e4m3fn scales [rows, K / 16], uint8 codes [..., K / 2]).

    Per block of 16, in fp32: ``b = amax / 6`` (``/ per_tensor_scale`` too where there is one), the
    scale is ``e4m3fn(clamp(b, 2^-6, 448))``, round to nearest even, and the codes are the e2m1
    rounding (nearest even) of ``clamp(x / (scale or per_tensor_scale * scale), -6, 6)``, element
    2 j of a row in the high nibble of byte j."""
    assert data_hp.dtype in (torch.bfloat16, torch.float), f"{data_hp.dtype} not supported"
    assert data_hp.size(-1) % block_size == 0, "K dim must be divisible by block_size"
    assert data_hp.is_contiguous(), "Only support contiguous data for now"
    assert block_size == 16, "NVFP4 requires block_size=16"
    x = data_hp.float().reshape(data_hp.shape[0], -1, block_size)
    b = x.abs().amax(-1) / F4_E2M1_MAX
    if per_tensor_scale is not None:
        b = b / per_tensor_scale
    scale = b.clamp(min=E4M3_EPS, max=F8E4M3_MAX).to(torch.float8_e4m3fn)
    div = scale.to(torch.float32)
    if per_tensor_scale is not None:
        div = per_tensor_scale * div
    y = (x / div.unsqueeze(-1)).clamp(-F4_E2M1_MAX, F4_E2M1_MAX).view(data_hp.shape)
    return scale, _pack_e2m1(_f32_to_e2m1_codes(y))


def _e2m1_values(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [..., K / 2] -> fp32 [..., K]."""
    table = torch.tensor(F4_E2M1_VALUES + tuple(-v for v in F4_E2M1_VALUES),
                         dtype=torch.float32, device=packed.device)
    return table[_unpack_e2m1(packed).long()]


def _hip_scale(t: Optional[torch.Tensor], like: torch.Tensor) -> bool:
    """A per-tensor scale the kernels take: none, or a 0-dim fp32 tensor on the same device (the
    dequantizer's rounding is the reference's for a 0-dim scale)."""
    return t is None or (t.dim() == 0 and t.dtype == torch.float32 and t.device == like.device)


def _hip_shape(N: int, K: int) -> bool:
    return N > 0 and K > 0 and N % 16 == 0 and K % 64 == 0


class NVFP4Tensor(TorchAOBaseTensor):
    """Attributes as in the reference: ``qdata`` uint8 [N, K / 2] (the tensor's own shape is the
    logical [N, K]), ``_scale_e4m3`` float8_e4m3fn, row-major [N, K / 16] or flat in the swizzled
    128 x 4 layout (``_is_swizzled_scales``), the optional fp32 ``_per_tensor_scale`` and
    ``_act_per_tensor_scale``, and the recipe."""

    tensor_data_names = ["qdata", "_scale_e4m3"]
    optional_tensor_data_names = ["_per_tensor_scale", "_act_per_tensor_scale"]
    tensor_attribute_names = [
        "_block_size",
        "_orig_dtype",
        "_is_swizzled_scales",
        "use_triton_kernel",
        "act_quant_kwargs",
    ]

    def __new__(cls, qdata, blockwise_scales, per_tensor_scale, act_per_tensor_scale, block_size,
                orig_dtype, is_swizzled_scales=False, use_triton_kernel=False,
                act_quant_kwargs=None):
        size = list(qdata.size())
        size[-1 if qdata.stride(0) > qdata.stride(1) else 0] *= 2  # the packed dimension
        self = torch.Tensor._make_wrapper_subclass(
            cls, size, dtype=orig_dtype, device=qdata.device, requires_grad=False)
        self.qdata = qdata
        self._scale_e4m3 = blockwise_scales
        self._per_tensor_scale = per_tensor_scale
        self._act_per_tensor_scale = act_per_tensor_scale
        self._block_size = block_size
        self._orig_dtype = orig_dtype
        self._is_swizzled_scales = is_swizzled_scales
        self.use_triton_kernel = use_triton_kernel
        self.act_quant_kwargs = act_quant_kwargs
        return self

    def __repr__(self):
        return (f"NVFP4Tensor(shape={tuple(self.shape)}, orig_dtype={self._orig_dtype}, "
                f"device={self.qdata.device}, swizzled_scales={self._is_swizzled_scales}, "
                f"per_tensor_scale={self._per_tensor_scale is not None}, "
                f"mm={'weight_only' if self.act_quant_kwargs is None else 'dynamic'})")

    def _data_names(self):
        return self.tensor_data_names + [n for n in self.optional_tensor_data_names
                                         if getattr(self, n) is not None]

    def __tensor_flatten__(self):
        return self._data_names(), [getattr(self, n) for n in self.tensor_attribute_names]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        return cls(tensor_data_dict["qdata"], tensor_data_dict["_scale_e4m3"],
                   tensor_data_dict.get("_per_tensor_scale"),
                   tensor_data_dict.get("_act_per_tensor_scale"), *tensor_attributes)

    def _with(self, qdata, scales, orig_dtype=None):
        """The same recipe and per-tensor scales around other codes and scales."""
        return NVFP4Tensor(qdata, scales, self._per_tensor_scale, self._act_per_tensor_scale,
                           self._block_size, orig_dtype or self._orig_dtype,
                           self._is_swizzled_scales, self.use_triton_kernel, self.act_quant_kwargs)

    def _apply_fn_to_data(self, fn):
        opt = [None if getattr(self, n) is None else fn(getattr(self, n))
               for n in self.optional_tensor_data_names]
        return NVFP4Tensor(fn(self.qdata), fn(self._scale_e4m3), *opt, self._block_size,
                           self._orig_dtype, self._is_swizzled_scales, self.use_triton_kernel,
                           self.act_quant_kwargs)

    @staticmethod
    def to_nvfp4(data_hp: torch.Tensor, block_size: int = 16,
                 per_tensor_scale: Optional[torch.Tensor] = None,
                 act_per_tensor_scale: Optional[torch.Tensor] = None,
                 is_swizzled_scales: bool = False, use_triton_kernel: bool = False,
                 act_quant_kwargs: Optional[QuantizeTensorToNVFP4Kwargs] = None):
        """The fused HIP quantizer for a 2D bf16 tensor on the GPU, ``nvfp4_quantize`` (and
        ``to_blocked``) otherwise: the same bytes either way."""
        if use_triton_kernel:
            raise NotImplementedError(NO_TRITON)
        assert block_size == 16, "NVFP4 requires block_size=16"
        if (data_hp.is_cuda and data_hp.dtype == torch.bfloat16 and data_hp.dim() == 2
                and data_hp.shape[1] % 16 == 0 and data_hp.is_contiguous()
                and _hip_scale(per_tensor_scale, data_hp)):
            codes, scales = torch.ops.torchao.nvfp4_quantize(data_hp, per_tensor_scale,
                                                             is_swizzled_scales)
            scales = scales.view(torch.float8_e4m3fn)
            if not is_swizzled_scales:
                scales = scales.view(data_hp.shape[0], -1)
        else:
            scales, codes = nvfp4_quantize(data_hp, block_size, per_tensor_scale)
            if is_swizzled_scales:
                scales = to_blocked(scales.view(data_hp.shape[0], -1)).flatten()
        return NVFP4Tensor(codes, scales, per_tensor_scale, act_per_tensor_scale, block_size,
                           data_hp.dtype, is_swizzled_scales, use_triton_kernel, act_quant_kwargs)

    def _rows_cols(self):
        transposed = self.qdata.stride(0) < self.qdata.stride(1)
        return transposed, (self.shape[1], self.shape[0]) if transposed else tuple(self.shape)

    def _plain_scales(self) -> torch.Tensor:
        """The block scales row-major, float8_e4m3fn [rows, K / 16]."""
        _, (M, K) = self._rows_cols()
        if self._is_swizzled_scales:
            return from_blocked(self._scale_e4m3, M, K // self._block_size)
        return self._scale_e4m3.view(M, K // self._block_size)

    def get_hp_scales(self) -> torch.Tensor:
        """The block scales in the original dtype, times the per-tensor scale where there is one."""
        s = self._plain_scales().to(self._orig_dtype)
        return s if not self._per_tensor_scale else self._per_tensor_scale * s

    def to_dtype(self, target_dtype: torch.dtype) -> torch.Tensor:
        """value(code) * float(get_hp_scales()) in ``target_dtype``."""
        transposed, (M, K) = self._rows_cols()
        if (self.qdata.is_cuda and target_dtype == torch.bfloat16 and not transposed
                and self._orig_dtype == torch.bfloat16 and self.qdata.is_contiguous()
                and _hip_scale(self._per_tensor_scale, self.qdata)):
            return torch.ops.torchao.nvfp4_dequantize(
                self.qdata, self._scale_e4m3.view(torch.uint8).reshape(-1),
                self._per_tensor_scale, self._is_swizzled_scales)
        data = self.qdata.t() if transposed else self.qdata
        v = _e2m1_values(data.contiguous()).view(M, K // self._block_size, self._block_size)
        s = self.get_hp_scales().view(M, K // self._block_size, 1).to(torch.float32)
        out = (v * s).view(M, K).to(target_dtype)
        return out.t() if transposed else out

    def dequantize(self, output_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        return self.to_dtype(self._orig_dtype if output_dtype is None else output_dtype)

    @classmethod
    def _same_metadata(cls, self: "NVFP4Tensor", src: "NVFP4Tensor") -> bool:
        def alike(a, b):
            return (a is None and b is None) or (a is not None and b is not None
                                                 and a.shape == b.shape)
        return (isinstance(self, NVFP4Tensor) and isinstance(src, NVFP4Tensor)
                and self._block_size == src._block_size and self._orig_dtype == src._orig_dtype
                and self._is_swizzled_scales == src._is_swizzled_scales
                and self._scale_e4m3.shape == src._scale_e4m3.shape
                and alike(self._per_tensor_scale, src._per_tensor_scale)
                and alike(self._act_per_tensor_scale, src._act_per_tensor_scale)
                and self.qdata.shape == src.qdata.shape
                and self.act_quant_kwargs == src.act_quant_kwargs)


implements = NVFP4Tensor.implements
to_nvfp4 = NVFP4Tensor.to_nvfp4


def to_dtype(tensor: NVFP4Tensor, target_dtype: torch.dtype) -> torch.Tensor:
    return tensor.to_dtype(target_dtype)


def get_hp_scales(tensor: NVFP4Tensor) -> torch.Tensor:
    return tensor.get_hp_scales()


# ---- the linear -------------------------------------------------------------------------------
def _snap(x: torch.Tensor, per_tensor_scale) -> torch.Tensor:
    """x on its NVFP4 grid, fp32: value(code) * scale, which is exact."""
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    if x2.dtype not in (torch.bfloat16, torch.float32):
        x2 = x2.float()
    scale, codes = nvfp4_quantize(x2, 16, per_tensor_scale)
    v = _e2m1_values(codes).view(x2.shape[0], -1, 16) * scale.to(torch.float32).unsqueeze(-1)
    return v.view(x2.shape)


def _nvfp4_linear(x: torch.Tensor, w: NVFP4Tensor, bias) -> torch.Tensor:
    if not isinstance(w, NVFP4Tensor):
        raise NotImplementedError("NVFP4Tensor: weight must be NVFP4Tensor")
    if isinstance(x, NVFP4Tensor):
        x = x.to_dtype(x._orig_dtype)
    k = w.act_quant_kwargs
    if k is not None:
        if k.use_triton_kernel:
            raise NotImplementedError(NO_TRITON)
        assert k.block_size == 16, "NVFP4 requires block_size=16"
    transposed, (N, K) = w._rows_cols()
    if (x.is_cuda and x.dtype == torch.bfloat16 and w._orig_dtype == torch.bfloat16
            and w.qdata.is_cuda and not transposed and w.qdata.is_contiguous() and _hip_shape(N, K)
            and _hip_scale(w._per_tensor_scale, x) and _hip_scale(w._act_per_tensor_scale, x)):
        return torch.ops.torchao.nvfp4_linear(
            x, w.qdata, w._scale_e4m3.view(torch.uint8).reshape(-1), w._per_tensor_scale, bias,
            w._is_swizzled_scales, k is not None, None if k is None else w._act_per_tensor_scale)
    if k is None:  # the reference's weight-only form
        return torch.nn.functional.linear(x, w.to_dtype(w._orig_dtype), bias)
    # DYNAMIC, in fp32 with one rounding
    codes = (w.qdata.t() if transposed else w.qdata).contiguous()
    wd = (_e2m1_values(codes).view(N, -1, 16)
          * w._plain_scales().to(torch.float32).unsqueeze(-1)).view(N, K)
    y = _snap(x, w._act_per_tensor_scale) @ wd.t()
    for s in (w._per_tensor_scale, w._act_per_tensor_scale):
        if s is not None:
            y = y * s.to(torch.float32)
    if bias is not None:
        y = y + bias.to(torch.float32)
    return y.to(x.dtype).reshape(*x.shape[:-1], N)


@implements([torch.nn.functional.linear, aten.linear.default])
def _(func, types, args, kwargs):
    bias = args[2] if len(args) > 2 else kwargs.get("bias", None)
    return _nvfp4_linear(args[0], args[1], bias)


@implements([aten.mm.default, aten.matmul.default])
def _(func, types, args, kwargs):
    if not isinstance(args[1], NVFP4Tensor):
        raise NotImplementedError("NVFP4Tensor: weight must be NVFP4Tensor")
    return _nvfp4_linear(args[0], args[1].t(), None)


@implements(aten.addmm.default)
def _(func, types, args, kwargs):
    if not isinstance(args[2], NVFP4Tensor):
        raise NotImplementedError("NVFP4Tensor: weight must be NVFP4Tensor")
    return _nvfp4_linear(args[1], args[2].t(), args[0])


# ---- tensor plumbing ----------------------------------------------------------------------------
@implements([aten.detach.default, aten.alias.default])
def _(func, types, args, kwargs):
    return return_and_correct_aliasing(func, args, kwargs, args[0]._apply_fn_to_data(func))


@implements(aten.clone.default)
def _(func, types, args, kwargs):
    fmt = kwargs.get("memory_format", None)
    return args[0]._apply_fn_to_data(
        (lambda t: t.clone()) if fmt is None else (lambda t: t.clone(memory_format=fmt)))


@implements(aten._to_copy.default)
def _(func, types, args, kwargs):
    """Device movement, and a change of the dtype the tensor dequantizes to."""
    src, dtype, device = args[0], kwargs.get("dtype"), kwargs.get("device")
    if dtype is not None:
        assert dtype in (torch.float16, torch.bfloat16, torch.float32), (
            "Only support floating point conversion for autocast w/ NVFP4Tensor")
    out = src if device is None else src._apply_fn_to_data(lambda t: t.to(device=device))
    if dtype is not None and dtype != out._orig_dtype:
        out = out._with(out.qdata, out._scale_e4m3, dtype)
    return out._apply_fn_to_data(torch.clone) if out is src else out


@implements(aten.copy_.default)
def _(func, types, args, kwargs):
    dst, src = args[0], args[1]
    if NVFP4Tensor._same_metadata(dst, src):
        for name in dst._data_names():
            getattr(dst, name).copy_(getattr(src, name))
        return dst
    raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst}, {src}")


@implements(aten.t.default)
def _(func, types, args, kwargs):
    return args[0]._with(args[0].qdata.t(), args[0]._scale_e4m3)


@implements(aten.view.default)
def _(func, types, args, kwargs):
    src, size = args[0], list(args[1])
    size[-1 if src.qdata.is_contiguous() else 0] //= 2
    return src._with(func(src.qdata, size, *args[2:], **kwargs), src._scale_e4m3)


def _aligned(what, name, value, limit, step):
    """The reference's alignment rule of a swizzled slice: a multiple of step, or the end."""
    if value is not None and value != limit and value % step != 0:
        tail = "" if name == "start" else f" or equal to tensor size {limit}"
        raise RuntimeError(f"{what} slicing of NVFP4Tensor with swizzled scales requires {name} "
                           f"index to be a multiple of {step}{tail}, got {value}")


@implements(aten.slice.Tensor)
def _(func, types, args, kwargs):
    x, dim, start, end, step = fill_defaults(args, 5, [0, None, None, 1])
    if step != 1:
        raise ValueError("Only support aten.slice with step=1")
    if dim not in (0, 1):
        raise ValueError(f"NVFP4Tensor only supports slicing along dimensions 0 and 1, got dim={dim}")
    assert x.qdata.is_contiguous(), "Only support contiguous data for now"
    M, K = x.shape
    limit = (M, K)[dim]
    if end is not None and end >= min(limit, sys.maxsize):
        end = limit
    if dim == 1:
        for name, v in (("Start", start), ("End", end)):
            if v is not None and v % 2 != 0:
                raise RuntimeError(f"{name} index {v} must be even for FP4 packing")
    if x._is_swizzled_scales:
        # whole 128-row / 64-column tiles only: the tiles of the flat buffer are kept or dropped
        _aligned(("Row", "Column")[dim], "start", None if not start else start, -1, (128, 64)[dim])
        _aligned(("Row", "Column")[dim], "end", end, limit, (128, 64)[dim])
        nrb, ncb = ceil_div(M, 128), ceil_div(K // x._block_size, 4)
        tiles = x._scale_e4m3.view(nrb, ncb, 512)
        lo = (start or 0) // (128, 64)[dim]
        hi = (nrb, ncb)[dim] if end is None or end == limit else end // (128, 64)[dim]
        tiles = tiles[lo:hi] if dim == 0 else tiles[:, lo:hi]
        scales = tiles.reshape(-1)
    else:
        if dim == 1:
            for name, v in (("Start", start), ("End", end)):
                assert v is None or v % x._block_size == 0, (
                    f"{name} index {v} must be a multiple of block_size {x._block_size}")
        per = 1 if dim == 0 else x._block_size
        scales = aten.slice.Tensor(x._scale_e4m3.view(M, K // x._block_size), dim,
                                   None if start is None else start // per,
                                   None if end is None else end // per, 1).flatten()
    per = 1 if dim == 0 else 2
    qdata = aten.slice.Tensor(x.qdata, dim, None if start is None else start // per,
                              None if end is None else end // per, 1)
    return return_and_correct_aliasing(func, args, kwargs, x._with(qdata, scales))


torch.serialization.add_safe_globals([NVFP4Tensor, NVFP4MMConfig, QuantizeTensorToNVFP4Kwargs])
