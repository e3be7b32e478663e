"""Float8 layout of ``AffineQuantizedTensor`` and the e4m3fn weight-only linear on MI355X.

Reference: torchao/dtypes/floatx/float8_layout.py. ``Float8AQTTensorImpl`` (:76-231) keeps the
float8 data and its fp32 scale as plain tensors plus a ``transposed`` flag; attribute names,
flatten order and module path are the reference's, so a ``state_dict`` it saved with
``Float8WeightOnlyConfig(version=1)`` loads here with ``torch.load(weights_only=True)``.

Two quantized-linear pairs are registered from here (affine_quantized_tensor_ops.py):

* float activation x float8 weight (:370-396). The reference runs
  ``F.linear(x, weight.dequantize(), bias)``: a bf16 copy of W is written and read back on every
  call. Here ``torch.ops.torchao.fp8_weight_only_linear`` reads the e4m3fn codes once (HIP GEMV up
  to the GEMV crossover, bf16-MFMA tiles above) and applies the per-row scale once per output.
* float8 activation x float8 weight (:313-367, ``Float8DynamicActivationFloat8WeightConfig``).
  The reference calls ``torch._scaled_mm`` with row-wise scales; here
  ``torch.ops.torchao.fp8_scaled_mm`` runs the product on the fp8 matrix cores (HIP GEMV up to the
  crossover) with both fp32 scales and the bias in one epilogue, rounded to bf16 once.

Only per-row scaled e4m3fn operands are served; e5m2 and per-tensor scales are out of scope and
raise.
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch.utils._python_dispatch import (
    is_traceable_wrapper_subclass,
    return_and_correct_aliasing,
)

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.utils import AQTTensorImpl, Layout
from torchao.float8.inference import Float8MMConfig
from torchao.quantization.quant_primitives import FP8_TYPES
from torchao.utils import fill_defaults

aten = torch.ops.aten

__all__ = ["Float8MMConfig", "Float8Layout", "Float8AQTTensorImpl"]


@dataclass(frozen=True)
class Float8Layout(Layout):
    """Float8 data + fp32 scale kept as plain tensors. ``mm_config``: see ``Float8MMConfig``
    (None for weight-only quantization)."""

    mm_config: Optional[Float8MMConfig] = None


@register_layout(Float8Layout)
class Float8AQTTensorImpl(AQTTensorImpl):
    """``float8_data`` / ``scale`` as they are; ``transposed`` records a ``t()`` without moving
    data (the outer tensor's shape carries the transpose)."""

    def __new__(cls, float8_data, scale, transposed, _layout):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            float8_data.shape,
            device=float8_data.device,
            layout=float8_data.layout,
            dtype=float8_data.dtype,
            requires_grad=False,
        )

    def __init__(
        self,
        float8_data: torch.Tensor,
        scale: torch.Tensor,
        transposed: bool,
        _layout: Layout,
    ):
        self.float8_data = float8_data
        self.scale = scale
        self.transposed = transposed
        self._layout = _layout

    def __tensor_flatten__(self):
        return ["float8_data", "scale"], [self.transposed, self._layout]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        transposed, layout = tensor_attributes
        return cls(tensor_data_dict["float8_data"], tensor_data_dict["scale"], transposed, layout)

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return type(self)(
            self.float8_data.to(device), self.scale.to(device), self.transposed, self._layout
        )

    def _apply_fn_to_data(self, fn):
        return type(self)(fn(self.float8_data), fn(self.scale), self.transposed, self._layout)

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs):
        kwargs = {} if kwargs is None else kwargs
        if func in (aten.detach.default, aten.alias.default, aten.clone.default):
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(func)
            )
        if func is aten._to_copy.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0].to(*args[1:], **kwargs)._apply_fn_to_data(torch.clone)
            )
        if func is aten.t.default:
            t = args[0]
            new = cls(t.float8_data, t.scale, not t.transposed, t._layout)
            return return_and_correct_aliasing(func, args, kwargs, new)
        if func is aten.copy_.default:
            dst, src = args[0], args[1]
            if (
                isinstance(src, cls)
                and dst.float8_data.shape == src.float8_data.shape
                and dst.scale.shape == src.scale.shape
                and bool(dst.transposed) == bool(src.transposed)
                and type(dst._layout) is type(src._layout)
            ):
                dst.float8_data.copy_(src.float8_data)
                dst.scale.copy_(src.scale)
                return
            raise ValueError(f"Not supported args for copy_ due to metadata mismatch: {dst, src}")
        if func in (aten.select.int, aten.index.Tensor):
            return return_and_correct_aliasing(
                func,
                args,
                kwargs,
                args[0]._apply_fn_to_data(lambda t: func(t, *args[1:], **kwargs)),
            )
        if func is aten.slice.Tensor:
            self, dim, start, end, step = fill_defaults(args, 5, [0, None, None, 1])
            assert step == 1, "only step 1 slicing is supported"
            assert dim in (0, 1), f"Float8AQTTensorImpl: slice on dim {dim} is not supported"
            data = aten.slice.Tensor(self.float8_data, dim, start, end, step)
            scale = self.scale
            if scale.numel() != 1:
                # one scale per block along `dim`: per-row scales follow a row slice and are
                # untouched by a slice inside their own (whole-row) block
                per = self.float8_data.shape[dim] // scale.shape[dim]
                if per == 1:
                    scale = aten.slice.Tensor(scale, dim, start, end, step)
                elif per != self.float8_data.shape[dim]:
                    raise NotImplementedError(
                        "Float8AQTTensorImpl: slicing across scale blocks is not supported"
                    )
            return return_and_correct_aliasing(
                func, args, kwargs, cls(data, scale, self.transposed, self._layout)
            )
        raise NotImplementedError(f"Float8AQTTensorImpl dispatch: {func} is not supported")

    __torch_function__ = torch._C._disabled_torch_function_impl

    def get_plain(self) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        return self.float8_data, self.scale, None

    def get_layout(self) -> Layout:
        return self._layout

    @classmethod
    def from_plain(cls, data, scale, zero_point, _layout):
        assert data.dtype in FP8_TYPES, (
            f"Float8 TensorImpl must be constructed from float8 dtype but got {data.dtype}"
        )
        assert isinstance(_layout, Float8Layout), (
            f"Float8 TensorImpl must be constructed from Float8Layout but got {_layout}"
        )
        return cls(data, scale, False, _layout)

    def __repr__(self):
        return (
            f"{type(self).__name__}(float8_data={self.float8_data}, scale={self.scale}, "
            f"transposed={self.transposed}, _layout={self._layout})"
        )


def _is_rowwise_scaled(aqt) -> bool:
    """One scale per row of a 2-D weight: block_size (1, K)."""
    return (
        len(aqt.shape) == 2
        and len(aqt.block_size) == 2
        and aqt.block_size[0] == 1
        and aqt.block_size[1] == aqt.shape[1]
    )


def _linear_fp_act_fp8_weight_check(input_tensor, weight_tensor, bias) -> bool:
    return (
        not is_traceable_wrapper_subclass(input_tensor)
        and input_tensor.is_floating_point()
        and isinstance(weight_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor._layout, Float8Layout)
        and weight_tensor.tensor_impl.dtype == torch.float8_e4m3fn
        and not weight_tensor.tensor_impl.transposed
        and _is_rowwise_scaled(weight_tensor)
    )


def _linear_fp_act_fp8_weight_impl(input_tensor, weight_tensor, bias):
    """y = bf16((x @ f(W)^T) * scale) (+ bias), W e4m3fn per-row scaled (reference :391-396).
    bf16 inputs on the GPU run the HIP kernels; any other input raises from the op (a missing
    kernel is an error, never a quiet dequantize -> F.linear)."""
    impl = weight_tensor.tensor_impl
    return torch.ops.torchao.fp8_weight_only_linear(
        input_tensor, impl.float8_data, impl.scale.reshape(-1), bias
    )


def _is_rowwise_scaled_nd(aqt) -> bool:
    """One scale per row of a tensor of any rank (an activation [..., K]): block (1, ..., 1, K)."""
    return tuple(aqt.block_size) == (1,) * (len(aqt.shape) - 1) + (aqt.shape[-1],)


def _linear_fp8_act_fp8_weight_check(input_tensor, weight_tensor, bias) -> bool:
    def check_aqt(aqt) -> bool:
        return (
            isinstance(aqt, AffineQuantizedTensor)
            and isinstance(aqt._layout, Float8Layout)
            and aqt.tensor_impl.dtype in FP8_TYPES
            and (tuple(aqt.shape) == tuple(aqt.block_size) or _is_rowwise_scaled_nd(aqt))
        )

    return check_aqt(input_tensor) and check_aqt(weight_tensor)


def _linear_fp8_act_fp8_weight_impl(input_tensor, weight_tensor, bias):
    """y = bf16(((f(xq) @ f(wq)^T) * x_scale[m]) * w_scale[n] + bias) (reference :329-367, its
    row-wise ``torch._scaled_mm``). Only per-row scaled e4m3fn operands with an untransposed
    weight; anything else the check lets through raises (no quiet dequantize -> F.linear)."""
    assert weight_tensor._layout.mm_config is not None
    x_impl, w_impl = input_tensor.tensor_impl, weight_tensor.tensor_impl
    if w_impl.transposed or x_impl.transposed:
        raise NotImplementedError("float8 x float8 linear: a transposed operand is not supported")
    if not (_is_rowwise_scaled_nd(input_tensor) and _is_rowwise_scaled(weight_tensor)):
        raise NotImplementedError(
            "float8 x float8 linear: only per-row scales (granularity=PerRow()) are supported"
        )
    if x_impl.dtype != torch.float8_e4m3fn or w_impl.dtype != torch.float8_e4m3fn:
        raise NotImplementedError("float8 x float8 linear: only torch.float8_e4m3fn is supported")
    return torch.ops.torchao.fp8_scaled_mm(
        x_impl.float8_data, x_impl.scale, w_impl.float8_data, w_impl.scale.reshape(-1), bias
    )
