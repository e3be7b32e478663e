"""2:4 sparse int4 weight-only layout (reference torchao/dtypes/uintx/marlin_sparse_layout.py), for
``Int4WeightOnlyConfig(layout=MarlinSparseLayout())``.

The reference pre-packs the weight for its CUDA-only, fp16-only ``marlin_24_gemm``. Here the storage
is ours and documented (csrc/int4_sparse24.hip, DESIGN.md "2:4 sparse int4"); the reference's
checkpoints of this layout do not load:

* ``int_data`` int32 [N, K/16]: dword j holds the eight kept uint4 codes of dense k
  16 j .. 16 j + 15, code i in bits [4i+3:4i] (zero point 8: a pruned weight is code 8);
* ``meta`` int32 [N, K/32]: sixteen 2-bit positions per dword (``SemiSparseLayout``'s);
* ``scale`` [K/group_size, N], group-major: the order the GEMM's epilogue loads;
* ``zero_point`` [N, K/group_size], all 8, kept for ``get_plain``.

0.375 B per dense weight plus scales. bf16 activations on the GPU run
``torch.ops.torchao.int4_sp24_weight_only_linear``; CPU tensors and other dtypes take
``F.linear`` on the dequantized weight (the reference raises there).
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch.utils._python_dispatch import return_and_correct_aliasing

from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor, register_layout
from torchao.dtypes.uintx.semi_sparse_layout import SemiSparseLayout
from torchao.dtypes.utils import AQTTensorImpl, Layout
from torchao.quantization.quant_primitives import ZeroPointDomain

aten = torch.ops.aten

__all__ = ["MarlinSparseLayout", "MarlinSparseAQTTensorImpl"]


@dataclass(frozen=True)
class MarlinSparseLayout(Layout):
    """``pre_process`` prunes the weight 2:4 along the input features with ``SemiSparseLayout``'s
    rule (of equal magnitudes the lower index is pruned first)."""

    def pre_process(self, input: torch.Tensor) -> torch.Tensor:
        return SemiSparseLayout().pre_process(input)


@register_layout(MarlinSparseLayout)
class MarlinSparseAQTTensorImpl(AQTTensorImpl):
    """Compressed codes, positions and scales of a 2:4 sparse uint4 weight."""

    def __new__(cls, int_data, scale, zero_point, meta, _layout, original_shape, group_size,
                num_bits):
        return torch.Tensor._make_wrapper_subclass(
            cls,
            tuple(original_shape),
            device=int_data.device,
            layout=int_data.layout,
            dtype=int_data.dtype,
            requires_grad=False,
        )

    def __init__(
        self,
        int_data: torch.Tensor,
        scale: torch.Tensor,
        zero_point: torch.Tensor,
        meta: torch.Tensor,
        _layout: Layout,
        original_shape: torch.Size,
        group_size: int,
        num_bits: int,
    ):
        self.int_data = int_data
        self.scale = scale
        self.zero_point = zero_point
        self.meta = meta
        self._layout = _layout
        self.original_shape = torch.Size(original_shape)
        self.group_size = group_size
        self.num_bits = num_bits

    def __tensor_flatten__(self):
        return ["int_data", "scale", "zero_point", "meta"], [
            self._layout, self.original_shape, self.group_size, self.num_bits]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        layout, original_shape, group_size, num_bits = tensor_attributes
        return cls(
            tensor_data_dict["int_data"],
            tensor_data_dict["scale"],
            tensor_data_dict["zero_point"],
            tensor_data_dict["meta"],
            layout,
            original_shape,
            group_size,
            num_bits,
        )

    def _apply_fn_to_data(self, fn):
        return type(self)(
            fn(self.int_data),
            fn(self.scale),
            fn(self.zero_point),
            fn(self.meta),
            self._layout,
            self.original_shape,
            self.group_size,
            self.num_bits,
        )

    def to(self, *args, **kwargs):
        device = self._get_to_kwargs(*args, **kwargs)["device"]
        return self._apply_fn_to_data(lambda t: t.to(device))

    @classmethod
    def __torch_dispatch__(cls, func, types, args, kwargs):
        kwargs = {} if kwargs is None else kwargs
        if func is aten.detach.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.detach)
            )
        if func is aten.clone.default:
            return return_and_correct_aliasing(
                func, args, kwargs, args[0]._apply_fn_to_data(torch.clone)
            )
        raise NotImplementedError(f"MarlinSparseAQTTensorImpl dispatch: {func} is not supported")

    __torch_function__ = torch._C._disabled_torch_function_impl

    def get_plain(self) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """int32 codes [N, K] (8 where pruned), scale and zero point [N, K/group_size]."""
        codes = torch.ops.torchao.int4_sp24_decompress(self.int_data, self.meta)
        return codes, self.scale.t(), self.zero_point

    def get_layout(self) -> Layout:
        return self._layout

    @classmethod
    def from_plain(cls, int_data, scale, zero_point, _layout):
        assert isinstance(_layout, MarlinSparseLayout)
        if int_data.dim() != 2 or int_data.shape[1] % 128 != 0:
            raise NotImplementedError(
                "MarlinSparseLayout serves 2-D weights whose in_features are a multiple of 128, "
                f"got {tuple(int_data.shape)}"
            )
        N, K = int_data.shape
        scale = scale.reshape(N, -1)
        group_size = K // scale.shape[1]
        values, meta, err = torch.ops.torchao.int4_sp24_compress(
            int_data.to(torch.int32).contiguous())
        if int(err.item()) != 0:  # a host sync, at quantization time only
            raise ValueError(
                "MarlinSparseLayout: the weight is not 2:4 sparse (a group of four input features "
                "holds more than two codes other than the zero point 8)"
            )
        return cls(values, scale.t().contiguous(), zero_point.reshape(N, -1), meta, _layout,
                   int_data.shape, group_size, 4)


torch.serialization.add_safe_globals([MarlinSparseLayout, MarlinSparseAQTTensorImpl])


def _linear_fp_act_int4_weight_sparse_marlin_check(input_tensor, weight_tensor, bias) -> bool:
    return (
        not isinstance(input_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor, AffineQuantizedTensor)
        and isinstance(weight_tensor._layout, MarlinSparseLayout)
        and len(weight_tensor.shape) == 2
        and weight_tensor.zero_point_domain == ZeroPointDomain.INT
    )


def _linear_fp_act_int4_weight_sparse_marlin_impl(input_tensor, weight_tensor, bias):
    """bf16 on the GPU: the HIP op on the compressed weight. Anything else (CPU tensors, fp16,
    fp32): ``F.linear`` on the dequantized weight in plain torch."""
    impl = weight_tensor.tensor_impl
    if (input_tensor.is_cuda and input_tensor.dtype == torch.bfloat16
            and weight_tensor.dtype == torch.bfloat16 and impl.int_data.is_cuda):
        return torch.ops.torchao.int4_sp24_weight_only_linear(
            input_tensor, impl.int_data, impl.meta, impl.scale, impl.group_size, bias)
    return torch.nn.functional.linear(
        input_tensor, weight_tensor.dequantize().to(input_tensor.dtype), bias)
