"""``AffineQuantizedTensor`` — the quantized-weight tensor subclass.

Mirrors the reference (torchao/dtypes/affine_quantized_tensor.py:57-614) for the integer
workflows on the hot path: ``from_hp_to_intx`` (pre_process -> choose_qparams -> quantize ->
post_process -> layout constructor, :231-373), ``from_hp_to_intx_static``, ``dequantize``
(:134-196), flatten/unflatten (:198-229), ``to`` and ``_apply_fn_to_data``, and the float8
weight-only constructor ``from_hp_to_floatx`` (:449-480; e4m3fn, ``Float8Layout``) and the FP6
constructor ``from_hp_to_fpx`` (:526-553; ``FloatxTensorCoreLayout``), and the HQQ branch of
``from_hp_to_intx`` (:252-288). The static float8 constructor belongs to an out-of-scope workflow
and is not provided.
"""

import logging
import math
from typing import Optional, Tuple, Union

import torch

from torchao.dtypes.utils import AQTTensorImpl, Layout, PlainLayout
from torchao.quantization.quant_primitives import (
    MappingType,
    ZeroPointDomain,
    FLOATX_SERVED,
    FP8_TYPES,
    _choose_qparams_affine_floatx,
    _choose_qparams_affine_tinygemm,
    _choose_qparams_and_quantize_affine_hqq,
    _dequantize_affine_floatx,
    _quantize_affine_floatx,
    _choose_scale_float8,
    _dequantize_affine_float8,
    _dequantize_affine_no_zero_point,
    _dequantize_affine_tinygemm,
    _quantize_affine_float8,
    _quantize_affine_no_zero_point,
    _quantize_affine_tinygemm,
    choose_qparams_affine,
    dequantize_affine,
    quantize_affine,
)
from torchao.utils import TorchAOBaseTensor

logger = logging.getLogger(__name__)
aten = torch.ops.aten

__all__ = [
    "AffineQuantizedTensor",
    "register_layout",
    "to_affine_quantized_intx",
    "to_affine_quantized_intx_static",
    "to_affine_quantized_floatx",
    "to_affine_quantized_fpx",
]


def _fused_weight_quant(x, mapping_type, block_size, target_dtype, quant_min, quant_max, eps,
                        scale_dtype, zero_point_dtype, preserve_zero, zero_point_domain, layout):
    """The tensor impl from one fused gfx950 quantizer kernel, or None to take the torch-op
    path. Covers the two weight recipes of the hot path on bf16 CUDA weights, with results
    bit-identical to the torch-op path (tests/test_gpu_quantize.py):
      * int4 tinygemm (Int4WeightOnlyConfig): ASYMMETRIC, FLOAT zero domain, preserve_zero
        False, [0, 15], blocks (1, ..., g) -> torchao::int4_quantize_pack straight into the
        TensorCoreTiledLayout impl (no int32 [N, K] intermediate, no separate pack);
      * int8 symmetric per row (Int8WeightOnlyConfig, int8 dyn weights): SYMMETRIC, blocks
        (1, ..., K), [-128, 127] -> torchao::int8_quantize_rows into the PlainLayout impl;
      * the two W4A8 recipes (Int8DynamicActivationInt4WeightConfig with CutlassInt4PackedLayout):
        SYMMETRIC per row, no zero point, float32 scale, eps = finfo(float32).eps; int8 into
        PlainLayout (the activation) -> torchao::int8_quantize_per_token_f32, [-8, 7] into
        CutlassInt4PackedLayout (the weight) -> torchao::int4_quantize_rows_packed
        (tests/test_gpu_w4a8.py)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() in (2, 3) and eps is not None):
        return None
    if any(b != 1 for b in block_size[:-1]):
        return None
    K = x.shape[-1]
    g = block_size[-1]
    from torchao.dtypes.uintx.tensor_core_tiled_layout import (
        TensorCoreTiledAQTTensorImpl,
        TensorCoreTiledLayout,
    )

    if (
        isinstance(layout, TensorCoreTiledLayout)
        and mapping_type is MappingType.ASYMMETRIC
        and zero_point_domain == ZeroPointDomain.FLOAT
        and not preserve_zero
        and target_dtype == torch.int32
        and (quant_min, quant_max) == (0, 15)
        and g in (32, 64, 128, 256)
        and K % g == 0
        and scale_dtype in (None, torch.bfloat16)
        and zero_point_dtype in (None, torch.bfloat16)
    ):
        packed, sz = torch.ops.torchao.int4_quantize_pack(x, g, float(eps))
        return TensorCoreTiledAQTTensorImpl(packed, sz, False, layout)
    if (
        type(layout) is PlainLayout
        and mapping_type is MappingType.SYMMETRIC
        and zero_point_domain in (ZeroPointDomain.INT, ZeroPointDomain.NONE)
        and preserve_zero
        and target_dtype == torch.int8
        and quant_min in (None, -128)
        and quant_max in (None, 127)
        and g == K
        and K % 8 == 0
        and scale_dtype in (None, torch.bfloat16)
    ):
        q, scale = torch.ops.torchao.int8_quantize_rows(x, float(eps))
        zero_point = None
        if zero_point_domain == ZeroPointDomain.INT:
            zero_point = torch.zeros_like(scale, dtype=zero_point_dtype or torch.int32)
        q, scale, zero_point = layout.post_process(q, scale, zero_point, block_size)
        return AffineQuantizedTensor.get_tensor_impl_constructor(type(layout))(
            q, scale, zero_point, layout
        )
    # The two W4A8 recipes (quant_api._int8_symm_cutlass_quant / _int4_symm_cutlass_quant):
    # SYMMETRIC per row, no zero point, float32 scale clamped at finfo(float32).eps.
    w4a8 = (
        mapping_type is MappingType.SYMMETRIC
        and zero_point_domain == ZeroPointDomain.NONE
        and preserve_zero
        and target_dtype == torch.int8
        and g == K
        and K % 8 == 0
        and scale_dtype == torch.float32
        and float(eps) == float(torch.finfo(torch.float32).eps)
    )
    if w4a8 and type(layout) is PlainLayout and quant_min in (None, -128) and quant_max in (None, 127):
        q, scale = torch.ops.torchao.int8_quantize_per_token_f32(x)
        return AffineQuantizedTensor.get_tensor_impl_constructor(type(layout))(
            q, scale, None, layout
        )
    from torchao.dtypes.uintx.cutlass_int4_packed_layout import (
        CutlassInt4PackedLayout,
        Int4PackedTensorImpl,
    )

    if (w4a8 and isinstance(layout, CutlassInt4PackedLayout) and x.dim() == 2
            and (quant_min, quant_max) == (-8, 7)):
        packed, scale = torch.ops.torchao.int4_quantize_rows_packed(x)
        return Int4PackedTensorImpl(packed, scale, layout)
    return None


def _adopt_loaded_impl(impl, shape):
    """A layout impl may recognise storage written by another build and convert it
    (``_adopt(shape)``, e.g. the reference's int4 tile format); others pass through."""
    adopt = getattr(type(impl), "_adopt", None)
    return impl if adopt is None else adopt(impl, tuple(shape))


class AffineQuantizedTensor(TorchAOBaseTensor):
    """float_tensor ~= dequantize(tensor_impl) with qparams shared over ``block_size`` blocks.

    fields: ``tensor_impl`` (layout-specific storage), ``block_size``, ``shape`` (of the
    original high-precision tensor), ``quant_min`` / ``quant_max``, ``zero_point_domain``,
    ``dtype`` (of the original high-precision tensor).
    """

    @staticmethod
    def __new__(
        cls,
        tensor_impl: AQTTensorImpl,
        block_size: Tuple[int, ...],
        shape: torch.Size,
        quant_min: Optional[Union[int, float]] = None,
        quant_max: Optional[Union[int, float]] = None,
        zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
        dtype=None,
        strides=None,
    ):
        if zero_point_domain is None:
            raise ValueError("please use ZeroPointDomain.NONE instead of None")
        kwargs = {
            "device": tensor_impl.device,
            "layout": tensor_impl.layout,
            "dtype": dtype,
            "requires_grad": False,
        }
        if strides is not None:
            kwargs["strides"] = strides
        return torch.Tensor._make_wrapper_subclass(cls, shape, **kwargs)

    def __init__(
        self,
        tensor_impl: AQTTensorImpl,
        block_size: Tuple[int, ...],
        shape: torch.Size,
        quant_min: Optional[Union[int, float]] = None,
        quant_max: Optional[Union[int, float]] = None,
        zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
        dtype=None,
        strides=None,
    ):
        self.tensor_impl = tensor_impl
        self.block_size = block_size
        self.quant_min = quant_min
        self.quant_max = quant_max
        self.zero_point_domain = zero_point_domain

    def __repr__(self):
        return (
            f"{type(self).__name__}(tensor_impl={self.tensor_impl}, block_size={self.block_size}, "
            f"shape={self.shape}, device={self.device}, dtype={self.dtype}, "
            f"requires_grad={self.requires_grad})"
        )

    def _quantization_type(self):
        return (
            f"shape={self.shape}, block_size={self.block_size}, device={self.device}, "
            f"_layout={self._layout}, tensor_impl_dtype={self.tensor_impl.dtype}, "
            f"quant_min={self.quant_min}, quant_max={self.quant_max}"
        )

    @property
    def _layout(self) -> Layout:
        return self.tensor_impl._layout

    def dequantize(self, output_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """High-precision tensor of ``self.shape``: get_plain() -> the domain's dequant formula."""
        output_dtype = self.dtype if output_dtype is None else output_dtype
        if hasattr(self.tensor_impl, "packed_floatx_data"):
            return self._dequantize_floatx(output_dtype)
        data, scale, zero_point = self.tensor_impl.get_plain()
        if data.dtype in FP8_TYPES:
            return self._dequantize_float8(data, scale, output_dtype)
        if self.zero_point_domain == ZeroPointDomain.FLOAT:
            fn = _dequantize_affine_tinygemm
        elif self.zero_point_domain == ZeroPointDomain.NONE:
            fn = _dequantize_affine_no_zero_point
        else:
            fn = dequantize_affine
        dq = fn(
            data,
            self.block_size,
            scale,
            zero_point,
            data.dtype,
            self.quant_min,
            self.quant_max,
            output_dtype=output_dtype,
        )
        # layouts may pad; return the logical shape
        for dim, size in enumerate(self.shape):
            if dq.shape[dim] != size:
                dq = dq.narrow(dim, 0, size)
        return dq

    def _dequantize_float8(self, data, scale, output_dtype):
        """float(q) * scale, rounded once to ``output_dtype`` (_dequantize_affine_float8,
        reference :149-151). Per-row e4m3fn data on the GPU with a bf16 result runs the HIP
        kernel (``torchao::fp8_dequantize``), bit-identical to the torch-op formulation."""
        if (
            data.is_cuda
            and output_dtype == torch.bfloat16
            and data.dtype == torch.float8_e4m3fn
            and data.dim() == 2
            and data.shape[1] % 8 == 0
            and scale.numel() == data.shape[0]
        ):
            dq = torch.ops.torchao.fp8_dequantize(data, scale.reshape(-1))
        else:
            dq = _dequantize_affine_float8(data, scale, output_dtype)
        return dq.t() if getattr(self.tensor_impl, "transposed", False) else dq

    def _dequantize_floatx(self, output_dtype):
        """bf16(fp32(value(code)) * fp32(scale)) of an FP6 weight (_dequantize_affine_floatx,
        reference :140-148). Native storage on the GPU with a bf16 scale and result runs the HIP
        kernel (``torchao::fp6_dequantize``), bit-identical to the torch-op formulation."""
        impl = self.tensor_impl
        ebits, mbits = impl._layout.ebits, impl._layout.mbits
        if impl.is_cuda and output_dtype == torch.bfloat16 and impl.scale.dtype == torch.bfloat16:
            return torch.ops.torchao.fp6_dequantize(impl._native(), impl.scale, ebits, mbits)
        codes, scale = impl.get_plain()
        return _dequantize_affine_floatx(codes, scale, ebits, mbits, output_dtype=output_dtype)

    def __tensor_flatten__(self):
        with torch._C.DisableTorchFunctionSubclass():
            return ["tensor_impl"], [
                self.block_size,
                self.shape,
                self.quant_min,
                self.quant_max,
                self.zero_point_domain,
                self.dtype,
            ]

    @classmethod
    def __tensor_unflatten__(cls, tensor_data_dict, tensor_attributes, outer_size, outer_stride):
        block_size, shape, quant_min, quant_max, zero_point_domain, dtype = tensor_attributes
        impl = _adopt_loaded_impl(tensor_data_dict["tensor_impl"],
                                  shape if outer_size is None else outer_size)
        return cls(
            impl,
            block_size,
            shape if outer_size is None else outer_size,
            quant_min,
            quant_max,
            zero_point_domain,
            dtype=dtype,
            strides=outer_stride,
        )

    def __setstate__(self, state):
        """Unpickling (torch.load): restore the fields, then let the layout adopt storage that
        another build wrote (a reference TensorCoreTiledLayout checkpoint holds the tile format;
        tensor_core_tiled_layout.convert_from_tensor_core_tiled)."""
        torch._utils._set_obj_state(self, state)
        self.tensor_impl = _adopt_loaded_impl(self.tensor_impl, self.shape)

    @classmethod
    def from_hp_to_intx(
        cls,
        input_float: torch.Tensor,
        mapping_type: MappingType,
        block_size: Tuple[int, ...],
        target_dtype: torch.dtype,
        quant_min: Optional[int] = None,
        quant_max: Optional[int] = None,
        eps: Optional[float] = None,
        scale_dtype: Optional[torch.dtype] = None,
        zero_point_dtype: Optional[torch.dtype] = None,
        preserve_zero: bool = True,
        zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
        _layout: Layout = PlainLayout(),
        use_hqq: bool = False,
    ):
        """Quantize a high-precision tensor into an integer AQT with ``_layout``."""
        original_shape = input_float.shape
        input_float = _layout.pre_process(input_float)
        if use_hqq:
            return cls._from_hp_to_intx_hqq(
                input_float, original_shape, mapping_type, block_size, target_dtype, quant_min,
                quant_max, zero_point_dtype, zero_point_domain, _layout,
            )
        fused = _fused_weight_quant(
            input_float, mapping_type, block_size, target_dtype, quant_min, quant_max, eps,
            scale_dtype, zero_point_dtype, preserve_zero, zero_point_domain, _layout,
        )
        if fused is not None:
            return cls(
                fused,
                block_size,
                original_shape,
                quant_min,
                quant_max,
                zero_point_domain,
                dtype=input_float.dtype,
            )
        if zero_point_domain == ZeroPointDomain.FLOAT and not preserve_zero:
            scale, zero_point = _choose_qparams_affine_tinygemm(
                input_float, mapping_type, block_size, target_dtype, quant_min, quant_max, eps,
                scale_dtype, zero_point_dtype,
            )
        elif not preserve_zero:
            raise NotImplementedError(
                "preserve_zero=False with an integer zero point is outside the hot-path scope"
            )
        else:
            scale, zero_point = choose_qparams_affine(
                input_float, mapping_type, block_size, target_dtype, quant_min, quant_max, eps,
                scale_dtype, zero_point_dtype,
            )
        if zero_point_domain == ZeroPointDomain.NONE:
            zero_point = None
            data = _quantize_affine_no_zero_point(
                input_float, block_size, scale, zero_point, target_dtype, quant_min, quant_max
            )
        elif zero_point_domain == ZeroPointDomain.FLOAT:
            data = _quantize_affine_tinygemm(
                input_float, block_size, scale, zero_point, target_dtype, quant_min, quant_max
            )
        else:
            data = quantize_affine(
                input_float, block_size, scale, zero_point, target_dtype, quant_min, quant_max
            )
        data, scale, zero_point = _layout.post_process(data, scale, zero_point, block_size)
        tensor_impl = cls.get_tensor_impl_constructor(type(_layout))(
            data, scale, zero_point, _layout
        )
        return cls(
            tensor_impl,
            block_size,
            original_shape,
            quant_min,
            quant_max,
            zero_point_domain,
            dtype=input_float.dtype,
        )

    @classmethod
    def _from_hp_to_intx_hqq(cls, input_float, original_shape, mapping_type, block_size,
                             target_dtype, quant_min, quant_max, zero_point_dtype,
                             zero_point_domain, _layout):
        """The ``use_hqq=True`` branch of ``from_hp_to_intx`` (reference :252-288), in fp32 on
        every device (the reference iterates in fp16 on a GPU; its CPU arithmetic is served here).

        A bf16 CUDA weight with ``TensorCoreTiledLayout``, [0, 15] and g in {32, 64, 128, 256}
        runs the fused HIP quantizer (``torchao::int4_hqq_quantize_pack``) straight into the
        layout's storage; everything else runs the plain-torch function and the layout's pack."""
        assert (
            zero_point_domain == ZeroPointDomain.FLOAT
            and mapping_type == MappingType.ASYMMETRIC
            and quant_min == 0
        ), "Invalid input parameters for HQQ quantization."
        from torchao.dtypes.uintx.tensor_core_tiled_layout import (
            TensorCoreTiledAQTTensorImpl,
            TensorCoreTiledLayout,
        )

        if not isinstance(_layout, (TensorCoreTiledLayout, PlainLayout)):
            raise NotImplementedError(f"HQQ (raw_output) is not served for {type(_layout).__name__}")
        if block_size[0] != 1:
            raise NotImplementedError("HQQ along axis 0 is not served")
        nbits = int(math.log2(quant_max + 1))
        group_size = max(block_size)
        compute_dtype = zero_point_dtype if zero_point_dtype is not None else input_float.dtype
        if (
            input_float.is_cuda
            and input_float.dtype == torch.bfloat16
            and input_float.dim() in (2, 3)
            and isinstance(_layout, TensorCoreTiledLayout)
            and all(b == 1 for b in block_size[:-1])
            and target_dtype == torch.int32
            and quant_max == 15
            and group_size in (32, 64, 128, 256)
            and input_float.shape[-1] % group_size == 0
            and compute_dtype == torch.bfloat16
        ):
            packed, sz, _ = torch.ops.torchao.int4_hqq_quantize_pack(input_float, group_size)
            tensor_impl = TensorCoreTiledAQTTensorImpl(packed, sz, False, _layout)
        else:
            data, scale, zero_point, _ = _choose_qparams_and_quantize_affine_hqq(
                input_float, nbits=nbits, group_size=group_size, axis=1,
                compute_dtype=compute_dtype, device=input_float.device, verbose=False,
                raw_output=False,
            )
            data = data.to(target_dtype)
            data, scale, zero_point = _layout.post_process(data, scale, zero_point, block_size)
            tensor_impl = cls.get_tensor_impl_constructor(type(_layout))(
                data, scale, zero_point, _layout
            )
        return cls(
            tensor_impl,
            block_size,
            original_shape,
            quant_min,
            quant_max,
            zero_point_domain,
            dtype=input_float.dtype,
        )

    @classmethod
    def from_hp_to_intx_static(
        cls,
        input_float: torch.Tensor,
        scale: torch.Tensor,
        zero_point: Optional[torch.Tensor],
        block_size: Tuple[int, ...],
        target_dtype: torch.dtype,
        quant_min: Optional[int] = None,
        quant_max: Optional[int] = None,
        zero_point_domain: ZeroPointDomain = ZeroPointDomain.INT,
        _layout: Layout = PlainLayout(),
    ):
        """Quantize with caller-supplied qparams."""
        if zero_point_domain is None:
            raise ValueError("please use ZeroPointDomain.NONE instead of None")
        if zero_point_domain is ZeroPointDomain.NONE and zero_point is not None:
            raise ValueError("zero_point should be None when zero_point_domain is NONE")
        original_shape = input_float.shape
        input_float, scale, zero_point = _layout.pre_process_static(
            input_float, scale, zero_point, block_size
        )
        if zero_point_domain == ZeroPointDomain.NONE:
            data = _quantize_affine_no_zero_point(
                input_float, block_size, scale, None, target_dtype, quant_min, quant_max
            )
        elif zero_point_domain == ZeroPointDomain.FLOAT:
            data = _quantize_affine_tinygemm(
                input_float, block_size, scale, zero_point, target_dtype, quant_min, quant_max
            )
        else:
            data = quantize_affine(
                input_float, block_size, scale, zero_point, target_dtype, quant_min, quant_max
            )
        data, scale, zero_point = _layout.post_process(data, scale, zero_point, block_size)
        tensor_impl = cls.get_tensor_impl_constructor(type(_layout))(
            data, scale, zero_point, _layout
        )
        return cls(
            tensor_impl,
            block_size,
            original_shape,
            quant_min,
            quant_max,
            zero_point_domain,
            dtype=input_float.dtype,
        )

    @classmethod
    def from_hp_to_floatx(
        cls,
        input_float: torch.Tensor,
        block_size: Tuple[int, ...],
        target_dtype: torch.dtype,
        _layout: Layout,
        scale_dtype: Optional[torch.dtype] = None,
    ):
        """Quantize a high-precision tensor into a float8 AQT with ``_layout`` (reference
        :449-480): scale = amax|block| / max (no eps), data = float8(clamp(x / scale)).

        bf16 CUDA weights with per-row blocks (1, ..., K) run the fused HIP quantizer
        (``torchao::fp8_quantize_rows``); everything else runs the torch-op formulation. The two
        agree byte for byte (tests/test_gpu_float8.py)."""
        if target_dtype != torch.float8_e4m3fn:
            raise NotImplementedError(
                f"Unsupported dtype {target_dtype} for from_hp_to_floatx: only "
                "torch.float8_e4m3fn is in scope"
            )
        original_shape = input_float.shape
        input_float = _layout.pre_process(input_float)
        K = input_float.shape[-1]
        if (
            input_float.is_cuda
            and input_float.dtype == torch.bfloat16
            and input_float.dim() in (2, 3)
            and all(b == 1 for b in block_size[:-1])
            and block_size[-1] == K
            and K % 8 == 0
        ):
            data, scale = torch.ops.torchao.fp8_quantize_rows(input_float)
        else:
            scale = _choose_scale_float8(
                input_float, float8_dtype=target_dtype, block_size=block_size
            )
            data = _quantize_affine_float8(input_float, scale, target_dtype)
        data, scale, zero_point = _layout.post_process(data, scale, None, block_size)
        tensor_impl = cls.get_tensor_impl_constructor(type(_layout))(
            data, scale, zero_point, _layout
        )
        return cls(tensor_impl, block_size, original_shape, dtype=input_float.dtype)

    @classmethod
    def from_hp_to_fpx(cls, input_float: torch.Tensor, _layout: Layout):
        """Quantize a 2-D high-precision tensor into an FP6 AQT (reference :526-553; ``_layout``
        a ``FloatxTensorCoreLayout`` of (3, 2) or (2, 3)): one scale per row in the tensor's dtype,
        codes rounded to nearest even and saturated.

        bf16 CUDA weights with K % 32 == 0 run the fused HIP quantizer
        (``torchao::fp6_quantize_rows``) straight into the native storage; everything else runs
        the torch-op formulation. The two agree bit for bit on finite rows
        (tests/test_gpu_fp6.py)."""
        from torchao.dtypes.floatx.floatx_tensor_core_layout import (
            FloatxTensorCoreAQTTensorImpl,
            FloatxTensorCoreLayout,
        )

        assert isinstance(_layout, FloatxTensorCoreLayout), (
            f"Only FloatxTensorCoreLayout is supported for floatx, got {_layout}"
        )
        ebits, mbits = _layout.ebits, _layout.mbits
        if (ebits, mbits) not in FLOATX_SERVED:
            raise NotImplementedError(
                f"floatx (ebits, mbits) = ({ebits}, {mbits}) is not served; served: the FP6 "
                f"formats (3, 2) and (2, 3)")
        assert input_float.dim() == 2, f"floatx only works for 2-d Tensor, got: {input_float.dim()}"
        original_shape = input_float.shape
        input_float = _layout.pre_process(input_float)
        # one scale per row (the reference spells this block size [N, 1])
        block_size = list(input_float.shape)
        block_size[1] = 1
        if (input_float.is_cuda and input_float.dtype == torch.bfloat16
                and input_float.shape[1] % 32 == 0):
            packed, scale = torch.ops.torchao.fp6_quantize_rows(input_float, ebits, mbits)
            tensor_impl = FloatxTensorCoreAQTTensorImpl(packed, scale, _layout)
        else:
            scale = _choose_qparams_affine_floatx(input_float, ebits, mbits)
            codes = _quantize_affine_floatx(input_float, scale, ebits, mbits)
            codes, scale, _ = _layout.post_process(codes, scale, None, block_size)
            tensor_impl = cls.get_tensor_impl_constructor(type(_layout))(
                codes, scale, None, _layout
            )
        return cls(tensor_impl, block_size, original_shape, dtype=input_float.dtype)

    def to(self, *args, **kwargs):
        kwargs = self._get_to_kwargs(*args, **kwargs)
        device = kwargs.pop("device")
        return type(self)(
            self.tensor_impl.to(device),
            self.block_size,
            self.shape,
            self.quant_min,
            self.quant_max,
            self.zero_point_domain,
            **kwargs,
        )

    def _apply_fn_to_data(self, fn):
        return type(self)(
            fn(self.tensor_impl),
            self.block_size,
            self.shape,
            self.quant_min,
            self.quant_max,
            self.zero_point_domain,
            dtype=self.dtype,
            strides=self.stride(),
        )


register_layout = AffineQuantizedTensor.register_layout
get_tensor_impl_constructor = AffineQuantizedTensor.get_tensor_impl_constructor
to_affine_quantized_intx = AffineQuantizedTensor.from_hp_to_intx
to_affine_quantized_intx_static = AffineQuantizedTensor.from_hp_to_intx_static
to_affine_quantized_floatx = AffineQuantizedTensor.from_hp_to_floatx
to_affine_quantized_fpx = AffineQuantizedTensor.from_hp_to_fpx

torch.serialization.add_safe_globals([AffineQuantizedTensor])
