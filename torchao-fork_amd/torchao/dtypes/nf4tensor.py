"""NF4 (QLoRA) weight tensor: ``NF4Tensor``, ``to_nf4``, ``linear_nf4``.

The format (that of the reference's torchao/dtypes/nf4tensor.py; attribute names, dtypes and
shapes are kept so that its checkpoints load): the contiguous weight ``W`` of dtype ``T`` is
flattened and cut into blocks of ``block_size`` (64); the per-block absmaxes are themselves
quantized to int8 in groups of ``scaler_block_size`` (256) around their mean.

  quantized_data       uint8 [numel / 2]     element 2j in the HIGH nibble of byte j
  quantized_scalers    int8  [n_blocks]
  quantization_factor  T     [n_blocks / scaler_block_size]
  scaler_mean          T     0-dim
  nf4                  T     [16]            the sixteen levels rounded to T

Every operation is the eager torch op on ``T`` tensors (evaluated in fp32, rounded to ``T`` once):

  quantize     a[b] = max|W| over block b;  v = T(W / a[b]);
               code = first j minimising T(|T(v - nf4[j])|)  (a NaN difference wins: an all-zero
               block has v = NaN and takes code 0)
               m = T(mean(a));  c = T(a - m);  per 256: A = max|c|, qf = T(256 / T(2 A)),
               q = int8(clamp(round_half_even(T(c qf)), -128, 127))
  dequantize   s[b] = T(T(float(q[b]) / qf[b / 256]) + m);  w^ = T(nf4[code] s[b])
  linear       y = T(sum_k x w^), fp32 sum over the T-rounded w^; a bias is a second rounding

Dispatch: bf16 HIP tensors with the default block sizes run the gfx950 kernels of csrc/nf4.hip
(``torch.ops.torchao.nf4_quantize_blocks / nf4_dequantize / nf4_linear``: the block quantizer in
one read with no numel x 16 intermediate, a streaming dequantizer, and for K % 64 == 0 the decode
GEMV up to 4 tokens and dequantize + bf16 matmul beyond). Everything else (CPU, fp32 / fp16, other
block sizes, K % 64 != 0 for the linear) runs the formulas above in plain torch ops; that path is
the tests' oracle. ``linear_nf4``'s backward is the HIP dequantizer + matmul.

Not served: FSDP2 sharding. split, new_zeros, slice, view, as_strided, cat, pin_memory, the
all-gather / scatter / wait collectives and ``fsdp_pre/post_all_gather`` raise
``NotImplementedError`` naming what is served.
"""

from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn.functional as F

NF4_LEVELS = (
    -1.0, -0.6962, -0.5251, -0.3949, -0.2844, -0.1848, -0.0911, 0.0,
    0.0796, 0.1609, 0.2461, 0.3379, 0.4407, 0.5626, 0.7230, 1.0,
)
DEFAULT_BLOCK_SIZE = 64
DEFAULT_SCALER_BLOCK_SIZE = 256
# values whose 16 differences the plain-torch quantizer forms at a time
_PIECE = 1 << 20

# the stored tensors in the constructor's order, and the stored ints
_TENSOR_FIELDS = ("quantized_scalers", "quantization_factor", "scaler_mean", "quantized_data",
                  "nf4")
_INT_FIELDS = ("block_size", "n_blocks", "scaler_block_size")

_SERVED = ("detach, clone, _to_copy / to(dtype) (dequantize), t, mm, copy_, F.linear, "
           "Tensor.to / .cpu / .cuda")

# aten overload -> handler(op, args, kwargs); torch function -> handler(*args, **kwargs)
_ATEN_HANDLERS = {}
_FUNCTION_HANDLERS = {}


def _on_aten(*overloads):
    def register(handler):
        _ATEN_HANDLERS.update((ov, handler) for ov in overloads)
        return handler

    return register


def _on_function(fn):
    def register(handler):
        _FUNCTION_HANDLERS[fn] = handler
        return handler

    return register


@dataclass(frozen=True)
class SubclassTensorArgs:
    original_shape: torch.Size
    original_strides: Tuple
    storage_offset: int
    dtype: torch.dtype
    device: torch.device
    requires_grad: bool


def _outer_of(t: torch.Tensor, **changes) -> SubclassTensorArgs:
    """The wrapper metadata of ``t``, fields replaced by name."""
    fields = dict(original_shape=t.shape, original_strides=t.stride(),
                  storage_offset=t.storage_offset(), dtype=t.dtype, device=t.device,
                  requires_grad=t.requires_grad)
    fields.update(changes)
    return SubclassTensorArgs(**fields)


def get_block_absmax(input_tensor: torch.Tensor, block_size: int) -> torch.Tensor:
    """max|.| of every ``block_size`` consecutive elements of a flat tensor."""
    if input_tensor.dim() != 1:
        raise AssertionError(f"get_block_absmax takes a flat tensor, got {input_tensor.dim()}-D")
    if input_tensor.numel() % block_size:
        raise AssertionError(f"{input_tensor.numel()} elements are not whole blocks of {block_size}")
    return input_tensor.reshape(-1, block_size).abs().amax(dim=1)


def _require_hip_ops():
    from torchao import ops

    if "nf4_linear" not in ops.native_dispatch_nf4():
        raise RuntimeError(
            "NF4 on a bf16 HIP tensor needs the native op kernels (libtorchao_ops.so), which did "
            f"not load: {ops._native_error}")


def _takes_hip(t: torch.Tensor, block_size: int, scaler_block_size: int) -> bool:
    """bf16 HIP tensors with the default block sizes run csrc/nf4.hip; a missing kernel library
    is an error there, not a reason to run the torch formulation."""
    if not (t.is_cuda and t.dtype is torch.bfloat16 and block_size == DEFAULT_BLOCK_SIZE
            and scaler_block_size == DEFAULT_SCALER_BLOCK_SIZE):
        return False
    _require_hip_ops()
    return True


# ---- the format in plain torch ops ---------------------------------------------------------------
def _double_quantize_absmax(absmax: torch.Tensor, scaler_block_size: int):
    """Second stage of the quantizer on the n_blocks absmaxes (a tensor 64 times smaller than the
    weight): (int8 scalers, per-group factors, mean)."""
    if absmax.numel() % scaler_block_size:
        raise AssertionError(f"{absmax.numel()} block scalers are not whole groups of "
                             f"{scaler_block_size}")
    mean = absmax.mean()
    centred = absmax - mean
    groups = centred.view(-1, scaler_block_size)
    group_absmax = groups.abs().max(dim=1).values
    factor = 256 / (2 * group_absmax)
    if factor.dtype is torch.bfloat16:
        # A group that holds an inf or NaN weight has a NaN factor. Which NaN a bf16 op writes
        # depends on the device and on whether a CPU kernel took its vector path; the stored one is
        # the all-ones pattern the reference's CPU quantizer writes, on every device. The pattern
        # is read off that quantizer's output, not derived from the format. The int8 scalers of
        # such a group are the conversion of NaN to int8, which torch leaves undefined; it gives 0
        # on x86 and on gfx950, and the edge fixture's scalers match only because of that.
        all_ones = torch.full((), -1, dtype=torch.int16, device=factor.device).view(torch.bfloat16)
        factor = torch.where(factor.isnan(), all_ones, factor)
    q = (groups * factor.unsqueeze(-1)).round().clamp(-128, 127)
    return q.flatten().to(torch.int8), factor.contiguous(), mean


def _nearest_codes(scaled: torch.Tensor, nf4: torch.Tensor) -> torch.Tensor:
    """First index of the smallest |v - nf4[j]| for a flat tensor, _PIECE values at a time."""
    out = torch.empty(scaled.numel(), dtype=torch.uint8, device=scaled.device)
    for start in range(0, scaled.numel(), _PIECE):
        piece = scaled[start:start + _PIECE]
        out[start:start + _PIECE] = (
            (piece.unsqueeze(-1) - nf4).abs().min(dim=-1).indices.to(torch.uint8))
    return out


def _quantize_plain(flat: torch.Tensor, block_size: int, scaler_block_size: int,
                    nf4: torch.Tensor):
    """(codes, int8 scalers, factors, mean) of a flat tensor by the module docstring's formulas."""
    absmax = get_block_absmax(flat, block_size)
    scaled = (flat.view(-1, block_size) / absmax.unsqueeze(-1)).flatten()
    codes = _nearest_codes(scaled, nf4)
    packed = (codes[0::2] << 4) | codes[1::2]
    return (packed,) + _double_quantize_absmax(absmax, scaler_block_size)


def _dequantize_plain(t: "NF4Tensor") -> torch.Tensor:
    """w^ of a contiguous NF4Tensor in plain torch ops, on any device: two shifts / masks, two
    gathers, a division, an add, two multiplies, a stack (also what bf16 HIP tensors are measured
    against: experiments/bench_nf4.py)."""
    groups = t.quantized_scalers.view(-1, t.scaler_block_size)
    scalers = (groups / t.quantization_factor.unsqueeze(-1)).flatten().to(t.dtype) + t.scaler_mean
    per_byte = scalers.repeat_interleave(t.block_size // 2)
    even = t.nf4[(t.quantized_data >> 4).long()] * per_byte
    odd = t.nf4[(t.quantized_data & 0xF).long()] * per_byte
    return torch.stack((even, odd), dim=-1).reshape(t.shape)


class NF4Tensor(torch.Tensor):
    """A weight in the QLoRA NF4 format (see the module docstring)."""

    @torch._dynamo.disable
    def __new__(cls, tensor_meta: SubclassTensorArgs, block_size: int, n_blocks: int,
                scaler_block_size: int, quantized_scalers: torch.Tensor,
                quantization_factor: torch.Tensor, scaler_mean: torch.Tensor,
                quantized_data: torch.Tensor, nf4: torch.Tensor):
        return torch.Tensor._make_wrapper_subclass(
            cls, tensor_meta.original_shape, strides=tensor_meta.original_strides,
            storage_offset=tensor_meta.storage_offset, dtype=tensor_meta.dtype,
            device=tensor_meta.device, requires_grad=tensor_meta.requires_grad)

    @torch._dynamo.disable
    def __init__(self, tensor_meta: SubclassTensorArgs, block_size: int, n_blocks: int,
                 scaler_block_size: int, quantized_scalers: torch.Tensor,
                 quantization_factor: torch.Tensor, scaler_mean: torch.Tensor,
                 quantized_data: torch.Tensor, nf4: torch.Tensor):
        stored = (block_size, n_blocks, scaler_block_size, quantized_scalers,
                  quantization_factor, scaler_mean, quantized_data, nf4)
        for name, value in zip(_INT_FIELDS + _TENSOR_FIELDS, stored):
            setattr(self, name, value)

    def _with(self, outer=None, **tensors) -> "NF4Tensor":
        """This tensor with other wrapper metadata and / or other stored tensors."""
        parts = [tensors.get(name, getattr(self, name)) for name in _TENSOR_FIELDS]
        ints = [getattr(self, name) for name in _INT_FIELDS]
        return NF4Tensor(_outer_of(self) if outer is None else outer, *ints, *parts)

    def _map_stored(self, fn) -> "NF4Tensor":
        """fn applied to every stored tensor; the wrapper follows them to their device."""
        moved = {name: fn(getattr(self, name)) for name in _TENSOR_FIELDS}
        return self._with(_outer_of(self, device=moved["quantized_data"].device), **moved)

    # ---- quantize ----------------------------------------------------------------------------
    @classmethod
    @torch.no_grad()
    def from_tensor(cls, input_tensor: torch.Tensor, block_size: int, scaler_block_size: int):
        numel = input_tensor.numel()
        if input_tensor.dim() > 2:
            raise AssertionError(f"NF4 takes 1-D and 2-D tensors, got {input_tensor.dim()}-D")
        if not input_tensor.is_contiguous():
            raise AssertionError("NF4 takes a contiguous tensor")
        for size, what in ((block_size, "block_size"), (scaler_block_size, "scaler_block_size")):
            if numel % size:
                raise AssertionError(f"{numel} elements are not a multiple of {what} = {size}")
        plain = input_tensor.detach()
        if type(plain) is not torch.Tensor:  # a Parameter, or another subclass' data
            plain = plain.as_subclass(torch.Tensor)
        nf4 = torch.tensor(NF4_LEVELS, device=plain.device, dtype=plain.dtype)
        if _takes_hip(plain, block_size, scaler_block_size):
            codes, absmax = torch.ops.torchao.nf4_quantize_blocks(plain, nf4)
            scalers, factor, mean = _double_quantize_absmax(absmax, scaler_block_size)
        else:
            codes, scalers, factor, mean = _quantize_plain(plain.flatten(), block_size,
                                                           scaler_block_size, nf4)
        return cls(_outer_of(input_tensor), block_size, numel // block_size, scaler_block_size,
                   scalers, factor, mean, codes, nf4)

    # ---- dequantize --------------------------------------------------------------------------
    def _hip(self) -> bool:
        """Whether this tensor's dequantize and linear run the HIP kernels."""
        if not (self.quantized_data.is_cuda and self.dtype is torch.bfloat16):
            return False
        return _takes_hip(self.nf4, self.block_size, self.scaler_block_size)

    def _stored(self):
        """The stored tensors in the ops' argument order."""
        return (self.quantized_data, self.quantized_scalers, self.quantization_factor,
                self.scaler_mean, self.nf4)

    def get_original_weight(self) -> torch.Tensor:
        """w^ in the tensor's dtype and shape; of a transposed view (``t()``), the transpose of
        the stored weight's."""
        if not self.is_contiguous():
            if self.dim() != 2 or not self.t().is_contiguous():
                raise AssertionError("an NF4Tensor is contiguous or the transpose of one")
            return self.t().get_original_weight().t()
        if self._hip():
            return torch.ops.torchao.nf4_dequantize(*self._stored(), list(self.shape))
        return _dequantize_plain(self)

    # ---- plumbing ------------------------------------------------------------------------------
    def __repr__(self) -> str:
        return (f"NF4Tensor(shape={tuple(self.shape)}, dtype={self.dtype}, device={self.device}, "
                f"block_size={self.block_size}, scaler_block_size={self.scaler_block_size})")

    __str__ = __repr__

    def __tensor_flatten__(self):
        # the reference's key order and metadata, which its checkpoints and torch.compile see
        names = ["quantized_data", "scaler_mean", "quantization_factor", "quantized_scalers", "nf4"]
        meta = {name: getattr(self, name) for name in _INT_FIELDS}
        meta["tensor_meta"] = _outer_of(self)
        return names, meta

    @staticmethod
    def __tensor_unflatten__(inner_tensors, metadata, outer_size, outer_stride):
        if set(inner_tensors) != set(_TENSOR_FIELDS):
            raise AssertionError(f"NF4Tensor holds {_TENSOR_FIELDS}, got {sorted(inner_tensors)}")
        return NF4Tensor(metadata["tensor_meta"], *(metadata[k] for k in _INT_FIELDS),
                         *(inner_tensors[k] for k in _TENSOR_FIELDS))

    @classmethod
    @torch._dynamo.disable
    def __torch_dispatch__(cls, func, types, args, kwargs=None):
        passing = (torch._subclasses.fake_tensor.FakeTensor,
                   torch._subclasses.functional_tensor.FunctionalTensor)
        for t in types:
            if not (issubclass(cls, t) or any(issubclass(p, t) for p in passing)):
                return NotImplemented  # another subclass in the call: let it handle the op
        handler = _ATEN_HANDLERS.get(func)
        if handler is None:
            raise NotImplementedError(
                f"NF4Tensor does not serve {func} (served: {_SERVED})")
        return handler(func, args, kwargs or {})

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        handler = _FUNCTION_HANDLERS.get(func)
        if handler is not None:
            return handler(*args, **(kwargs or {}))
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **(kwargs or {}))

    def fsdp_pre_all_gather(self, *args, **kwargs):
        raise NotImplementedError(_fsdp_message("fsdp_pre_all_gather"))

    def fsdp_post_all_gather(self, *args, **kwargs):
        raise NotImplementedError(_fsdp_message("fsdp_post_all_gather"))


def _fsdp_message(what: str) -> str:
    return (f"NF4Tensor: {what} belongs to FSDP2 sharding of NF4 weights, which this build does "
            f"not serve (served: {_SERVED})")


def _same_blocking(a, b) -> bool:
    return (isinstance(a, NF4Tensor) and isinstance(b, NF4Tensor)
            and all(getattr(a, k) == getattr(b, k) for k in _INT_FIELDS))


# ---- aten overloads ----------------------------------------------------------------------------
aten = torch.ops.aten


@_on_aten(aten.detach.default)
def _detach(op, args, kwargs):
    # the stored tensors are shared, as a detach of a plain tensor shares its storage
    return args[0]._with(_outer_of(args[0], requires_grad=False))


@_on_aten(aten.clone.default)
def _clone(op, args, kwargs):
    return args[0]._map_stored(torch.clone)


@_on_aten(aten._to_copy.default)
def _to_copy(op, args, kwargs):
    src = args[0]
    out = src.get_original_weight().to(kwargs.get("dtype") or src.dtype)
    device = kwargs.get("device")
    return out if device is None else out.to(device)


@_on_aten(aten.to.dtype)
def _to_dtype(op, args, kwargs):
    return args[0].get_original_weight().to(args[1])


@_on_aten(aten.t.default)
def _transpose(op, args, kwargs):
    a = args[0]
    if a.dim() != 2:
        raise AssertionError(f"NF4Tensor.t() takes a 2-D tensor, got {a.dim()}-D")
    rows, cols = a.shape
    return a._with(_outer_of(a, original_shape=torch.Size((cols, rows)),
                             original_strides=a.stride()[::-1]))


@_on_aten(aten.mm.default)
def _mm(op, args, kwargs):
    x, w = args
    if isinstance(x, NF4Tensor) or not isinstance(w, NF4Tensor):
        raise NotImplementedError(
            f"NF4Tensor: mm is served for (plain, NF4Tensor) only (served: {_SERVED})")
    if w.is_contiguous():
        return x @ w.get_original_weight().to(x.dtype)
    return linear_nf4(x, w.t())  # x @ W^T with W stored row-major: the linear


@_on_aten(aten.copy_.default)
def _copy_(op, args, kwargs):
    dst, src = args[0], args[1]
    if src.shape != dst.shape:
        raise RuntimeError(f"NF4Tensor.copy_: source shape {tuple(src.shape)} is not the "
                           f"target's {tuple(dst.shape)}")
    if not _same_blocking(dst, src):
        # a plain tensor, or an NF4Tensor of other block sizes, is quantized to the target's
        plain = src.get_original_weight() if isinstance(src, NF4Tensor) else src
        src = NF4Tensor.from_tensor(plain.to(dst.device).contiguous(), dst.block_size,
                                    dst.scaler_block_size)
    for name in _TENSOR_FIELDS:
        getattr(dst, name).copy_(getattr(src, name))
    return dst


def _refuse(name):
    def handler(op, args, kwargs):
        raise NotImplementedError(_fsdp_message(name))

    return handler


def _register_fsdp_refusals():
    refused = {
        "split": (aten.split.Tensor, aten.split_with_sizes.default),
        "new_zeros": (aten.new_zeros.default, aten.empty_like.default),
        "slice": (aten.slice.Tensor,),
        "view": (aten.view.default,),
        "as_strided": (aten.as_strided.default,),
        "cat": (aten.cat.default,),
        "pin_memory": (aten._pin_memory.default, aten.is_pinned.default),
    }
    for name, overloads in refused.items():
        _on_aten(*overloads)(_refuse(name))
    for ns, packet in (("_c10d_functional", "all_gather_into_tensor"),
                       ("_c10d_functional", "wait_tensor"),
                       ("c10d_functional", "all_gather_into_tensor"),
                       ("c10d_functional", "wait_tensor"), ("c10d", "scatter_")):
        try:
            overload = getattr(getattr(torch.ops, ns), packet).default
        except (AttributeError, RuntimeError):  # a build without distributed
            continue
        _on_aten(overload)(_refuse(f"{ns}.{packet}"))


_register_fsdp_refusals()


# ---- linear --------------------------------------------------------------------------------------
def _hip_linear_ok(x: torch.Tensor, weight: NF4Tensor) -> bool:
    return (isinstance(weight, NF4Tensor) and weight.dim() == 2 and weight.is_contiguous()
            and x.is_cuda and x.dtype is torch.bfloat16 and weight.dtype is torch.bfloat16
            and x.dim() >= 1 and weight.size(1) % DEFAULT_BLOCK_SIZE == 0
            and x.device == weight.quantized_data.device and weight._hip())


def _nf4_linear_forward(x: torch.Tensor, weight: NF4Tensor, bias=None) -> torch.Tensor:
    if _hip_linear_ok(x, weight):
        return torch.ops.torchao.nf4_linear(x, *weight._stored(), weight.size(0), bias)
    out = F.linear(x, weight.get_original_weight().to(x.dtype))
    return out if bias is None else out + bias


class LinearNF4(torch.autograd.Function):
    """y = x @ w^.T; the weight never has a gradient, grad_x = grad_y @ w^."""

    @staticmethod
    def forward(ctx, input: torch.Tensor, weight: NF4Tensor):
        ctx.nf4_weight = weight
        return _nf4_linear_forward(input, weight)

    @staticmethod
    def backward(ctx, grad_output):
        w_hat = ctx.nf4_weight.get_original_weight()
        return grad_output @ w_hat.to(grad_output.dtype), None


def linear_nf4(input: torch.Tensor, weight: NF4Tensor) -> torch.Tensor:
    """``input @ w^.T`` with an NF4 weight; differentiable in ``input``."""
    return LinearNF4.apply(input, weight)


def to_nf4(tensor, block_size: int = DEFAULT_BLOCK_SIZE,
           scaler_block_size: int = DEFAULT_SCALER_BLOCK_SIZE):
    """Quantize a 1-D or 2-D tensor to NF4."""
    return NF4Tensor.from_tensor(tensor, block_size, scaler_block_size)


# ---- torch-function overrides ----------------------------------------------------------------
def _to_request(args, kwargs):
    """(device, dtype, non_blocking) asked of Tensor.to(*args, **kwargs); None where not given."""
    device, dtype = kwargs.get("device"), kwargs.get("dtype")
    non_blocking = bool(kwargs.get("non_blocking", False))
    other = kwargs.get("other")
    flags = []
    for a in args:
        if isinstance(a, torch.dtype):
            dtype = a
        elif isinstance(a, torch.Tensor):
            other = a
        elif isinstance(a, bool):
            flags.append(a)
        elif isinstance(a, (str, torch.device, int)):
            device = a
    if other is not None:
        device, dtype = other.device, other.dtype
    if flags:
        non_blocking = flags[0]
    return (None if device is None else torch.device(device)), dtype, non_blocking


@_on_function(torch.Tensor.to)
def _tensor_to(self, *args, **kwargs):
    device, dtype, non_blocking = _to_request(args, kwargs)
    if dtype is not None:  # asking for a dtype dequantizes
        return self.get_original_weight().to(device=device or self.device, dtype=dtype,
                                             non_blocking=non_blocking)
    if device is None:
        return self
    return self._map_stored(lambda t: t.to(device, non_blocking=non_blocking))


@_on_function(torch.Tensor.cpu)
def _tensor_cpu(self, *args, **kwargs):
    return self._map_stored(lambda t: t.cpu())


@_on_function(torch.Tensor.cuda)
def _tensor_cuda(self, *args, **kwargs):
    return self._map_stored(lambda t: t.cuda(*args, **kwargs))


@_on_function(F.linear)
def _functional_linear(input, weight, bias=None):
    if not isinstance(weight, NF4Tensor):  # an NF4Tensor as input or bias is not a linear we serve
        with torch._C.DisableTorchFunctionSubclass():
            return F.linear(input, weight, bias)
    needs_grad = torch.is_grad_enabled() and (
        input.requires_grad or (bias is not None and bias.requires_grad))
    if bias is not None and not needs_grad and _hip_linear_ok(input, weight):
        # inference: the bias' second rounding inside the launch
        return _nf4_linear_forward(input, weight, bias)
    out = LinearNF4.apply(input, weight)
    return out if bias is None else out + bias


@torch._dynamo.allow_in_graph
def nf4_constructor(tensor_meta: SubclassTensorArgs, block_size: int, n_blocks: int,
                    scaler_block_size: int, quantized_scalers: torch.Tensor,
                    quantization_factor: torch.Tensor, scaler_mean: torch.Tensor,
                    quantized_data: torch.Tensor, nf4: torch.Tensor):
    """NF4Tensor from its parts (a function torch.compile may keep in a graph)."""
    return NF4Tensor(tensor_meta=tensor_meta, block_size=block_size, n_blocks=n_blocks,
                     scaler_block_size=scaler_block_size, quantized_scalers=quantized_scalers,
                     quantization_factor=quantization_factor, scaler_mean=scaler_mean,
                     quantized_data=quantized_data, nf4=nf4)


torch.serialization.add_safe_globals([NF4Tensor])
