"""Python wrappers of the MoE expert kernels on 3-D int4 weights, shared by the decode harness
(torchao/_models/llama/kernels.py) and the MoE module (torchao/prototype/moe_quant): the
one-token grouped GEMV (csrc/int4_gemv.hip) and the many-token route / grouped GEMM / combine
(csrc/moe_gemm.hip, through the ``torchao::moe_route``, ``int4_grouped_linear`` and
``moe_combine`` ops). Outputs are allocated with torch (graph-capture safe); launches go on
torch's current stream; nothing here synchronises."""

import torch

from torchao import _lib


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous CUDA {dtype} tensor, got "
                           f"{t.dtype} on {t.device} (contiguous={t.is_contiguous()})")


def int4_parts(w):
    """(packed [E, N, K/8] int32, scale_and_zero [E, N, K/g, 2] bf16, group size) of a 3-D
    Int4WeightOnlyConfig weight."""
    impl = w.tensor_impl
    return impl.packed_weight, impl.scale_and_zero, w.block_size[-1]


def int4_grouped_decode(x: torch.Tensor, packed: torch.Tensor, scale_and_zero: torch.Tensor,
                        group_size: int, expert_idx: torch.Tensor) -> torch.Tensor:
    """The A = expert_idx.numel() experts' int4 linears of one token in one launch
    (tao_int4wo_grouped_gemv_bf16): packed [E, N, K/8] int32, scale_and_zero [E, N, K/g, 2] bf16
    (a 3-D Int4WeightOnlyConfig weight's tensor_impl), x [K] / [1, K] (shared) or [A, K] (row a
    for expert a) bf16 -> y [A, N] bf16, row a bit-identical to expert expert_idx[a]'s linear."""
    _check(x, torch.bfloat16, "int4_grouped x")
    _check(expert_idx, torch.int64, "int4_grouped expert_idx")
    if packed.dim() != 3:
        raise RuntimeError(f"int4_grouped: packed must be [E, N, K/8], got {tuple(packed.shape)}")
    E, N, K8 = packed.shape
    K, A = K8 * 8, expert_idx.numel()
    rows = x.numel() // K
    if x.shape[-1] != K or rows not in (1, A):
        raise RuntimeError(f"int4_grouped: x {tuple(x.shape)} must be [K] or [A, K] with K = {K}")
    y = torch.empty(A, N, dtype=x.dtype, device=x.device)
    _lib.call("tao_int4wo_grouped_gemv_bf16", x.data_ptr(), rows, packed.data_ptr(),
              scale_and_zero.data_ptr(), expert_idx.data_ptr(), A, E, N, K, int(group_size),
              y.data_ptr(), _stream(x))
    return y


def int4_moe_ffn_one_token(x: torch.Tensor, w1, w2, w3, expert_indices: torch.Tensor,
                           expert_weights: torch.Tensor) -> torch.Tensor:
    """The one-token branch of the reference's ConditionalFeedForwardAOQuantizable on 3-D int4
    weights (AffineQuantizedTensor [E, I, D] / [E, D, I] / [E, I, D]): three grouped launches
    instead of 3 A per-expert linears, the same bf16 ops in between (silu(w1 x) * w3 x, then w2,
    then the expert-weighted sum) -> [D]; the callers give it their own shape."""
    idx = expert_indices.reshape(-1)
    y1 = torch.nn.functional.silu(int4_grouped_decode(x, *int4_parts(w1), idx))
    y3 = int4_grouped_decode(x, *int4_parts(w3), idx)
    y2 = int4_grouped_decode((y1 * y3).contiguous(), *int4_parts(w2), idx)  # [A, D]
    return (y2 * expert_weights.view(-1, 1)).sum(dim=0)


def moe_dual(R: int, E: int) -> bool:
    """Whether the many-token expert FFN runs gate and up in one launch (csrc/moe_host.h, under the
    calling thread's ``tuning(moe=...)``)."""
    return bool(_lib.lib().tao_moe_dual(R, E))


def int4_moe_ffn_grouped(x: torch.Tensor, w1, w2, w3, expert_indices: torch.Tensor,
                         expert_weights: torch.Tensor, top_k: int) -> torch.Tensor:
    """The many-token branch on 3-D int4 weights: x [T, D] bf16, expert_indices / expert_weights
    [T, A] -> [T, D]. Route (stable sort of the T A activations by expert), gate-up (one launch
    with SwiGLU in the epilogue, or two and torch's silu and mul), down, combine: four or five
    launches, no host sync, deterministic."""
    ops = torch.ops.torchao
    _check(x, torch.bfloat16, "int4_moe_ffn x")
    p1, s1, g = int4_parts(w1)
    p3, s3, g3 = int4_parts(w3)
    p2, s2, g2 = int4_parts(w2)
    E = p1.shape[0]
    if g3 != g or p3.shape != p1.shape:
        raise RuntimeError("int4_moe_ffn: w1 and w3 must share their shape and group size")
    offsets, order, inverse = ops.moe_route(expert_indices, E, top_k)
    if moe_dual(order.numel(), E):
        h = ops.int4_grouped_linear(x, order, top_k, p1, s1, p3, s3, offsets, g)
    else:
        y1 = torch.nn.functional.silu(
            ops.int4_grouped_linear(x, order, top_k, p1, s1, None, None, offsets, g))
        h = y1 * ops.int4_grouped_linear(x, order, top_k, p3, s3, None, None, offsets, g)
    y2 = ops.int4_grouped_linear(h, None, 1, p2, s2, None, None, offsets, g2)
    w = expert_weights.reshape(-1)
    if w.dtype != torch.bfloat16:
        raise RuntimeError(f"int4_moe_ffn: expert_weights must be bf16, got {w.dtype}")
    return ops.moe_combine(y2, w, inverse, top_k)
