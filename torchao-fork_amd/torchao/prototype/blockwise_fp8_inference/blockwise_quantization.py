"""Blockwise float8 quantization (the DeepSeek-V3 recipe): e4m3fn codes, one fp32 scale per 1 x 128
block of an activation and per 128 x 128 block of a weight.

The four functions keep the names and signatures of the reference's Triton module
(torchao/prototype/blockwise_fp8_inference/blockwise_quantization.py). On HIP tensors they call
the ``torch.ops.torchao.blockfp8_*`` ops (csrc/block_fp8.hip); on CPU tensors they run the same
arithmetic in plain torch, which is the oracle of the tests and lets a checkpoint be prepared
offline. The arithmetic, per block, from float32(x):

    amax = max |x|, a NaN element ignored; 0 if the block holds no number
    s    = amax / 448                      (fp32, a subnormal quotient kept)
    code = e4m3fn_rne(x / s)               (fp32 division, no clamp; NaN stays NaN)
           e4m3fn_rne(x) where amax == 0   (the reference computes 0 / 0 and stores NaN codes)

    y[m, n] = bf16( sum_b P[m, n, b] * (xs[m, b] * ws[n // 128, b]) )      fp32, one rounding

Served: ``block_size`` 128 and ``torch.float8_e4m3fn`` only; K a multiple of 128, any N (the
reference's weight quantizer needs N % 128 == 0 as well). The product is bf16 always (the
reference returns ``torch.get_default_dtype()``).
"""

from typing import Optional, Tuple

import torch

BLOCK = 128
_E4M3_MAX = 448.0


def _check_served(block_size: int, dtype: torch.dtype = torch.float8_e4m3fn) -> None:
    if block_size != BLOCK:
        raise NotImplementedError(
            f"blockwise float8: block_size {block_size} is not served (128 only)")
    if dtype is not torch.float8_e4m3fn:
        raise NotImplementedError(
            f"blockwise float8: dtype {dtype} is not served (torch.float8_e4m3fn only)")


def _check_k(K: int) -> None:
    if K % BLOCK != 0:
        raise ValueError(f"blockwise float8: K ({K}) must be a multiple of {BLOCK}")


def _quant_blocks(xb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """xb fp32 [..., E], one block per row of the last dimension -> (codes [..., E], s [...])."""
    a = xb.abs()
    amax = torch.where(a.isnan(), torch.zeros_like(a), a).amax(-1, keepdim=True)
    s = amax / torch.tensor(_E4M3_MAX, dtype=torch.float32)
    v = torch.where(amax == 0, xb, xb / s)
    return v.to(torch.float8_e4m3fn), s.squeeze(-1)


def fp8_blockwise_act_quant(
    x: torch.Tensor, block_size: int = 128, dtype: torch.dtype = torch.float8_e4m3fn
) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] -> (e4m3fn codes [..., K], fp32 scales [..., K/128]), one scale per 128
    consecutive elements of the last dimension. bf16 on a HIP device; any float dtype on the CPU."""
    _check_served(block_size, dtype)
    K = x.size(-1)
    _check_k(K)
    if x.is_cuda:
        return torch.ops.torchao.blockfp8_quantize_act(x)
    q, s = _quant_blocks(x.float().reshape(*x.shape[:-1], K // BLOCK, BLOCK))
    return q.reshape(x.shape), s.contiguous()


def fp8_blockwise_weight_quant(
    x: torch.Tensor, block_size: int = 128, dtype=torch.float8_e4m3fn
) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] -> (e4m3fn codes [N, K], fp32 scales [ceil(N/128), K/128]), one scale per block of
    up to 128 rows x 128 columns (a ragged last row block takes its amax over the rows it has)."""
    _check_served(block_size, dtype)
    if x.dim() != 2:
        raise ValueError("blockwise float8: the weight must have 2 dimensions")
    N, K = x.shape
    _check_k(K)
    if x.is_cuda:
        return torch.ops.torchao.blockfp8_quantize_weight(x)
    NB, KB = (N + BLOCK - 1) // BLOCK, K // BLOCK
    xf = torch.zeros(NB * BLOCK, K, dtype=torch.float32)
    xf[:N] = x.float()
    xb = xf.reshape(NB, BLOCK, KB, BLOCK).permute(0, 2, 1, 3).reshape(NB, KB, BLOCK * BLOCK)
    q, s = _quant_blocks(xb)
    q = q.view(torch.uint8).reshape(NB, KB, BLOCK, BLOCK).permute(0, 2, 1, 3).reshape(-1, K)[:N]
    return q.contiguous().view(torch.float8_e4m3fn), s.contiguous()


def _weight_scale_rows(s: torch.Tensor, N: int) -> torch.Tensor:
    """[NB, K/128] -> [N, K/128]: the scale row of each weight row."""
    return s.repeat_interleave(BLOCK, 0)[:N]


def _check_weight(x: torch.Tensor, s: torch.Tensor) -> None:
    if x.dim() != 2 or s.dim() != 2:
        raise ValueError("blockwise float8: weight and scale must have 2 dimensions")
    N, K = x.shape
    _check_k(K)
    if tuple(s.shape) != ((N + BLOCK - 1) // BLOCK, K // BLOCK):
        raise ValueError(f"blockwise float8: scale must be [ceil(N/128), K/128] = "
                         f"[{(N + BLOCK - 1) // BLOCK}, {K // BLOCK}], got {tuple(s.shape)}")


def fp8_blockwise_weight_dequant(
    x: torch.Tensor, s: torch.Tensor, block_size: int = 128
) -> torch.Tensor:
    """float(code) * scale in fp32, returned in ``torch.get_default_dtype()`` as the reference
    does (float32, or bfloat16 rounded once)."""
    _check_served(block_size)
    _check_weight(x, s)
    out = torch.get_default_dtype()
    if out not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"blockwise float8: dequantization to {out} is not served "
                                  f"(float32 and bfloat16 only)")
    if x.is_cuda:
        return torch.ops.torchao.blockfp8_dequantize_weight(x, s, out is torch.bfloat16)
    N, K = x.shape
    y = x.float() * _weight_scale_rows(s, N).repeat_interleave(BLOCK, 1)
    return y.to(out)


def _blockwise_mm_cpu(a, a_s, b, b_s, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The product of the module docstring in plain torch: fp32 block dot products, the rounded
    fp32 factor xs * ws per block, an fp32 sum over blocks, the bias, one rounding to bf16."""
    N, K = b.shape
    KB = K // BLOCK
    af = a.float().reshape(-1, KB, BLOCK)
    bf = b.float().reshape(N, KB, BLOCK)
    P = torch.einsum("mbk,nbk->mnb", af, bf)
    f = a_s.reshape(-1, 1, KB).float() * _weight_scale_rows(b_s, N).reshape(1, N, KB)
    y = (P * f).sum(-1)
    if bias is not None:
        y = y + bias.float()
    return y.to(torch.bfloat16).reshape(*a.shape[:-1], N)


def blockwise_fp8_gemm(
    a: torch.Tensor,
    a_s: torch.Tensor,
    b: torch.Tensor,
    b_s: torch.Tensor,
    block_size: int = 128,
) -> torch.Tensor:
    """a [..., K] codes with a_s [..., K/128], b [N, K] codes with b_s [ceil(N/128), K/128] ->
    bf16 [..., N]."""
    _check_served(block_size)
    _check_weight(b, b_s)
    if a.size(-1) != b.size(1):
        raise ValueError(f"blockwise float8: a last dim {a.size(-1)} != K {b.size(1)}")
    if a.is_cuda:
        return torch.ops.torchao.blockfp8_scaled_mm(a, a_s, b, b_s, None)
    return _blockwise_mm_cpu(a, a_s, b, b_s)
