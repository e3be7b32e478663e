"""The quantizable MoE feed-forward (reference
torchao/prototype/moe_quant/quantizable_moe_modules.py), with the reference's attribute names
(``router``, ``experts``, ``w1`` / ``w2`` / ``w3``) so that its checkpoints and filters apply.

``ConditionalFeedForwardAOQuantizable.forward`` picks one of three paths:

* 3-D int4 ``AffineQuantizedTensor`` weights on the GPU, bf16 activations, ``act_fn is F.silu``:
  one token runs the grouped GEMV (three launches), more tokens run route, grouped gate-up, grouped
  down and combine (csrc/moe_gemm.hip; four or five launches, no host sync, deterministic);
* anything else (plain weights, CPU tensors, int8 / float8 weights, another ``act_fn``): the
  reference's op sequence in plain torch, one ``F.linear`` per expert, which the quantized weights
  serve through their own linear dispatch. Its one-token and many-token branches stay separate:
  their reductions round differently. On the CPU, where this tree has no quantized linear kernels,
  a quantized expert weight is dequantized first (``F.linear(x, w.dequantize())``, the formula of
  the reference's dispatch when no kernel takes a weight); on the GPU a weight without a kernel
  raises, as every linear here does.
"""

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from torchao.dtypes import AffineQuantizedTensor, TensorCoreTiledLayout
from torchao.kernel.moe import int4_moe_ffn_grouped, int4_moe_ffn_one_token

__all__ = ["MOEFeedForwardAOQuantizable", "ConditionalFeedForwardAOQuantizable"]


class MOEFeedForwardAOQuantizable(nn.Module):
    def __init__(self, hidden_dim, expert_dim, num_experts, top_k, act_fn=F.silu,
                 shared_expert=None, return_scores=False, empty_init=True) -> None:
        super().__init__()
        self.router = nn.Linear(hidden_dim, num_experts, bias=False)
        self.experts = ConditionalFeedForwardAOQuantizable(
            num_experts, hidden_dim, expert_dim, act_fn, empty_init)
        self.hidden_dim = hidden_dim
        self.top_k = top_k
        self.shared_expert = shared_expert
        self.return_scores = return_scores

    def forward(self, x: Tensor) -> Tensor:
        batch_size = x.shape[0]
        x = x.view(-1, self.hidden_dim)  # [T, D]
        scores = F.softmax(self.router(x), dim=-1)  # [T, E]
        scores, expert_indices = torch.topk(scores, self.top_k, dim=-1)  # [T, A] each
        scores /= scores.sum(dim=-1, keepdim=True).to(x.dtype)
        out = self.experts(x, expert_indices, scores, self.top_k)
        if self.shared_expert:
            out += self.shared_expert(x)
        out = out.reshape(batch_size, -1, self.hidden_dim)
        return (out, scores) if self.return_scores else out


def _is_int4_stack(w) -> bool:
    return (isinstance(w, AffineQuantizedTensor) and w.dim() == 3
            and isinstance(w._layout, TensorCoreTiledLayout))


class ConditionalFeedForwardAOQuantizable(nn.Module):
    def __init__(self, num_experts, hidden_dim, expert_dim, act_fn, empty_init=True):
        super().__init__()
        make = torch.empty if empty_init else torch.randn
        self.w1 = nn.Parameter(make(num_experts, expert_dim, hidden_dim))  # E, I, D
        self.w2 = nn.Parameter(make(num_experts, hidden_dim, expert_dim))  # E, D, I
        self.w3 = nn.Parameter(make(num_experts, expert_dim, hidden_dim))  # E, I, D
        self.num_experts = num_experts
        self.act_fn = act_fn
        self.hidden_dim = hidden_dim
        self.expert_dim = expert_dim

    def _takes_grouped_kernels(self, x: Tensor) -> bool:
        return (x.is_cuda and x.dtype is torch.bfloat16 and self.act_fn is F.silu
                and _is_int4_stack(self.w1) and _is_int4_stack(self.w2)
                and _is_int4_stack(self.w3))

    def forward(self, x: Tensor, expert_indices: Tensor, expert_weights: Tensor,
                top_k: int) -> Tensor:
        num_tokens = x.shape[0]
        if self._takes_grouped_kernels(x):
            x = x.contiguous()
            if num_tokens == 1:
                return int4_moe_ffn_one_token(x, self.w1, self.w2, self.w3, expert_indices,
                                              expert_weights).reshape(x.shape)
            return int4_moe_ffn_grouped(x, self.w1, self.w2, self.w3, expert_indices,
                                        expert_weights, top_k)
        if num_tokens == 1:
            return self._one_token(x, expert_indices, expert_weights, top_k)
        return self._many_tokens(x, expert_indices, expert_weights, top_k)

    def _expert(self, x: Tensor, w1, w2, w3) -> Tensor:
        if not x.is_cuda:
            w1, w2, w3 = (w.dequantize() if isinstance(w, AffineQuantizedTensor) else w
                          for w in (w1, w2, w3))
        return F.linear(self.act_fn(F.linear(x, w1)) * F.linear(x, w3), w2)

    def _one_token(self, x, expert_indices, expert_weights, top_k):
        idx = expert_indices.view(top_k)
        w1, w2, w3 = self.w1[idx], self.w2[idx], self.w3[idx]
        outs = [self._expert(x, w1[i], w2[i], w3[i]) for i in range(top_k)]
        return (torch.cat(outs, dim=0) * expert_weights.view(-1, 1)).sum(dim=0).reshape(x.shape)

    def _many_tokens(self, x, expert_indices, expert_weights, top_k):
        flat = expert_indices.reshape(-1)
        order = flat.argsort(stable=True)  # [T A] activations grouped by expert
        token_of = order.div(top_k).floor().to(torch.int64)
        ends = torch.bincount(flat, minlength=self.num_experts).cumsum(0).tolist()  # host sync
        outs, start = [], 0
        for e in range(self.num_experts):
            cur_x = x[token_of[start:ends[e]]]
            outs.append(self._expert(cur_x, self.w1[e], self.w2[e], self.w3[e]))
            start = ends[e]
        weighted = torch.cat(outs, dim=0) * expert_weights.reshape(-1, 1)[order].view(-1, 1)
        index = token_of.unsqueeze(-1).expand(flat.numel(), self.hidden_dim)
        return torch.zeros_like(x).scatter_add(dim=0, index=index, src=weighted)
