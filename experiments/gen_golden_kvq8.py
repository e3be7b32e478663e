"""Generate tests/golden/kvq8_N128.npz by running the REFERENCE torchao on the CPU.

Run where the reference checkout is available, with it first on the import path (it is not
needed, and not present, where the tests run):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python3 experiments/gen_golden_kvq8.py

It calls the reference's own ``_quantize_activation_per_token_absmax``, its
``AffineQuantizedKVCache`` and its llama ``Transformer`` and records inputs and outputs as data;
bf16 tensors are stored as their uint16 bit patterns. Nothing of the reference's source is stored.

  rows, row_names   bf16 bits [R, 128] and what each row is there for: random rows, an all-zero
                    row, a row of bf16 subnormals, a row whose largest value is negative, a row
                    with one outlier of 200, rows whose amax / 127 falls just below, on and just
                    above a bf16 rounding boundary, a row whose scaled values land on .5
  row_q, row_s      the reference's int8 codes [R, 128] and scale bits [R]
  A reference AffineQuantizedKVCache(1, 16, 2, 128) (batch 1, 16 positions, 2 heads), one update
  of 5 positions then three of 1 position:
  upd{i}_pos, upd{i}_k, upd{i}_v        the call's positions and bf16 bits of k_val / v_val
  upd{i}_kc, upd{i}_vc                  int8 caches after the call
  upd{i}_ks, upd{i}_vs                  scale bits after the call
  upd{i}_kout, upd{i}_vout              bits of the returned k_out / v_out
  A stories15M run in bf16 on the CPU (weights from ``model_weights(seed)`` below, prompt
  ``sd_prompt``, prefill then ``SD_STEPS`` greedy one-token steps), unquantized and with
  kv_cache_quantization:
  sd_seed, sd_prompt, sd_steps
  sd_sqnr_db        20 log10(|l| / |l - l_q|) over the logits of all decode steps, the reference's
                    own figure for what the int8 cache costs on this input
"""

import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "kvq8_N128.npz")
D = 128
SD_SEED, SD_PROMPT_LEN, SD_STEPS = 5, 12, 6


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def edge_rows():
    g = torch.Generator().manual_seed(21)
    names, rows = [], []

    def add(name, row):
        names.append(name)
        rows.append(row.to(torch.bfloat16))

    for i in range(3):
        add(f"random{i}", torch.randn(D, generator=g) * (0.3 * 4 ** i))
    add("zero", torch.zeros(D))
    add("subnormal", from_bits(np.arange(1, D + 1) * 2).float())
    add("negative_amax", -torch.rand(D, generator=g) - 0.25)
    r = torch.randn(D, generator=g)
    r[17] = 200.0
    add("outlier200", r)
    # amax / 127 beside a bf16 rounding boundary: of the bf16 amaxes in [0.5, 2), the two whose
    # fp32 quotient lies closest below and closest above the midpoint of two bf16 numbers (one
    # rounds down, the other up), and 127 * 2^-7, whose quotient is a bf16 number exactly
    cands = from_bits(np.arange(0x3F00, 0x4000)).float()
    frac = ((cands / 127.0).view(torch.int32) & 0xFFFF).float() / 65536.0
    below = cands[torch.where(frac < 0.5, frac, -1.0).argmax()]
    above = cands[torch.where(frac > 0.5, frac, 2.0).argmin()]
    for name, amax in (("boundary_below", float(below)), ("boundary_above", float(above)),
                       ("boundary_exact", 0.9921875)):
        r = torch.rand(D, generator=g) * 0.9 - 0.45
        r[3] = -amax
        add(name, r)
    # amax 127 -> s = 1, r = 1: x.5 stays x.5 after scaling (round half to even both ways)
    r = torch.arange(D, dtype=torch.float32) % 64 + 0.5
    r[1::2] *= -1
    r[0] = 127.0
    add("halves", r)
    return names, torch.stack(rows)


def model_weights(state, seed):
    """Deterministic weights by parameter name (module order differs between the two packages):
    linears U(-1/sqrt(K), 1/sqrt(K)), embeddings N(0, 0.02), norms 1, in bf16."""
    out = {}
    for i, name in enumerate(sorted(state)):
        shape = state[name].shape
        g = torch.Generator().manual_seed(seed * 1000 + i)
        if "norm" in name:
            w = torch.ones(shape)
        elif "tok_embeddings" in name:
            w = torch.randn(shape, generator=g) * 0.02
        else:
            bound = 1.0 / math.sqrt(shape[-1])
            w = (torch.rand(shape, generator=g) * 2 - 1) * bound
        out[name] = w.to(torch.bfloat16)
    return out


def sqnr_db(ref, x):
    return float(20 * torch.log10(ref.norm() / (ref - x).norm()))


@torch.no_grad()
def decode_logits(model, prompt, steps):
    """fp32 logits [steps, vocab] of `steps` greedy one-token steps after the prompt's prefill."""
    P = prompt.shape[1]
    logits = model(prompt, torch.arange(P))
    tok = logits[:, -1].argmax(-1, keepdim=True)
    out = []
    for i in range(steps):
        logits = model(tok, torch.tensor([P + i]))
        out.append(logits[0, -1].float())
        tok = logits[:, -1].argmax(-1, keepdim=True)
    return torch.stack(out)


def main():
    import torchao  # the reference

    assert not os.path.realpath(torchao.__file__).startswith(ROOT), (
        f"{torchao.__file__} is this repository's package; put the reference checkout first on "
        "PYTHONPATH"
    )
    from torchao._models.llama.model import AffineQuantizedKVCache, Transformer
    from torchao.quantization.utils import _quantize_activation_per_token_absmax

    rec = {}
    names, rows = edge_rows()
    q, s = _quantize_activation_per_token_absmax(rows)
    assert q.dtype == torch.int8 and s.dtype == torch.bfloat16 and s.numel() == rows.shape[0]
    rec.update(rows=bf16_bits(rows), row_names=np.array(names), row_q=q.numpy(),
               row_s=bf16_bits(s.reshape(-1)))
    for n, sc, qq in zip(names, s.reshape(-1).tolist(), q.tolist()):
        print(f"{n:14s} scale {sc:.6g} codes {min(qq)}..{max(qq)}")

    cache = AffineQuantizedKVCache(1, 16, 2, D)
    g = torch.Generator().manual_seed(22)
    calls = [torch.tensor([0, 1, 2, 3, 4]), torch.tensor([5]), torch.tensor([6]),
             torch.tensor([9])]
    for i, pos in enumerate(calls):
        k = (torch.randn(1, 2, len(pos), D, generator=g) * 1.5).to(torch.bfloat16)
        v = torch.randn(1, 2, len(pos), D, generator=g).to(torch.bfloat16)
        k_out, v_out = cache.update(pos, k, v)
        assert k_out.dtype == torch.bfloat16 and k_out.shape == (1, 2, 16, D)
        rec.update({f"upd{i}_pos": pos.numpy(), f"upd{i}_k": bf16_bits(k),
                    f"upd{i}_v": bf16_bits(v), f"upd{i}_kc": cache.k_cache.numpy().copy(),
                    f"upd{i}_vc": cache.v_cache.numpy().copy(),
                    f"upd{i}_ks": bf16_bits(cache.k_cache_scale).copy(),
                    f"upd{i}_vs": bf16_bits(cache.v_cache_scale).copy(),
                    f"upd{i}_kout": bf16_bits(k_out), f"upd{i}_vout": bf16_bits(v_out)})

    gp = torch.Generator().manual_seed(SD_SEED + 1)
    logits = {}
    for quant in (False, True):
        model = Transformer.from_name("stories15M").to(torch.bfloat16).eval()
        model.load_state_dict(model_weights(model.state_dict(), SD_SEED))
        if quant == 0:
            prompt = torch.randint(0, model.config.vocab_size, (1, SD_PROMPT_LEN), generator=gp)
        with torch.device("cpu"):
            model.setup_caches(1, SD_PROMPT_LEN + SD_STEPS + 1, kv_cache_quantization=quant)
        logits[quant] = decode_logits(model, prompt, SD_STEPS)
    fig = sqnr_db(logits[False], logits[True])
    print("stories15M: reference SQNR of the int8 KV cache over", SD_STEPS, "decode steps:",
          round(fig, 2), "dB")
    rec.update(sd_seed=SD_SEED, sd_prompt=prompt.numpy(), sd_steps=SD_STEPS, sd_sqnr_db=fig)

    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
