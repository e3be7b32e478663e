"""Int8 KV cache on the CPU: the per-row quantizer and AffineQuantizedKVCache against the
reference's recorded results (tests/golden/kvq8_N128.npz, experiments/gen_golden_kvq8.py),
Transformer.setup_caches(kv_cache_quantization=...), a stories15M decode against the reference's own
figure for what the int8 cache costs, and the argument checks of the two C entries."""

import math
import os

import numpy as np
import pytest
import torch

from torchao._models.llama.model import AffineQuantizedKVCache, KVCache, ModelArgs, Transformer
from torchao.quantization.utils import _quantize_activation_per_token_absmax

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kvq8_N128.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def from_bits(v) -> torch.Tensor:
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def test_quantizer_matches_reference_rows(gold):
    rows = from_bits(gold["rows"])
    names = [str(n) for n in gold["row_names"]]
    for must in ("zero", "subnormal", "negative_amax", "outlier200", "boundary_below",
                 "boundary_above", "halves"):
        assert must in names
    q, s = _quantize_activation_per_token_absmax(rows)
    assert q.dtype == torch.int8 and s.dtype == torch.bfloat16 and s.shape == rows.shape[:-1]
    for i, name in enumerate(names):
        assert bits(s)[i] == gold["row_s"][i], name
        np.testing.assert_array_equal(q[i].numpy(), gold["row_q"][i], err_msg=name)
    # a leading batch shape, and the rows one at a time, change nothing
    q3, s3 = _quantize_activation_per_token_absmax(rows.reshape(1, -1, 1, rows.shape[-1]))
    assert torch.equal(q3.reshape(q.shape), q) and torch.equal(s3.reshape(s.shape), s)
    # scale dtype: the input's, fp32 for fp16 (reference utils.py:165)
    assert _quantize_activation_per_token_absmax(rows.float())[1].dtype == torch.float32
    assert _quantize_activation_per_token_absmax(rows.half())[1].dtype == torch.float32


def test_cache_update_matches_reference_run(gold):
    cache = AffineQuantizedKVCache(1, 16, 2, 128)
    assert set(dict(cache.named_buffers())) == {"k_cache", "v_cache", "k_cache_scale",
                                                "v_cache_scale"}
    assert not cache.state_dict()  # non-persistent, as KVCache
    assert bool((cache.k_cache_scale == 1).all()) and cache.k_cache_scale.shape == (1, 2, 16, 1)
    for i in range(4):
        pos = torch.tensor(gold[f"upd{i}_pos"])
        k_out, v_out = cache.update(pos, from_bits(gold[f"upd{i}_k"]), from_bits(gold[f"upd{i}_v"]))
        assert k_out.dtype == torch.bfloat16 and k_out.shape == (1, 2, 16, 128)
        np.testing.assert_array_equal(cache.k_cache.numpy(), gold[f"upd{i}_kc"])
        np.testing.assert_array_equal(cache.v_cache.numpy(), gold[f"upd{i}_vc"])
        np.testing.assert_array_equal(bits(cache.k_cache_scale), gold[f"upd{i}_ks"])
        np.testing.assert_array_equal(bits(cache.v_cache_scale), gold[f"upd{i}_vs"])
        np.testing.assert_array_equal(bits(k_out), gold[f"upd{i}_kout"])
        np.testing.assert_array_equal(bits(v_out), gold[f"upd{i}_vout"])
        # the rows just written come back exact
        assert torch.equal(k_out[:, :, pos], from_bits(gold[f"upd{i}_k"]))


def test_from_float_shapes_and_dtypes():
    kv = KVCache(2, 24, 3, 64, torch.bfloat16)
    q = AffineQuantizedKVCache.from_float(kv)
    assert q.k_cache.shape == q.v_cache.shape == (2, 3, 24, 64)
    assert q.k_cache.dtype == q.v_cache.dtype == torch.int8
    assert q.k_cache_scale.shape == q.v_cache_scale.shape == (2, 3, 24, 1)
    assert q.k_cache_scale.dtype == torch.bfloat16
    assert AffineQuantizedKVCache.from_float(
        KVCache(1, 8, 1, 16, torch.float32)).v_cache_scale.dtype == torch.float32


def test_setup_caches_installs_and_reallocates():
    model = Transformer(ModelArgs(dim=64, n_layer=2, n_head=4, vocab_size=50, block_size=64))
    model.setup_caches(1, 16)
    first = model.layers[0].attention.kv_cache
    assert type(first) is KVCache
    model.setup_caches(1, 16)  # nothing changed: kept
    assert model.layers[0].attention.kv_cache is first
    model.setup_caches(1, 16, kv_cache_quantization=True)  # only the flag: reallocated
    for blk in model.layers:
        kv = blk.attention.kv_cache
        assert type(kv) is AffineQuantizedKVCache
        assert kv.k_cache.shape == (1, 4, 16, 16) and kv.k_cache_scale.dtype == torch.float32
    quant = model.layers[0].attention.kv_cache
    model.setup_caches(1, 8, True)  # smaller, same flag: kept
    assert model.layers[0].attention.kv_cache is quant
    model.setup_caches(1, 16)  # the flag off again: back to KVCache
    assert type(model.layers[0].attention.kv_cache) is KVCache


def _model_weights(state, seed):
    """experiments/gen_golden_kvq8.py model_weights: deterministic weights by parameter name."""
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


@torch.no_grad()
def _decode_logits(model, prompt, steps):
    P = prompt.shape[1]
    logits = model(prompt, torch.arange(P))
    tok = logits[:, -1].argmax(-1, keepdim=True)
    out = []
    for i in range(steps):
        logits = model(tok, torch.tensor([P + i]))
        out.append(logits[0, -1].float())
        tok = logits[:, -1].argmax(-1, keepdim=True)
    return torch.stack(out)


def test_stories15m_decode_stays_close_cpu(gold):
    """KV-cache decode with the flag against the unquantized run, stories15M in bf16 on the CPU,
    the generator's weights, prompt and steps. The measure is test_graph_decode_matches_eager_gpu's
    for quantization error, 20 log10(|l| / |l - l_q|). The reference's own figure on this input is
    in the fixture (sd_sqnr_db, 41.3 dB). update() is the reference's arithmetic bit for bit
    (test_cache_update_matches_reference_run), so what can differ is the bf16 rounding of the two
    packages' eager RMSNorm / RoPE / SDPA formulations, which moves both runs alike; the margin
    allowed below the reference's figure is 3 dB (a factor 1.4 in the error norm)."""
    seed, steps = int(gold["sd_seed"]), int(gold["sd_steps"])
    prompt = torch.tensor(gold["sd_prompt"])
    logits = {}
    for quant in (False, True):
        model = Transformer.from_name("stories15M").to(torch.bfloat16).eval()
        model.load_state_dict(_model_weights(model.state_dict(), seed))
        model.setup_caches(1, prompt.shape[1] + steps + 1, kv_cache_quantization=quant)
        logits[quant] = _decode_logits(model, prompt, steps)
    sqnr = float(20 * torch.log10(logits[False].norm() / (logits[False] - logits[True]).norm()))
    ref = float(gold["sd_sqnr_db"])
    print(f"stories15M int8 KV cache: SQNR {sqnr:.2f} dB, reference {ref:.2f} dB")
    assert sqnr > ref - 3.0, (sqnr, ref)


def test_library_refuses_bad_shapes_before_device_work():
    from torchao import _lib

    lib = _lib.lib()
    n = None
    # (B, S, H, Hkv, D, T) / (B, H, Hkv, D, T, scale, splits), null pointers throughout
    assert lib.tao_rope_kv_q8_bf16(n, n, n, n, n, n, n, n, n, n, 1, 1, 8, 2, 64, 16, n) == 1
    assert b"head_dim must be 128" in lib.tao_last_error()
    assert lib.tao_attn_decode_q8_bf16(n, n, n, n, n, n, n, n, n, n, 1, 8, 2, 64, 16, 1.0, 1,
                                       n) == 1
    assert b"head_dim must be 128" in lib.tao_last_error()
    assert lib.tao_attn_decode_q8_bf16(n, n, n, n, n, n, n, n, n, n, 1, 8, 2, 128, 16, 1.0, 3,
                                       n) == 1
    assert b"splits must be 1, 2 or 4" in lib.tao_last_error()
    assert lib.tao_attn_decode_q8_bf16(n, n, n, n, n, n, n, n, n, n, 1, 6, 2, 128, 16, 1.0, 1,
                                       n) == 1
    assert b"H / Hkv must be 1, 2, 4 or 8" in lib.tao_last_error()
    with pytest.raises(RuntimeError, match="splits must be 1, 2 or 4"):
        _lib.call("tao_attn_decode_q8_bf16", n, n, n, n, n, n, n, n, n, n, 1, 8, 2, 128, 16, 1.0,
                  8, n)
