"""Int8 KV cache on the GPU (torchao/_models/llama AffineQuantizedKVCache; csrc/kv_q8.hip):
tao_rope_kv_q8_bf16 against tao_rope_kv_bf16 and the torch quantizer, bit for bit;
tao_attn_decode_q8_bf16 against fp32 SDPA over the dequantized codes with the current token exact
(rtol / atol 2e-2, the bar of every attention test here: every input is exact in fp32), run-to-run
identical, split and unsplit one bf16 rounding apart; and the Llama harness with the flag on: the
fused path against the unfused update() formulation, graph replay against eager."""

import math

import pytest
import torch
import torch.nn.functional as F

from torchao._models.llama.generate import GraphDecoder, apply_quantization, generate, prefill
from torchao._models.llama.model import (
    AffineQuantizedKVCache,
    KVCache,
    ModelArgs,
    Transformer,
    _rope_freqs,
)
from torchao.quantization.utils import _quantize_activation_per_token_absmax

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 128
B, HKV = 2, 2


@pytest.mark.parametrize("S,positions", [(1, [13]), (5, [3, 17, 4, 30, 0])])
def test_rope_kv_q8_matches_rope_kv_and_quantizer(S, positions):
    from torchao._models.llama import kernels

    H, T = 8, 32
    g = torch.Generator(device=DEV).manual_seed(S)
    qkv = torch.randn(B, S, (H + 2 * HKV) * D, device=DEV, dtype=torch.bfloat16, generator=g)
    qkv[0, 0, H * D:(H + 1) * D] = 0  # an all-zero k row: the eps scale
    freqs = _rope_freqs(ModelArgs(dim=H * D, n_head=H, n_local_heads=HKV), 64).to(DEV)
    pos = torch.tensor(positions, device=DEV)
    ref = KVCache(B, T, HKV, D, torch.bfloat16, DEV)
    q_ref = kernels.rope_kv(qkv, freqs, pos, ref.k_cache, ref.v_cache, H)
    kv = AffineQuantizedKVCache(B, T, HKV, D, device=DEV)
    kv.k_cache.fill_(77)
    kv.v_cache.fill_(-77)
    kv.k_cache_scale.fill_(3.0)
    kv.v_cache_scale.fill_(5.0)
    q, k_cur, v_cur = kernels.rope_kv_q8(qkv, freqs, pos, kv, H)
    assert torch.equal(q, q_ref)
    assert torch.equal(k_cur, ref.k_cache[:, :, pos]) and torch.equal(v_cur, ref.v_cache[:, :, pos])
    for cur, codes, scales, sent_c, sent_s in ((k_cur, kv.k_cache, kv.k_cache_scale, 77, 3.0),
                                               (v_cur, kv.v_cache, kv.v_cache_scale, -77, 5.0)):
        cq, cs = _quantize_activation_per_token_absmax(cur)
        assert torch.equal(codes[:, :, pos], cq)
        assert torch.equal(scales[:, :, pos, 0], cs)
        rest = torch.ones(T, dtype=torch.bool, device=DEV)
        rest[pos] = False
        assert bool((codes[:, :, rest] == sent_c).all())
        assert bool((scales[:, :, rest] == sent_s).all())
    assert float(kv.k_cache_scale[0, 0, positions[0], 0]) == pytest.approx(1e-5, rel=1e-2)
    kernels.check_decode_status()


def test_rope_kv_q8_out_of_range_position_is_reported():
    from torchao._models.llama import kernels

    H, T = 8, 16
    qkv = torch.randn(B, 1, (H + 2 * HKV) * D, device=DEV, dtype=torch.bfloat16)
    freqs = _rope_freqs(ModelArgs(dim=H * D, n_head=H, n_local_heads=HKV), 64).to(DEV)
    kv = AffineQuantizedKVCache(B, T, HKV, D, device=DEV)
    kv.k_cache.fill_(9)
    kv.v_cache_scale.fill_(2.0)
    before = [b.clone() for b in kv.buffers()]
    canary = torch.full((4096,), 7, dtype=torch.int32, device=DEV)  # neighbouring allocation
    kernels.check_decode_status()
    for p in (T, -1):
        kernels.rope_kv_q8(qkv, freqs, torch.tensor([p], device=DEV), kv, H)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="past the KV cache"):
            kernels.check_decode_status()
        kernels.check_decode_status()  # the read cleared it
        for b, b0 in zip(kv.buffers(), before):
            assert torch.equal(b, b0)
    assert bool((canary == 7).all())


# (cache rows T, keys attended L): one key (the current token alone), the 16-key rounding of the
# ranges (16 cached keys at L = 17), empty trailing splits, more than one 256-key round per
# workgroup, the full cache, and a cache past the bf16 single-pass kernel's 1024 rows
CASES = ((64, 1), (64, 2), (64, 16), (64, 17), (64, 18), (328, 129), (328, 328), (1536, 1100))
_CASE_CACHE = {}


def _case(G, T, L):
    """Inputs of one attention case and its fp32 reference, made once and shared by the splits."""
    key = (G, T, L)
    if key not in _CASE_CACHE:
        H = HKV * G
        g = torch.Generator(device=DEV).manual_seed(1000 * G + T + L)
        kv = AffineQuantizedKVCache(B, T, HKV, D, device=DEV)
        for name in ("k_cache", "v_cache"):
            getattr(kv, name).copy_(torch.randint(-127, 128, (B, HKV, T, D), device=DEV,
                                                  generator=g))
            getattr(kv, name + "_scale").copy_(
                torch.rand(B, HKV, T, 1, device=DEV, generator=g) * 0.03 + 0.004)
        q = torch.randn(B, H, 1, D, device=DEV, dtype=torch.bfloat16, generator=g)
        k_cur = torch.randn(B, HKV, 1, D, device=DEV, dtype=torch.bfloat16, generator=g)
        v_cur = torch.randn(B, HKV, 1, D, device=DEV, dtype=torch.bfloat16, generator=g)
        kd = (kv.k_cache.float() * kv.k_cache_scale.float())[:, :, :L].clone()
        vd = (kv.v_cache.float() * kv.v_cache_scale.float())[:, :, :L].clone()
        kd[:, :, L - 1] = k_cur[:, :, 0].float()
        vd[:, :, L - 1] = v_cur[:, :, 0].float()
        ref = F.scaled_dot_product_attention(q.float(), kd, vd, enable_gqa=True)
        _CASE_CACHE[key] = (kv, q, k_cur, v_cur, ref.transpose(1, 2).reshape(B, 1, H * D))
    return _CASE_CACHE[key]


def _attend(kv, q, k_cur, v_cur, L, splits):
    from torchao._models.llama import kernels

    pos = torch.tensor([L - 1], device=DEV)
    y = kernels.attn_decode_q8(q, kv, k_cur, v_cur, pos, 1 / math.sqrt(D), splits)
    return y if splits == 1 else kernels.attn_merge(y, B, q.shape[1])


@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_attn_decode_q8_matches_sdpa(G, splits):
    for T, L in CASES:
        kv, q, k_cur, v_cur, ref = _case(G, T, L)
        got = _attend(kv, q, k_cur, v_cur, L, splits)
        assert torch.equal(got, _attend(kv, q, k_cur, v_cur, L, splits)), (T, L)
        err = (got.float() - ref).abs().max()
        print(f"G {G} splits {splits} T {T} L {L}: max abs err {float(err):.3e}")
        torch.testing.assert_close(got.float(), ref, rtol=2e-2, atol=2e-2)
        if splits > 1:
            # same fp32 softmax and P.V, another association of the sums: one bf16 rounding apart
            one = _attend(kv, q, k_cur, v_cur, L, 1).float()
            diff = (got.float() - one).abs()
            assert (diff <= one.abs() * 2 ** -7 + 1e-6).all(), (T, L, float(diff.max()))


@pytest.mark.parametrize("splits", [1, 4])
def test_attn_decode_q8_current_token_comes_from_k_cur(splits):
    """Row L - 1 of the caches (the current token's codes) and every row past it are not read:
    garbage there changes nothing, while k_cur / v_cur do matter."""
    T, L = 64, 17
    kv, q, k_cur, v_cur, ref = _case(4, T, L)
    got = _attend(kv, q, k_cur, v_cur, L, splits)
    bad = AffineQuantizedKVCache(B, T, HKV, D, device=DEV)
    for b, b0 in zip(bad.buffers(), kv.buffers()):
        b.copy_(b0)
    bad.k_cache[:, :, L - 1:] = 127
    bad.v_cache[:, :, L - 1:] = -127
    bad.k_cache_scale[:, :, L - 1:] = 1000.0
    bad.v_cache_scale[:, :, L - 1:] = 1000.0
    assert torch.equal(_attend(bad, q, k_cur, v_cur, L, splits), got)
    torch.testing.assert_close(got.float(), ref, rtol=2e-2, atol=2e-2)
    other = _attend(kv, q, k_cur, (v_cur.float() + 4).to(torch.bfloat16), L, splits)
    assert not torch.equal(other, got)


# test_llama_harness.py's head_dim-128 GQA model (the fused kernels need head_dim 128)
TINY = dict(dim=512, n_layer=2, n_head=4, n_local_heads=2, vocab_size=1000, block_size=256)


def _tiny(seed=2):
    torch.manual_seed(seed)
    model = Transformer(ModelArgs(**TINY)).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.Linear):
                b = 1 / math.sqrt(mod.in_features)
                mod.weight.uniform_(-b, b)
        for blk in model.layers:  # non-trivial norm weights
            blk.attention_norm.weight.uniform_(0.5, 1.5)
            blk.ffn_norm.weight.uniform_(0.5, 1.5)
    return model.eval()


def _prefill_both_paths(quant, P, T):
    """The tiny model with int8 caches: the unfused prefill's cache buffers (cloned), its logits
    of one step at position P, and the model after a FUSED prefill of the same prompt into caches
    first filled with a sentinel (codes 55, scales 7)."""
    dev = torch.device(DEV)
    model = _tiny()
    apply_quantization(model, quant)
    model.setup_caches(1, P + T, kv_cache_quantization=True)
    assert all(type(b.attention.kv_cache) is AffineQuantizedKVCache for b in model.layers)
    torch.manual_seed(4)
    prompt = torch.randint(0, 1000, (1, P), device=dev)
    pos = torch.arange(P, device=dev)
    with torch.no_grad():
        assert not model.fused
        model(prompt, pos)
        cref = [[b.clone() for b in blk.attention.kv_cache.buffers()] for blk in model.layers]
        ref = model(prompt[:, -1:], torch.tensor([P], device=dev))
        assert model.enable_fused_kernels()
        for blk in model.layers:
            kv = blk.attention.kv_cache
            kv.k_cache.fill_(55)
            kv.v_cache.fill_(55)
            kv.k_cache_scale.fill_(7.0)
            kv.v_cache_scale.fill_(7.0)
        model(prompt, pos)  # fused prefill: rope_kv_q8, SDPA over the exact rows
    return model, prompt, pos, cref, ref


def _assert_caches_equal(blk, bufs, P, what):
    for b, b0 in zip(blk.attention.kv_cache.buffers(), bufs):
        same = float((b[:, :, :P] == b0[:, :, :P]).float().mean())
        print(f"{what} {tuple(b.shape)} {b.dtype}: {same:.4f} of the written entries equal")
    for b, b0 in zip(blk.attention.kv_cache.buffers(), bufs):
        assert torch.equal(b[:, :, :P], b0[:, :, :P]), what
        assert bool((b[:, :, P:] == (55 if b.dtype == torch.int8 else 7.0)).all()), what


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("quant", [None, "int4wo-32"])
def test_model_fused_matches_unfused_with_int8_cache(quant, split, monkeypatch):
    """Fused prefill + one fused step against the unfused forward (update() and SDPA) on the same
    model: logits within test_fused_decode_matches_unfused_gpu's bar; the first layer's int8 caches
    and scales (the layer both paths enter with the same bits) bit-equal after prefill and nothing
    written past the prompt; graph-replayed decode == eager fused decode over 12 steps. split: the
    attention over one key range, or over four (forced for this small cache) with the merge in its
    own launch (bf16 wo) or folded into the int4 wo."""
    from torchao._models.llama import kernels

    monkeypatch.setattr(kernels, "ATTN_Q8_SPLIT_MIN_T", 0 if split else 10 ** 9)
    P, T = 9, 12
    model, prompt, pos, cref, ref = _prefill_both_paths(quant, P, T)
    _assert_caches_equal(model.layers[0], cref[0], P, "layer 0")
    with torch.no_grad():
        got = model(prompt[:, -1:], torch.tensor([P], device=DEV))
    rel = (got - ref).norm() / ref.norm()
    print(f"quant {quant}: fused vs unfused step, rel {float(rel):.3e}")
    assert rel < 2e-2, float(rel)
    eager, _, _ = generate(model, prompt, T, None)
    dec = GraphDecoder(model, 1, P + T, torch.device(DEV))
    dec.reset(prompt, prefill(model, prompt, pos))
    dec.capture()
    graphed, _, _ = generate(model, prompt, T, dec)
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("quant", [None, "int4wo-32"])
def test_model_int8_caches_bit_equal_after_prefill(quant):
    """The int8 caches and scales of EVERY layer bit-equal between the fused and the unfused
    prefill. A layer past the first quantizes rows that went through the layer before it, its
    attention included, so this holds only because the fused prefill over an int8 cache attends
    with the unfused path's own SDPA call (Attention._prefill_q8); with tao_attn_prefill_bf16
    there, 92 % of the second layer's codes and 78-94 % of its scales were equal. Everything else
    on the fused path (rope_kv_q8, the fused norms, SiLU-mul, the int4 GEMMs' epilogues) adds no
    difference."""
    P = 9
    model, _, _, cref, _ = _prefill_both_paths(quant, P, 12)
    for i, (blk, bufs) in enumerate(zip(model.layers, cref)):
        _assert_caches_equal(blk, bufs, P, f"layer {i}")


def test_model_prefill_past_zero_takes_update_formulation():
    """A fused prefill that does not start at 0 goes through update() and SDPA: the same logits as
    the unfused forward, bit for bit up to the fused norms and linears' bar."""
    dev = torch.device(DEV)
    model = _tiny(seed=3)
    model.setup_caches(1, 24, kv_cache_quantization=True)
    prompt = torch.randint(0, 1000, (1, 12), device=dev)
    with torch.no_grad():
        model(prompt[:, :5], torch.arange(5, device=dev))
        ref = model(prompt[:, 5:], torch.arange(5, 12, device=dev))
        assert model.enable_fused_kernels()
        model(prompt[:, :5], torch.arange(5, device=dev))
        got = model(prompt[:, 5:], torch.arange(5, 12, device=dev))
    rel = (got - ref).norm() / ref.norm()
    assert rel < 2e-2, float(rel)
