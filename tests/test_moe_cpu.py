"""CPU tests of torchao.prototype.moe_quant against the reference fixtures (tests/golden/moe_*,
experiments/gen_golden_moe.py): the plain module bit for bit in its one-token and many-token
branches, the config and filters, every refusal leaving the module untouched, the launch rule of
csrc/moe_host.h through the C ABI and its hook, and the int8 weight-only fixture through
``quantize_``."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import bf16, load_golden

from torchao import _lib
from torchao.prototype.moe_quant import (ConditionalFeedForwardAOQuantizable,
                                         MOEFeedForwardAOQuantizable, MoEQuantConfig,
                                         UseFakeExtraDimTensor, cond_ffn_filter, moe_filter)
from torchao.quantization import (Float8WeightOnlyConfig,
                                  Int8DynamicActivationInt8WeightConfig, Int8WeightOnlyConfig,
                                  quantize_)

E, D, I = 4, 64, 128
TOKENS = (1, 2, 7)
TOP_KS = (1, 2, 3)


def _fixture(A):
    return load_golden(f"moe_E{E}_D{D}_I{I}_k{A}.npz")


def _module(rec, A, **kw):
    m = MOEFeedForwardAOQuantizable(D, I, E, A, return_scores=True, **kw).to(torch.bfloat16)
    with torch.no_grad():
        m.router.weight.copy_(bf16(rec["router"]))
        for name in ("w1", "w2", "w3"):
            getattr(m.experts, name).copy_(bf16(rec[name]))
    return m


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("A", TOP_KS)
@pytest.mark.parametrize("T", TOKENS)
def test_plain_module_matches_reference_bit_for_bit(A, T):
    """T = 1 is the one-token branch (cat, mul, sum over the experts), T > 1 the many-token branch
    (sort, per-expert linears, scatter_add); the routing the experts saw is rebuilt exactly too."""
    rec = _fixture(A)
    m = _module(rec, A)
    seen = {}
    m.experts.register_forward_pre_hook(lambda mod, args: seen.update(idx=args[1]))
    with torch.no_grad():
        y, scores = m(bf16(rec[f"x_T{T}"]))
    assert torch.equal(seen["idx"], torch.from_numpy(rec[f"idx_T{T}"]))
    assert torch.equal(scores, bf16(rec[f"scores_T{T}"]))
    assert y.shape == (T, 1, D)
    assert torch.equal(y, bf16(rec[f"y_T{T}"]))


def test_module_attributes_and_shared_expert():
    m = MOEFeedForwardAOQuantizable(D, I, E, 2)
    assert isinstance(m.router, torch.nn.Linear) and m.router.bias is None
    assert isinstance(m.experts, ConditionalFeedForwardAOQuantizable)
    assert (m.hidden_dim, m.top_k, m.shared_expert, m.return_scores) == (D, 2, None, False)
    ex = m.experts
    assert ex.w1.shape == (E, I, D) and ex.w2.shape == (E, D, I) and ex.w3.shape == (E, I, D)
    assert ex.act_fn is F.silu and (ex.num_experts, ex.hidden_dim, ex.expert_dim) == (E, D, I)
    rec = _fixture(2)
    shared = torch.nn.Linear(D, D, bias=False).to(torch.bfloat16)
    m = MOEFeedForwardAOQuantizable(D, I, E, 2, shared_expert=shared).to(torch.bfloat16)
    with torch.no_grad():
        m.router.weight.copy_(bf16(rec["router"]))
        for name in ("w1", "w2", "w3"):
            getattr(m.experts, name).copy_(bf16(rec[name]))
        x = bf16(rec["x_T7"])
        want = (bf16(rec["y_T7"]).view(-1, D) + shared(x.view(-1, D))).reshape(7, 1, D)
        assert torch.equal(m(x), want)


def test_config_fields_and_defaults():
    base = Int8WeightOnlyConfig()
    c = MoEQuantConfig(base)
    assert c.base_config is base
    assert c.use_fake_extra_dim_tensor is UseFakeExtraDimTensor.AS_FALLBACK
    assert c.set_inductor_config is True
    assert [v.name for v in UseFakeExtraDimTensor] == ["TRUE", "FALSE", "AS_FALLBACK"]
    c = MoEQuantConfig(base, UseFakeExtraDimTensor.FALSE, False)
    assert c.use_fake_extra_dim_tensor is UseFakeExtraDimTensor.FALSE and not c.set_inductor_config
    from torchao.core.config import AOBaseConfig
    from torchao.quantization.transform_module import _QUANTIZE_CONFIG_HANDLER

    assert isinstance(c, AOBaseConfig) and MoEQuantConfig in _QUANTIZE_CONFIG_HANDLER


def test_filters():
    m = torch.nn.Sequential(MOEFeedForwardAOQuantizable(D, I, E, 2), torch.nn.Linear(D, D))
    hits = {fqn: (moe_filter(mod, fqn), cond_ffn_filter(mod, fqn))
            for fqn, mod in m.named_modules()}
    assert hits["0"] == (True, False)
    assert hits["0.experts"] == (False, True)
    assert hits["0.router"] == hits["1"] == hits[""] == (False, False)


def _snapshot(m):
    return {n: (p, p.detach().clone()) for n, p in m.named_parameters()}


def _untouched(m, snap):
    now = dict(m.named_parameters())
    return set(now) == set(snap) and all(
        now[n] is p and type(now[n]) is torch.nn.Parameter and torch.equal(now[n], v)
        for n, (p, v) in snap.items())


@pytest.mark.parametrize("config,exc,match", [
    (MoEQuantConfig(Int8WeightOnlyConfig(), UseFakeExtraDimTensor.TRUE), NotImplementedError,
     "FakeExtraDimTensor is not served; served: Int4WeightOnlyConfig"),
    (MoEQuantConfig(Int8DynamicActivationInt8WeightConfig()), NotImplementedError,
     "Int8DynamicActivationInt8WeightConfig.* is not served; served: Int4WeightOnlyConfig"),
    (MoEQuantConfig(Float8WeightOnlyConfig(version=2)), NotImplementedError,
     "FakeExtraDimTensor fallback is not served; served: Int4WeightOnlyConfig"),
    (MoEQuantConfig(Float8WeightOnlyConfig(version=2), UseFakeExtraDimTensor.FALSE),
     NotImplementedError, "version=2"),
    (MoEQuantConfig(Int8WeightOnlyConfig), TypeError, "AOBaseConfig instance"),
])
def test_refusals_leave_every_module_untouched(config, exc, match):
    """Two MoE layers: the refusal comes before any parameter of either is replaced."""
    rec = _fixture(2)
    m = torch.nn.Sequential(_module(rec, 2), _module(rec, 2))
    snap = _snapshot(m)
    with pytest.raises(exc, match=match):
        quantize_(m, config, cond_ffn_filter)
    assert _untouched(m, snap)


def test_refusal_of_a_later_module_leaves_the_first_untouched():
    """The second layer's w2 is 2-D: nothing of the first, which is fine by itself, is swapped."""
    rec = _fixture(2)
    m = torch.nn.Sequential(_module(rec, 2), _module(rec, 2))
    m[1].experts.w2 = torch.nn.Parameter(torch.zeros(D, I, dtype=torch.bfloat16))
    snap = _snapshot(m)
    with pytest.raises(ValueError, match="expected a 3-D tensor for w2"):
        quantize_(m, MoEQuantConfig(Int8WeightOnlyConfig()), cond_ffn_filter)
    assert _untouched(m, snap)


def test_row_tile_rule_and_tuning_hook():
    """csrc/moe_host.h through the C ABI: 16 rows per tile while the mean rows per expert is at
    most 4, 64 from a mean of 64, 32 between (the measured rule); the hook forces either choice and tao_tune_reset restores both."""
    lib = _lib.lib()
    tile, dual = lib.tao_moe_row_tile, lib.tao_moe_dual
    _lib.call("tao_tune_reset")
    assert [tile(r, 8) for r in (2, 32, 33, 511, 512, 2048)] == [16, 16, 32, 32, 64, 64]
    assert [tile(r, 256) for r in (24, 1024, 1025, 16384)] == [16, 16, 32, 64]
    built_in = dual(64, 8)
    assert built_in in (0, 1)
    try:
        for bm in (16, 32, 64):
            _lib.call("tao_tune_moe", bm, 0)
            assert tile(2, 8) == tile(100000, 8) == bm
        _lib.call("tao_tune_moe", 0, 1)
        assert dual(64, 8) == 0 and tile(33, 8) == 32
        _lib.call("tao_tune_moe", 0, 2)
        assert dual(64, 8) == 1
        for bad in ((8, 0), (128, 0), (0, 3), (0, -1)):
            with pytest.raises(RuntimeError, match="tune: moe"):
                _lib.call("tao_tune_moe", *bad)
    finally:
        _lib.call("tao_tune_reset")
    assert tile(2, 8) == 16 and dual(64, 8) == built_in
    from torchao.kernel.tuning import tuning

    with tuning(moe=(64, 1)):
        assert tile(2, 8) == 64 and dual(64, 8) == 0
    assert tile(2, 8) == 16 and dual(64, 8) == built_in


def test_entry_bounds_are_checked_before_any_launch():
    lib = _lib.lib()

    def err(rc):
        assert rc != 0
        return lib.tao_last_error().decode()

    assert "E (257) must be in [1, 256]" in err(
        lib.tao_moe_route(None, 8, 2, 257, None, None, None, None))
    assert "top-k (9) must be in [1, 8]" in err(
        lib.tao_moe_route(None, 9, 9, 4, None, None, None, None))
    assert "multiple of top-k" in err(lib.tao_moe_route(None, 7, 2, 4, None, None, None, None))
    assert "must be a multiple of 32" in err(lib.tao_int4wo_grouped_linear_bf16(
        None, 4, None, 1, None, None, None, None, None, 4, 4, None, 64, 48, 32, None))
    assert "E (300)" in err(lib.tao_int4wo_grouped_linear_bf16(
        None, 4, None, 1, None, None, None, None, None, 4, 300, None, 64, 64, 32, None))
    assert "top-k (0)" in err(lib.tao_moe_combine_bf16(None, None, None, None, 4, 0, 64, None))
    assert "D (12) must be a multiple of 8" in err(
        lib.tao_moe_combine_bf16(None, None, None, None, 4, 2, 12, None))


@pytest.mark.parametrize("A", TOP_KS)
def test_int8wo_fixture_through_quantize(A):
    """quantize_(m, MoEQuantConfig(Int8WeightOnlyConfig(), FALSE), cond_ffn_filter) on the CPU, held
    to the reference's own quantization error: rel-L2 of its recorded int8 output against its
    recorded plain output (1.2e-2 to 1.7e-2 here). Both quantize the same weights with the same
    per-channel symmetric scheme and differ at most in where the dequantized matmul rounds to bf16,
    a relative 2^-8 per output against a quantization error five times that, so the margin is
    1.1 x the reference's error."""
    rec = _fixture(A)
    m = _module(rec, A)
    quantize_(m, MoEQuantConfig(Int8WeightOnlyConfig(), UseFakeExtraDimTensor.FALSE),
              cond_ffn_filter)
    from torchao.dtypes import AffineQuantizedTensor

    for name in ("w1", "w2", "w3"):
        w = getattr(m.experts, name)
        assert isinstance(w, AffineQuantizedTensor) and w.dim() == 3 and not w.requires_grad
    assert type(m.router.weight) is torch.nn.Parameter  # cond_ffn_filter selects the experts only
    for T in TOKENS:
        with torch.no_grad():
            y, _ = m(bf16(rec[f"x_T{T}"]))
        plain, ref_q = bf16(rec[f"y_T{T}"]), bf16(rec[f"yq8_T{T}"])
        ref_err, err = rel_l2(ref_q, plain), rel_l2(y, plain)
        print(f"top-{A} T={T}: reference int8 error {ref_err:.3e}, here {err:.3e}, "
              f"equal to the reference's output: {torch.equal(y, ref_q)}")
        assert err <= 1.1 * ref_err, (T, err, ref_err)


def test_float8_base_config_quantizes_on_cpu():
    """Float8WeightOnlyConfig swaps all three weights for 3-D quantized tensors too; the bar is the
    project's float8 weight-only one against a bf16 result (tests/test_gpu_float8.py: 1e-1 on
    e4m3's 2^-4 relative step through three linears)."""
    from torchao.dtypes import AffineQuantizedTensor

    rec = _fixture(2)
    m = _module(rec, 2)
    quantize_(m, MoEQuantConfig(Float8WeightOnlyConfig()), cond_ffn_filter)
    for name in ("w1", "w2", "w3"):
        assert isinstance(getattr(m.experts, name), AffineQuantizedTensor)
    with torch.no_grad():
        y, _ = m(bf16(rec["x_T7"]))
    assert rel_l2(y, bf16(rec["y_T7"])) < 0.1
