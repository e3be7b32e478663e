"""CPU tests of the SmoothQuant workflow (torchao.prototype.smoothquant, quantization/observer.py,
quantization/weight_tensor_linear_activation_quantization.py) against the reference's own results
(tests/golden/smoothquant_*.npz and smoothquant_recipe_*.pt, experiments/gen_golden_smoothquant.py):
the observer's qparams, the converted weight, the wrapper structure, the recipe round trip and the
reference's recipe files, the static wrapper's tensor protocol, the refusals, and the plain-torch
restatement of the activation quantizers and the int8 linear that the GPU tests use as their
oracle (tests/smoothquant_oracle.py). No GPU compute: a CPU forward of a converted module raises."""

import os

import pytest
import torch

import smoothquant_oracle as O
from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao.dtypes import AffineQuantizedTensor, PlainLayout
from torchao.prototype.smoothquant import (
    SmoothQuantConfig,
    SmoothQuantObservedLinear,
    SmoothQuantObserver,
    _ActQuantizer,
    insert_smooth_quant_observer_,
    load_smooth_quant_recipe,
    save_smooth_quant_recipe,
)
from torchao.quantization import (
    LinearActivationQuantizedTensor,
    WeightTensorWithLinearActivationScaleMetadata,
    quantize_,
)
from torchao.quantization.granularity import PerAxis as GranularityPerAxis
from torchao.quantization.observer import AffineQuantizedMinMaxObserver, PerAxis
from torchao.quantization.quant_primitives import MappingType
from torchao.quantization.weight_tensor_linear_activation_quantization import (
    WeightTensorWithLinearActivationQuantizationMetadata,
    to_weight_tensor_with_linear_activation_quantization_metadata,
)

FIXTURES = ["smoothquant_N48_K512.npz", "smoothquant_N64_K256.npz", "smoothquant_N96_K1024.npz"]
ALPHAS = (None, 0.5, 0.75)
MODES = ("dynamic", "static")


def _tag(alpha, mode):
    return f"a{alpha}_{mode}"


def _is_observed(m, fqn):
    return isinstance(m, SmoothQuantObservedLinear)


def _model(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias="bias" in rec.files, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if lin.bias is not None:
            lin.bias.copy_(bf16(rec["bias"]))
    return torch.nn.Sequential(lin)


def _calibrated(rec, alpha, mode):
    model = _model(rec)
    insert_smooth_quant_observer_(model, alpha, mode)
    calib = bf16(rec["calib"])
    model(calib[:40])  # two batches: the running min / max must merge
    model(calib[40:])
    return model


def _layers(wt):
    """(outer, middle, aqt) of a converted weight."""
    return wt, wt.original_weight_tensor, wt.original_weight_tensor.original_weight_tensor


def _assert_weight_matches(wt, rec, tag, mode):
    outer, mid, aqt = _layers(wt)
    assert type(outer) is WeightTensorWithLinearActivationScaleMetadata
    assert outer.scale.dtype == torch.bfloat16
    assert torch.equal(outer.scale, bf16(rec[f"smoothing_factor_{tag}"]))
    if mode == "dynamic":
        assert type(mid) is LinearActivationQuantizedTensor
        fn = mid.input_quant_func
        assert fn.__func__ is _ActQuantizer.dynamic_quantize and mid.quant_kwargs == {}
    else:
        assert type(mid) is WeightTensorWithLinearActivationQuantizationMetadata
        fn = mid.input_quant_func_static
        assert fn.__func__ is _ActQuantizer.static_quantize and mid.quant_kwargs == {}
        assert mid.scale.dtype == torch.bfloat16 and mid.scale.dim() == 0
        assert torch.equal(mid.scale, bf16(rec[f"act_scales_{tag}"]).reshape(()))
        assert mid.zero_point.dtype == torch.int64 and mid.zero_point.dim() == 0
        assert int(mid.zero_point) == 0
    assert fn.__self__.target_dtype == torch.int8 and fn.__self__.quant_min == -127
    assert type(aqt) is AffineQuantizedTensor and isinstance(aqt._layout, PlainLayout)
    assert aqt.dtype == torch.bfloat16 and tuple(aqt.block_size) == (1, aqt.shape[1])
    q, s, z = aqt.tensor_impl.get_plain()
    assert q.dtype == torch.int8 and torch.equal(q, torch.from_numpy(rec[f"wq_{tag}"]))
    assert s.dtype == torch.bfloat16 and torch.equal(s.reshape(-1), bf16(rec[f"ws_{tag}"]))
    assert z.dtype == torch.int64 and not z.any()


def test_fixture_files_present_and_small():
    assert golden_files("smoothquant_N") == FIXTURES
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if not f.startswith("smoothquant"))
    for f in os.listdir(GOLDEN):
        if f.startswith("smoothquant"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= largest, f


def test_min_max_observer_and_per_axis():
    assert PerAxis is GranularityPerAxis and PerAxis(0) == PerAxis(0) and PerAxis(-1).axis == -1
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(6, 16, generator=gen).to(torch.bfloat16)
    b = torch.randn(3, 16, generator=gen).to(torch.bfloat16)
    obs = AffineQuantizedMinMaxObserver(MappingType.SYMMETRIC, torch.int8, PerAxis(-1))
    assert obs(a) is a
    assert torch.equal(obs.min_val, a.amin(0)) and torch.equal(obs.max_val, a.amax(0))
    obs(b)
    both = torch.cat([a, b])
    assert obs.min_val.dtype == torch.bfloat16
    assert torch.equal(obs.min_val, both.amin(0)) and torch.equal(obs.max_val, both.amax(0))
    row = AffineQuantizedMinMaxObserver(MappingType.SYMMETRIC, torch.int8, PerAxis(0),
                                        quant_min=-127, quant_max=127, eps=1e-5)
    row(a)
    scale, zp = row.calculate_qparams()
    ref = torch.clamp(a.abs().amax(1) / 127.0, min=1e-5)
    assert scale.dtype == torch.bfloat16 and torch.equal(scale, ref)
    assert tuple(zp.shape) == (6,) and not zp.any()
    with pytest.raises(AssertionError, match="run the observer"):
        AffineQuantizedMinMaxObserver(MappingType.SYMMETRIC, torch.int8,
                                      PerAxis(0)).calculate_qparams()


@pytest.mark.parametrize("name", FIXTURES)
def test_observer_qparams_match_the_reference_bit_for_bit(name):
    rec = load_golden(name)
    for alpha in ALPHAS:
        for mode in MODES:
            tag = _tag(alpha, mode)
            model = _calibrated(rec, alpha, mode)
            obs = model[0].obs
            assert isinstance(model[0], SmoothQuantObservedLinear)
            assert isinstance(obs, SmoothQuantObserver)
            factor, act_scales, wei_scales = obs.calculate_qparams()
            assert factor.dtype == torch.bfloat16 and wei_scales.dtype == torch.bfloat16
            assert torch.equal(factor, bf16(rec[f"smoothing_factor_{tag}"])), tag
            assert torch.equal(wei_scales, bf16(rec[f"wei_scales_{tag}"])), tag
            if mode == "dynamic":
                assert act_scales is None
            else:
                assert act_scales.dtype == torch.bfloat16 and act_scales.dim() == 0
                assert torch.equal(act_scales, bf16(rec[f"act_scales_{tag}"]).reshape(())), tag
            if alpha is None:
                assert torch.equal(factor, torch.ones_like(factor))


@pytest.mark.parametrize("name", FIXTURES)
def test_convert_matches_the_reference_structure_and_bits(name):
    rec = load_golden(name)
    for alpha in ALPHAS:
        for mode in MODES:
            model = _calibrated(rec, alpha, mode)
            bias = model[0].bias
            quantize_(model, SmoothQuantConfig(), _is_observed)
            lin = model[0]
            assert type(lin) is torch.nn.Linear and lin.bias is bias
            assert not lin.weight.requires_grad
            _assert_weight_matches(lin.weight, rec, _tag(alpha, mode), mode)
            assert "WeightTensorWithLinearActivationScaleMetadata" in repr(lin)


@pytest.mark.parametrize("mode", MODES)
def test_recipe_round_trip_equals_direct_convert(tmp_path, mode):
    rec = load_golden(FIXTURES[1])
    path = str(tmp_path / "recipe.pt")
    model = _calibrated(rec, 0.5, mode)
    save_smooth_quant_recipe(model, path)
    recipe = torch.load(path, weights_only=True)
    assert sorted(recipe) == ["0.act_scales", "0.smoothing_factor", "0.wei_scales"]
    assert (recipe["0.act_scales"] is None) == (mode == "dynamic")
    fresh = _model(rec)
    insert_smooth_quant_observer_(fresh, 0.5, mode)  # no calibration: the recipe brings the qparams
    load_smooth_quant_recipe(fresh, path)
    quantize_(model, SmoothQuantConfig(), _is_observed)
    assert type(fresh[0]) is torch.nn.Linear
    for a, b in zip(_layers(fresh[0].weight), _layers(model[0].weight)):
        assert type(a) is type(b)
    _assert_weight_matches(fresh[0].weight, rec, _tag(0.5, mode), mode)
    _assert_weight_matches(model[0].weight, rec, _tag(0.5, mode), mode)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mode", MODES)
def test_reference_recipe_loads_and_converts_to_the_same_bits(name, mode):
    rec = load_golden(name)
    path = os.path.join(GOLDEN, name.replace("smoothquant_", "smoothquant_recipe_")
                        .replace(".npz", f"_{mode}.pt"))
    recipe = torch.load(path, weights_only=True)
    tag = _tag(0.5, mode)
    assert torch.equal(recipe["0.smoothing_factor"], bf16(rec[f"smoothing_factor_{tag}"]))
    model = _model(rec)
    insert_smooth_quant_observer_(model, 0.5, mode)
    load_smooth_quant_recipe(model, path)
    _assert_weight_matches(model[0].weight, rec, tag, mode)
    # a layer the recipe does not name stays observed
    other = torch.nn.Sequential(torch.nn.Identity(), _model(rec)[0])
    insert_smooth_quant_observer_(other, 0.5, mode)
    load_smooth_quant_recipe(other, path)
    assert isinstance(other[1], SmoothQuantObservedLinear)


def test_static_wrapper_tensor_protocol():
    rec = load_golden(FIXTURES[1])
    model = _calibrated(rec, 0.5, "static")
    quantize_(model, SmoothQuantConfig(), _is_observed)
    mid = model[0].weight.original_weight_tensor
    names, attrs = mid.__tensor_flatten__()
    assert names == ["original_weight_tensor", "scale", "zero_point"]
    assert attrs[0] is mid.input_quant_func_static and attrs[1] == {}
    again = WeightTensorWithLinearActivationQuantizationMetadata.__tensor_unflatten__(
        {n: getattr(mid, n) for n in names}, attrs, mid.shape, mid.stride())
    assert again.scale is mid.scale and again.zero_point is mid.zero_point
    no_zp = to_weight_tensor_with_linear_activation_quantization_metadata(
        mid.original_weight_tensor, mid.input_quant_func_static, mid.scale)
    assert no_zp.zero_point is None and no_zp.quant_kwargs == {}
    assert no_zp.__tensor_flatten__()[0] == ["original_weight_tensor", "scale"]
    q0 = mid.original_weight_tensor.tensor_impl.int_data
    for out in (mid.clone(), mid.detach(), mid.to("cpu"), no_zp.clone(),
                torch.ops.aten._to_copy.default(mid, device=torch.device("cpu"))):
        assert type(out) is WeightTensorWithLinearActivationQuantizationMetadata
        assert out.shape == mid.shape and out.dtype == torch.bfloat16
        assert torch.equal(out.original_weight_tensor.tensor_impl.int_data, q0)
        assert torch.equal(out.scale, mid.scale) and out.scale.dtype == torch.bfloat16
        assert out.input_quant_func_static is mid.input_quant_func_static
    cl = mid.clone()
    assert cl.scale.data_ptr() != mid.scale.data_ptr()
    assert cl.zero_point.dtype == torch.int64
    tr = mid.t()
    assert type(tr) is WeightTensorWithLinearActivationQuantizationMetadata
    assert tuple(tr.shape) == (mid.shape[1], mid.shape[0])
    assert torch.equal(tr.original_weight_tensor.tensor_impl.int_data, q0.t())
    assert torch.equal(tr.scale, mid.scale)
    # the whole converted weight survives detach / clone too (nn.Parameter does both)
    outer = model[0].weight.detach().clone()
    _assert_weight_matches(outer, rec, _tag(0.5, "static"), "static")
    assert "WeightTensorWithLinearActivationQuantizationMetadata" in repr(mid)


def test_refused_inputs_raise_and_leave_the_module_unchanged():
    def untouched(model, lin, w):
        return model[0] is lin and lin.weight is w and type(w) is torch.nn.Parameter

    lin = torch.nn.Linear(72, 16, dtype=torch.bfloat16)  # K % 16 != 0
    model, w = torch.nn.Sequential(lin), lin.weight
    with pytest.raises(NotImplementedError, match=r"in_features = 72.*served: 2-D"):
        insert_smooth_quant_observer_(model)
    assert untouched(model, lin, w)
    cfg = SmoothQuantConfig(torch.ones(72, dtype=torch.bfloat16), None,
                            torch.ones(16, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="in_features = 72"):
        quantize_(model, cfg)
    assert untouched(model, lin, w)

    class Experts(torch.nn.Module):  # a 3-D (MoE) weight behind a filter that selects it
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(2, 16, 32, dtype=torch.bfloat16))
            self.bias = None
            self.in_features, self.out_features = 32, 16

    moe = torch.nn.Sequential(Experts())
    w3 = moe[0].weight
    with pytest.raises(NotImplementedError, match="3-D weight"):
        quantize_(moe, cfg, lambda m, fqn: isinstance(m, Experts))
    assert moe[0].weight is w3 and isinstance(moe[0], Experts)

    # a second linear that is refused keeps the first one unobserved as well
    two = torch.nn.Sequential(torch.nn.Linear(32, 16, dtype=torch.bfloat16),
                              torch.nn.Linear(16, 8, dtype=torch.bfloat16),
                              torch.nn.Linear(8, 8, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="in_features = 8"):
        insert_smooth_quant_observer_(two)
    assert all(type(m) is torch.nn.Linear for m in two)

    # converting a linear that was never observed, without a recipe
    plain = torch.nn.Sequential(torch.nn.Linear(32, 16, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="SmoothQuantObservedLinear"):
        quantize_(plain, SmoothQuantConfig())
    assert type(plain[0].weight) is torch.nn.Parameter


def test_float32_module_converts_on_the_cpu():
    """Convert is plain torch: any float dtype on the CPU (the GPU route is bf16 only)."""
    gen = torch.Generator().manual_seed(11)
    model = torch.nn.Sequential(torch.nn.Linear(32, 16))
    insert_smooth_quant_observer_(model, 0.5, "static")
    model(torch.randn(8, 32, generator=gen))
    quantize_(model, SmoothQuantConfig(), _is_observed)
    outer, mid, aqt = _layers(model[0].weight)
    assert outer.scale.dtype == torch.float32 and mid.scale.dtype == torch.float32
    assert aqt.tensor_impl.int_data.dtype == torch.int8


def test_cpu_forward_of_a_converted_module_raises():
    rec = load_golden(FIXTURES[1])
    model = _calibrated(rec, 0.5, "dynamic")
    quantize_(model, SmoothQuantConfig(), _is_observed)
    with pytest.raises((NotImplementedError, RuntimeError)):
        model(bf16(rec["x"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_restatement_reproduces_the_reference(name):
    """tests/smoothquant_oracle.py against the reference's recorded activation codes, scales and
    CPU forward, bit for bit: the GPU tests' oracle is pinned by the reference."""
    rec = load_golden(name)
    x = bf16(rec["x"])
    bias = bf16(rec["bias"]) if "bias" in rec.files else None
    for alpha in ALPHAS:
        for mode in MODES:
            tag = _tag(alpha, mode)
            factor = bf16(rec[f"smoothing_factor_{tag}"])
            act = bf16(rec[f"act_scales_{tag}"]).reshape(()) if mode == "static" else None
            xq, xs = O.quant(x, factor, act)
            assert torch.equal(xq, torch.from_numpy(rec[f"xq_{tag}"])), tag
            ref_s = bf16(rec[f"xs_{tag}"])
            assert torch.equal(xs, ref_s if mode == "dynamic" else ref_s.expand(5)), tag
            if mode == "dynamic":  # the all-zero and the small token sit on the 2^-7 clamp
                assert float(xs[1]) == 2.0 ** -7 and float(xs[2]) == 2.0 ** -7
                assert not xq[1].any() and xq[2].any()
            else:
                assert int((xq[3].abs() == 127).sum()) >= 1
            wq, ws = torch.from_numpy(rec[f"wq_{tag}"]), bf16(rec[f"ws_{tag}"])
            y = O.linear(x, factor, act, wq, ws, bias)
            assert torch.equal(y, bf16(rec[f"y_ref_{tag}"])), tag
            if bias is not None:
                assert torch.equal(y[1], bias)


def test_the_fixture_shows_what_smoothquant_is_for():
    """Recorded y_ref against the float64 product on the two ordinary tokens: at alpha 0.5 the
    smoothed linear is closer than the conventional one (alpha None, a factor of ones)."""
    for name in FIXTURES:
        rec = load_golden(name)
        y64 = torch.from_numpy(rec["y64"])[[0, 4]]

        def err(tag):
            y = bf16(rec[f"y_ref_{tag}"])[[0, 4]].double()
            return float((y - y64).norm() / y64.norm())

        for mode in MODES:
            assert err(_tag(0.5, mode)) < err(_tag(None, mode)), (name, mode)


def test_ops_are_registered_with_fake_kernels():
    from torchao import ops

    for op in ("int8_smooth_quantize_per_token", "int8_smooth_quantize_static",
               "int8_smooth_dyn_linear", "int8_smooth_static_linear"):
        assert hasattr(torch.ops.torchao, op)
        assert op in ops.native_dispatch_smoothquant(), ops._native_error
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(3, 5, 64, dtype=torch.bfloat16)
        f = torch.empty(64, dtype=torch.bfloat16)
        a = torch.empty((), dtype=torch.bfloat16)
        w = torch.empty(24, 64, dtype=torch.int8)
        ws = torch.empty(24, dtype=torch.bfloat16)
        q, s = torch.ops.torchao.int8_smooth_quantize_per_token(x, f)
        assert q.shape == x.shape and q.dtype == torch.int8
        assert tuple(s.shape) == (15,) and s.dtype == torch.bfloat16
        q, s = torch.ops.torchao.int8_smooth_quantize_static(x, f, a)
        assert q.shape == x.shape and tuple(s.shape) == (15,)
        y = torch.ops.torchao.int8_smooth_dyn_linear(x, f, w, ws, None)
        assert tuple(y.shape) == (3, 5, 24) and y.dtype == torch.bfloat16
        y = torch.ops.torchao.int8_smooth_static_linear(x, f, a, w, ws, ws)
        assert tuple(y.shape) == (3, 5, 24)
        with pytest.raises(RuntimeError, match="K % 16"):
            torch.ops.torchao.int8_smooth_quantize_per_token(x[..., :40], f[:40])
