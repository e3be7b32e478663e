"""CPU tests of Int4WeightOnlyConfig(use_hqq=True): the plain-torch HQQ functions
(quantization/quant_primitives.py) and quantize_ on CPU linears against the reference's own
results bit for bit (tests/golden/hqq_*.npz, experiments/gen_golden_hqq.py), the refusals, the
checkpoint round trip, the op's schema and fake, and the harness's ``-q int4wo-<g>-hqq``."""

import io

import numpy as np
import pytest
import torch

from conftest import bf16, load_golden

from torchao.dtypes import AffineQuantizedTensor, TensorCoreTiledAQTTensorImpl
from torchao.quantization import Int4WeightOnlyConfig, quantize_
from torchao.quantization.quant_primitives import (
    HQQ_OPT_PARAMS,
    ZeroPointDomain,
    _choose_qparams_and_quantize_affine_hqq,
    _convert_to_affinequantized_format,
    _hqq_proximal_loop,
    _shrink_lp_op,
    optimize_weights_proximal_legacy,
)

FIXTURES = ["hqq_N64_K256_g32.npz", "hqq_N96_K1024_g64.npz", "hqq_N48_K512_g128.npz",
            "hqq_N40_K2048_g256.npz"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _linear(w):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
    return lin


@pytest.mark.parametrize("name", FIXTURES)
def test_quantize_on_cpu_equals_the_reference_bit_for_bit(name):
    rec = load_golden(name)
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    lin = _linear(bf16(rec["w"]))
    quantize_(lin, Int4WeightOnlyConfig(group_size=g, use_hqq=True))
    wt = lin.weight
    assert isinstance(wt, AffineQuantizedTensor)
    assert isinstance(wt.tensor_impl, TensorCoreTiledAQTTensorImpl)
    assert wt.shape == (N, K) and wt.block_size == (1, g) and wt.dtype == torch.bfloat16
    assert wt.zero_point_domain == ZeroPointDomain.FLOAT and (wt.quant_min, wt.quant_max) == (0, 15)
    q, s, z = wt.tensor_impl.get_plain()
    assert q.dtype == torch.int32 and s.dtype == z.dtype == torch.bfloat16
    assert np.array_equal(q.numpy().astype(np.uint8), rec["q"]), "codes differ"
    assert np.array_equal(_bits(s), rec["s"]), "scale bits differ"
    assert np.array_equal(_bits(z), rec["z"]), "zero bits differ"
    # and they are not the plain quantizer's
    assert not np.array_equal(rec["q"], rec["q_plain"])
    # dequantize() is the tinygemm form on those numbers (its bf16 op roundings: 2^-8 relative
    # on each of the product and the sum)
    deq = ((q.float() - 8).reshape(N, K // g, g) * s.float()[..., None]
           + z.float()[..., None]).reshape(N, K)
    bound = 2.0 ** -7 * float(((q.float() - 8).abs().reshape(N, K // g, g) * s.float()[..., None]
                               + z.float().abs()[..., None]).max())
    assert float((wt.dequantize().float() - deq).abs().max()) <= bound


@pytest.mark.parametrize("name", FIXTURES)
def test_error_trajectory_and_iterations_equal_the_reference(name):
    rec = load_golden(name)
    g = int(rec["g"])
    W = bf16(rec["w"]).float().reshape(-1, g)
    mn, mx = W.min(1, keepdim=True)[0], W.max(1, keepdim=True)[0]
    scale = (15 / (mx - mn)).clamp(max=2e4)
    zero = torch.round(-mn * scale)
    _, errors = _hqq_proximal_loop(W, scale, zero, [0, 15], 1, HQQ_OPT_PARAMS)
    assert len(errors) == int(rec["iters"])
    assert errors == rec["errors"].tolist()


def test_function_signatures_and_pieces():
    x = torch.tensor([-0.5, -1e-3, 0.0, 1e-3, 0.5])
    got = _shrink_lp_op(x, 10.0, 0.7)
    want = torch.sign(x) * torch.relu(x.abs() - 0.1 * x.abs().pow(-0.3))
    assert torch.equal(got, want) and got[2] == 0 and got[1] == 0 and got[4] > 0
    assert torch.equal(_shrink_lp_op(x, 10.0, 1), torch.sign(x) * torch.relu(x.abs() - 0.1))
    q, s, z = _convert_to_affinequantized_format(
        torch.arange(8.).reshape(4, 2), torch.tensor([[0.5]]), torch.tensor([[3.0]]), 4, (2, 4))
    assert q.shape == (2, 4) and float(z) == (8 - 3.0) * 0.5 and float(s) == 0.5
    # the solver alone: fp32 whatever the device default of the reference is
    W = torch.randn(4, 32, generator=torch.Generator().manual_seed(0))
    mn, mx = W.min(1, keepdim=True)[0], W.max(1, keepdim=True)[0]
    scale = 15 / (mx - mn)
    Wq, s2, z2 = optimize_weights_proximal_legacy(W, scale, torch.round(-mn * scale), [0, 15], axis=1)
    assert Wq.dtype == s2.dtype == z2.dtype == torch.float32 and torch.equal(s2, scale)
    assert float(Wq.min()) >= 0 and float(Wq.max()) <= 15
    with pytest.raises(NotImplementedError):
        _choose_qparams_and_quantize_affine_hqq(W, group_size=32, axis=0, device="cpu")
    with pytest.raises(NotImplementedError):
        _choose_qparams_and_quantize_affine_hqq(W, group_size=32, raw_output=True, device="cpu")


def test_edge_rows_equal_the_reference():
    rec = load_golden("hqq_quant_edges.npz")
    w = bf16(rec["w"])
    q, s, z, shape = _choose_qparams_and_quantize_affine_hqq(
        w, nbits=4, group_size=int(rec["g"]), axis=1, compute_dtype=torch.bfloat16, device="cpu")
    assert tuple(shape) == tuple(w.shape) and q.dtype == torch.uint8
    assert np.array_equal(q.numpy(), rec["q"])
    assert np.array_equal(_bits(s.reshape(5, 2)), rec["s"])
    assert np.array_equal(_bits(z.reshape(5, 2)), rec["z"])
    # the 2e4 clamp on the constant, the all-zero and the narrow group
    assert [float(v) for v in s.reshape(5, 2)[:3, 0]] == [float(torch.tensor(1 / 2e4).bfloat16())] * 3


def test_config_fields_and_defaults_are_unchanged():
    cfg = Int4WeightOnlyConfig()
    assert (cfg.group_size, cfg.use_hqq, cfg.zero_point_domain, cfg.set_inductor_config,
            cfg.preserve_zero, cfg.packing_format, cfg.version) == (
        128, False, ZeroPointDomain.NONE, True, None, "plain", 1)
    assert cfg.layout.inner_k_tiles == 8
    assert Int4WeightOnlyConfig(group_size=64, use_hqq=True).use_hqq is True
    assert "``use_hqq`` (unsupported" not in Int4WeightOnlyConfig.__doc__


def test_int_zero_domain_is_refused_before_the_module_is_touched():
    lin = torch.nn.Linear(64, 16, bias=False, dtype=torch.bfloat16)
    w = lin.weight
    with pytest.raises(AssertionError):
        quantize_(lin, Int4WeightOnlyConfig(group_size=32, use_hqq=True,
                                            zero_point_domain=ZeroPointDomain.INT))
    assert lin.weight is w and type(lin.weight) is torch.nn.Parameter
    # the reference's own assert in from_hp_to_intx
    from torchao.dtypes import to_affine_quantized_intx
    from torchao.quantization.quant_primitives import MappingType

    with pytest.raises(AssertionError, match="Invalid input parameters for HQQ"):
        to_affine_quantized_intx(w.detach(), MappingType.ASYMMETRIC, (1, 32), torch.int32, 0, 15,
                                 zero_point_domain=ZeroPointDomain.INT, _layout=cfg_layout(),
                                 use_hqq=True)


def cfg_layout():
    return Int4WeightOnlyConfig().layout


def test_incompatible_group_size_leaves_the_linear_alone():
    lin = torch.nn.Linear(96, 16, bias=False, dtype=torch.bfloat16)
    w = lin.weight.detach().clone()
    quantize_(lin, Int4WeightOnlyConfig(group_size=64, use_hqq=True))
    assert not isinstance(lin.weight, AffineQuantizedTensor) and torch.equal(lin.weight, w)


def test_state_dict_round_trips_through_weights_only_load():
    rec = load_golden(FIXTURES[0])
    lin = _linear(bf16(rec["w"]))
    quantize_(lin, Int4WeightOnlyConfig(group_size=32, use_hqq=True))
    buf = io.BytesIO()
    torch.save(lin.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    fresh = torch.nn.Linear(int(rec["K"]), int(rec["N"]), bias=False, dtype=torch.bfloat16)
    fresh.load_state_dict(sd, assign=True)
    a, b = lin.weight.tensor_impl, fresh.weight.tensor_impl
    assert isinstance(fresh.weight, AffineQuantizedTensor)
    assert torch.equal(a.packed_weight, b.packed_weight)
    assert torch.equal(a.scale_and_zero.view(torch.int16), b.scale_and_zero.view(torch.int16))


def test_op_has_a_schema_and_a_fake():
    op = torch.ops.torchao.int4_hqq_quantize_pack.default
    assert str(op._schema) == ("torchao::int4_hqq_quantize_pack(Tensor w, int group_size) -> "
                               "(Tensor, Tensor, Tensor)")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        for shape in ((40, 352), (2, 24, 256)):
            w = torch.empty(shape, dtype=torch.bfloat16)
            p, sz, it = torch.ops.torchao.int4_hqq_quantize_pack(w, 32)
            assert p.shape == (*shape[:-1], shape[-1] // 8) and p.dtype == torch.int32
            assert sz.shape == (*shape[:-1], shape[-1] // 32, 2) and sz.dtype == torch.bfloat16
            assert it.shape == (1,) and it.dtype == torch.int32
        with pytest.raises(RuntimeError, match="group_size"):
            torch.ops.torchao.int4_hqq_quantize_pack(torch.empty(8, 96, dtype=torch.bfloat16), 48)
        with pytest.raises(RuntimeError, match="divisible"):
            torch.ops.torchao.int4_hqq_quantize_pack(torch.empty(8, 96, dtype=torch.bfloat16), 64)


def test_generate_hqq_suffix_sets_use_hqq():
    from torchao._models.llama.generate import apply_quantization, build_model

    models = {}
    for q in ("int4wo-32-hqq", "int4wo-32", "cfg"):
        m = build_model("stories15M", torch.device("cpu"), seed=2)
        if q == "cfg":
            quantize_(m, Int4WeightOnlyConfig(group_size=32, use_hqq=True))
        else:
            apply_quantization(m, q)
        models[q] = m
    differs = 0
    for (n, a), (_, b), (_, c) in zip(*(models[k].named_parameters()
                                         for k in ("int4wo-32-hqq", "cfg", "int4wo-32"))):
        if not isinstance(a, AffineQuantizedTensor):
            continue
        assert isinstance(b, AffineQuantizedTensor) and isinstance(c, AffineQuantizedTensor), n
        assert torch.equal(a.tensor_impl.packed_weight, b.tensor_impl.packed_weight), n
        assert torch.equal(a.tensor_impl.scale_and_zero.view(torch.int16),
                           b.tensor_impl.scale_and_zero.view(torch.int16)), n
        differs += int(not torch.equal(a.tensor_impl.scale_and_zero.view(torch.int16),
                                       c.tensor_impl.scale_and_zero.view(torch.int16)))
    assert differs > 0
