"""CPU tests of the FP6 (e3m2 / e2m3) weight-only format against the reference fixtures
(tests/golden/fp6_*, written by experiments/gen_golden_fp6.py): the plain-torch quant primitives
and ``to_affine_quantized_fpx`` bit for bit, both storage conversions, the code tables, the
reference's checkpoint, the config's skip and refusal rules, the CPU linear and the route rule."""

import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, to_affine_quantized_fpx
from torchao.dtypes.floatx import (
    FloatxTensorCoreAQTTensorImpl,
    FloatxTensorCoreLayout,
    convert_from_floatx_tensor_core,
    convert_to_floatx_tensor_core,
)
from torchao.dtypes.floatx.floatx_tensor_core_layout import (
    pack_floatx_native,
    unpack_floatx_native,
)
from torchao.quantization import FPXWeightOnlyConfig, fpx_weight_only, quantize_
from torchao.quantization.quant_primitives import (
    _choose_qparams_affine_floatx,
    _dequantize_affine_floatx,
    _floatx_code_values,
    _floatx_max_normal,
    _quantize_affine_floatx,
)

FORMATS = {"e3m2": (3, 2), "e2m3": (2, 3)}
FIXTURES = golden_files("fp6_e")
CKPT = "fp6_refckpt_e3m2_N256_K64"


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def fmt_of(name):
    return FORMATS[name.split("_")[1]]


def native_ref(codes: np.ndarray) -> torch.Tensor:
    """Native storage of uint8 codes [N, K] from its definition, independent of the code under
    test: code k at bits 6 k .. 6 k + 5 of the row's little-endian bit stream, as int32."""
    N, K = codes.shape
    stream = np.zeros((N, K * 6), dtype=np.uint8)
    for b in range(6):
        stream[:, b::6] = (codes >> b) & 1
    by = np.packbits(stream, axis=1, bitorder="little")
    return torch.from_numpy(by.view(np.int32).copy())


def test_fixture_set():
    assert FIXTURES == sorted(f"fp6_{f}_N{n}_K{k}.npz" for f in FORMATS
                              for n, k in ((256, 64), (256, 320), (512, 192)))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_code_tables(fmt):
    """All 64 codes against the definition written out: OCP FP6, bias 3 / 1, max 28 / 7.5."""
    ebits, mbits = FORMATS[fmt]
    v = _floatx_code_values(ebits, mbits)
    assert v.shape == (64,) and v.dtype is torch.float32
    if fmt == "e3m2":
        pos = [0, 0.0625, 0.125, 0.1875] + [m * 2.0 ** e for e in range(-2, 5)
                                            for m in (1, 1.25, 1.5, 1.75)]
    else:
        pos = [m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** e for e in range(0, 3)
                                           for m in range(8)]
    assert len(pos) == 32
    assert v[:32].tolist() == pos
    assert v[32:].tolist() == [-p for p in pos]
    assert str(v[32].item()) == "-0.0"
    assert _floatx_max_normal(ebits, mbits) == {"e3m2": 28.0, "e2m3": 7.5}[fmt] == pos[-1]
    # every value is a bf16 number
    assert torch.equal(v.to(torch.bfloat16).float(), v)


@pytest.mark.parametrize("name", FIXTURES)
def test_primitives_match_reference(name):
    rec = load_golden(name)
    ebits, mbits = fmt_of(name)
    w = bf16(rec["w"])
    scale = _choose_qparams_affine_floatx(w, ebits, mbits)
    assert scale.dtype is torch.bfloat16 and np.array_equal(bits(scale), rec["scale"])
    codes = _quantize_affine_floatx(w, scale, ebits, mbits)
    assert codes.dtype is torch.uint8 and np.array_equal(codes.numpy(), rec["codes"])
    w_hat = _dequantize_affine_floatx(codes, scale, ebits, mbits, output_dtype=torch.bfloat16)
    assert np.array_equal(bits(w_hat), rec["w_hat"])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_quantizer_edges(fmt):
    """Ties, subnormals, saturation, the clamp and -0 (the rows are listed in the generator)."""
    rec = load_golden("fp6_quant_edges.npz")
    ebits, mbits = FORMATS[fmt]
    w = bf16(rec[f"{fmt}_w"])
    assert torch.isfinite(w.float()).all()
    t = to_affine_quantized_fpx(w, FloatxTensorCoreLayout(ebits, mbits))
    codes, scale = t.tensor_impl.get_plain()
    assert np.array_equal(bits(scale), rec[f"{fmt}_scale"])
    bad = np.argwhere(codes.numpy() != rec[f"{fmt}_codes"])
    assert bad.size == 0, f"first differing (row, col): {bad[:5].tolist()}"
    assert np.array_equal(bits(t.dequantize()), rec[f"{fmt}_w_hat"])
    # what the rows were built for
    mx = _floatx_max_normal(ebits, mbits)
    assert (codes[0] == 0).all()
    assert scale[0].item() == torch.tensor(1e-12 / mx).to(torch.bfloat16).item()
    assert scale[1].item() == 0.125 and scale[2].item() == 0.125 and scale[3].item() == 0.125
    assert (codes[12, :16] == 0x20).all()
    q = w.float() / scale.float().view(-1, 1)
    assert (q[4:12].abs().amax(1) > mx).all() and (codes[4:12, 0] == 0x1F).all()
    assert (codes[4:12, 1] == 0x3F).all()


@pytest.mark.parametrize("name", FIXTURES + ["fp6_quant_edges.npz"])
def test_storage_conversions(name):
    rec = load_golden(name)
    for fmt, (ebits, mbits) in FORMATS.items():
        pre = f"{fmt}_" if "edges" in name else ""
        if "edges" not in name and fmt_of(name) != (ebits, mbits):
            continue
        packed_ref = torch.from_numpy(rec[pre + "packed"])
        codes = rec[pre + "codes"]
        want = native_ref(codes)
        native = convert_from_floatx_tensor_core(packed_ref, ebits, mbits)
        assert native.dtype is torch.int32
        assert native.shape == (codes.shape[0], codes.shape[1] * 6 // 32)
        assert torch.equal(native, want)
        assert torch.equal(pack_floatx_native(torch.from_numpy(codes)), want)
        assert np.array_equal(unpack_floatx_native(want).numpy(), codes)
        back = convert_to_floatx_tensor_core(native, ebits, mbits)
        assert back.dtype is torch.uint8 and torch.equal(back, packed_ref)


def test_a_wide_code_stays_inside_its_field():
    """A NaN quotient's code is unspecified but six bits wide, and the packer masks: neither can
    change a neighbouring code."""
    codes = torch.randint(0, 64, (4, 64), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    wide = codes.clone()
    wide[:, 5::7] |= 0xC0
    assert torch.equal(pack_floatx_native(wide), pack_floatx_native(codes))
    x = torch.randn(2, 64)
    x[0, 9] = float("nan")
    x[1, 3] = float("inf")
    for ebits, mbits in FORMATS.values():
        q = _quantize_affine_floatx(x, torch.ones(2), ebits, mbits)
        assert int(q.max()) < 64
        clean = x.clone()
        clean[0, 9], clean[1, 3] = 0.0, 100.0
        qc = _quantize_affine_floatx(clean, torch.ones(2), ebits, mbits)
        keep = torch.ones_like(x, dtype=torch.bool)
        keep[0, 9] = False
        assert torch.equal(q[keep], qc[keep])  # +inf saturates like any value beyond the maximum


@pytest.mark.parametrize("name", FIXTURES)
def test_aqt_and_cpu_linear(name):
    rec = load_golden(name)
    ebits, mbits = fmt_of(name)
    w, x, bias = bf16(rec["w"]), bf16(rec["x"]), bf16(rec["bias"])
    t = to_affine_quantized_fpx(w, FloatxTensorCoreLayout(ebits, mbits))
    assert isinstance(t, AffineQuantizedTensor) and t.shape == w.shape and t.dtype is torch.bfloat16
    impl = t.tensor_impl
    assert isinstance(impl, FloatxTensorCoreAQTTensorImpl)
    assert impl.packed_floatx_data.dtype is torch.int32
    assert torch.equal(impl.packed_floatx_data, native_ref(rec["codes"]))
    assert impl.__tensor_flatten__() == (["packed_floatx_data", "scale"], [impl._layout])
    codes, scale = impl.get_plain()
    assert np.array_equal(codes.numpy(), rec["codes"]) and np.array_equal(bits(scale), rec["scale"])
    assert np.array_equal(bits(t.dequantize()), rec["w_hat"])
    # the CPU linear is F.linear on the dequantized weight: the reference's y_ref bit for bit
    y = F.linear(x, t, bias)
    assert y.dtype is torch.bfloat16 and np.array_equal(bits(y), rec["y_ref"])
    y3 = F.linear(x.reshape(1, 5, -1), t, bias)
    assert y3.shape == (1, 5, w.shape[0]) and np.array_equal(bits(y3[0]), rec["y_ref"])
    # an fp32 weight with fp32 activations takes the dispatch table's dequantize fallback
    t32 = to_affine_quantized_fpx(w.float(), FloatxTensorCoreLayout(ebits, mbits))
    assert t32.dtype is torch.float32 and t32.tensor_impl.scale.dtype is torch.float32
    assert np.array_equal(t32.tensor_impl.get_plain()[0].numpy(),
                          _quantize_affine_floatx(w.float(), t32.tensor_impl.scale, ebits,
                                                  mbits).numpy())
    y32 = F.linear(x.float(), t32, bias.float())
    assert y32.dtype is torch.float32
    assert torch.equal(y32, F.linear(x.float(), t32.dequantize(), bias.float()))
    # detach / clone / to keep the storage
    for u in (t.detach(), t.clone(), t.to("cpu")):
        assert torch.equal(u.tensor_impl.packed_floatx_data, impl.packed_floatx_data)
        assert torch.equal(u.tensor_impl.scale, impl.scale)


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    wt = sd["weight"]
    assert isinstance(wt, AffineQuantizedTensor)
    impl = wt.tensor_impl
    assert isinstance(impl, FloatxTensorCoreAQTTensorImpl)
    assert impl._layout == FloatxTensorCoreLayout(3, 2)
    # adopted into the native storage
    assert impl.packed_floatx_data.dtype is torch.int32
    assert torch.equal(impl.packed_floatx_data, native_ref(rec["codes"]))
    assert np.array_equal(impl.get_plain()[0].numpy(), rec["codes"])
    assert np.array_equal(bits(impl.scale), rec["scale"])
    assert np.array_equal(bits(wt.dequantize()), rec["w_hat"])
    m = torch.nn.Linear(64, 256, dtype=torch.bfloat16)
    m.load_state_dict(sd, assign=True)
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert torch.equal(m(x), F.linear(x, bf16(rec["w_hat"]), bf16(rec["bias"])))
    # and back: the reference's bytes
    assert np.array_equal(convert_to_floatx_tensor_core(impl.packed_floatx_data, 3, 2).numpy(),
                          rec["packed"])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_own_checkpoint_round_trips(fmt, tmp_path):
    ebits, mbits = FORMATS[fmt]
    torch.manual_seed(3)
    m = torch.nn.Linear(128, 256, dtype=torch.bfloat16)
    quantize_(m, fpx_weight_only(ebits, mbits))
    assert "FloatxTensorCoreLayout" in repr(m)
    path = str(tmp_path / "sd.pt")
    torch.save(m.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    a, b = m.weight.tensor_impl, sd["weight"].tensor_impl
    assert b.packed_floatx_data.dtype is torch.int32
    assert torch.equal(a.packed_floatx_data, b.packed_floatx_data) and torch.equal(a.scale, b.scale)
    m2 = torch.nn.Linear(128, 256, dtype=torch.bfloat16)
    m2.load_state_dict(sd, assign=True)
    x = torch.randn(2, 128).to(torch.bfloat16)
    assert torch.equal(m(x), m2(x))


def test_config_fields_and_alias():
    assert fpx_weight_only is FPXWeightOnlyConfig
    c = FPXWeightOnlyConfig(3, 2)
    assert (c.ebits, c.mbits, c.set_inductor_config) == (3, 2, True)
    assert FPXWeightOnlyConfig(ebits=2, mbits=3, set_inductor_config=False).mbits == 3
    lay = FloatxTensorCoreLayout(3, 2)
    with pytest.raises(Exception):
        lay.ebits = 2  # frozen


def test_quantize_skips_misfits(caplog):
    model = torch.nn.Sequential(
        torch.nn.Linear(64, 256), torch.nn.Linear(96, 256), torch.nn.Linear(64, 128),
    ).to(torch.bfloat16)
    with caplog.at_level(logging.INFO, logger="torchao.quantization.quant_api"):
        quantize_(model, fpx_weight_only(2, 3))
    assert isinstance(model[0].weight, AffineQuantizedTensor)
    assert type(model[1].weight) is torch.nn.Parameter and type(model[2].weight) is torch.nn.Parameter
    skipped = [r.getMessage() for r in caplog.records if "Skipping floatx" in r.getMessage()]
    assert len(skipped) == 2 and "in_dim=96" in skipped[0] and "out_dim=128" in skipped[1]


@pytest.mark.parametrize("pair", [(2, 2), (3, 1), (4, 3), (1, 4), (5, 2)])
def test_other_formats_refused_before_any_module_is_touched(pair):
    model = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.Linear(64, 256)).to(torch.bfloat16)
    before = [m.weight for m in model]
    with pytest.raises(NotImplementedError, match=r"\(3, 2\).*\(2, 3\)"):
        quantize_(model, fpx_weight_only(*pair))
    assert all(m.weight is w for m, w in zip(model, before))
    with pytest.raises(NotImplementedError, match=r"\(3, 2\) and \(2, 3\)"):
        to_affine_quantized_fpx(before[0].detach(), FloatxTensorCoreLayout(*pair))


def test_non_2d_weight_asserts():
    with pytest.raises(AssertionError, match="2-d"):
        to_affine_quantized_fpx(torch.zeros(2, 256, 64, dtype=torch.bfloat16),
                                FloatxTensorCoreLayout(3, 2))


def test_route_rule_and_tuning_hook():
    """csrc/fp6_host.h through the C ABI: GEMV up to the built-in boundary (at least one token, at
    most the 8 one launch serves), dequantize + matmul above; the hook forces a route and moves
    the boundary; N and K do not enter."""
    lib = _lib.lib()
    route = lib.tao_fp6_linear_route
    _lib.call("tao_tune_reset")
    boundary = max(m for m in range(0, 10) if m == 0 or route(m, 4096, 4096) == 1)
    assert 1 <= boundary <= 8
    for n, k in ((4096, 4096), (14336, 4096), (1, 64)):
        assert [route(m, n, k) for m in (1, boundary, boundary + 1, 512)] == [1, 1, 2, 2]
    try:
        _lib.call("tao_tune_fp6", 2, 0, 0, 0, 0, 0)
        assert route(1, 4096, 4096) == 2
        _lib.call("tao_tune_fp6", 1, 0, 0, 0, 0, 0)
        assert route(512, 4096, 4096) == 1
        _lib.call("tao_tune_fp6", 0, 2, 0, 0, 0, 0)
        assert [route(m, 256, 64) for m in (2, 3)] == [1, 2]
        for bad in ((3, 0, 0, 0, 0, 0), (0, -1, 0, 0, 0, 0), (0, 0, 3, 0, 0, 0),
                    (0, 0, 0, 4, 4, 0), (0, 0, 0, 0, 0, 3)):
            with pytest.raises(RuntimeError, match="tune: fp6"):
                _lib.call("tao_tune_fp6", *bad)
    finally:
        _lib.call("tao_tune_reset")
    assert route(boundary + 1, 4096, 4096) == 2
    from torchao.kernel.tuning import tuning

    with tuning(fp6=(2, 0, 0, 0, 0, 0)):
        assert route(1, 4096, 4096) == 2
    assert route(1, 4096, 4096) == 1
