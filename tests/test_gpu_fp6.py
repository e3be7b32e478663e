"""GPU tests of the FP6 (e3m2 / e2m3) weight-only linear against the reference fixtures
(tests/golden/fp6_*): the HIP quantizer, dequantizer and both storage conversions bit for bit, the
linear through ``quantize_`` + ``nn.Linear`` and through the op on both routes within the
project's float8 bars (tests/test_gpu_float8.py: 4e-3 against float64, 1e-2 against the
reference's own output), Llama shapes on the GEMV, tensor plumbing, argument errors and opcheck of
the three ops. The fixtures hold no inf or NaN row; such rows are outside the bit-exactness
claim."""

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
from torchao.dtypes.floatx.floatx_tensor_core_layout import unpack_floatx_native
from torchao.kernel.tuning import tuning
from torchao.quantization import fpx_weight_only, quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
FORMATS = {"e3m2": (3, 2), "e2m3": (2, 3)}
FIXTURES = golden_files("fp6_e")
BAR64, BAR_REF = 4e-3, 1e-2
MS = (1, 2, 4, 5, 8)
ROUTES = ((1, "fp6wo_gemv_kernel"), (2, "fp6_dequant_kernel"))


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def fmt_of(name):
    return FORMATS[name.split("_")[1]]


def rel_l2(y, ref):
    y, ref = y.detach(), ref.detach()
    return float(torch.linalg.norm(y.double() - ref.double()) / torch.linalg.norm(ref.double()))


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _rows(t, M):
    """M rows out of the fixture's 5 (rows wrap around beyond them)."""
    return t[torch.arange(M) % t.shape[0]]


def _weight(rec, ebits, mbits):
    """The fixture's weight on the device, from its codes (no quantizer involved)."""
    lay = FloatxTensorCoreLayout(ebits, mbits)
    impl = FloatxTensorCoreAQTTensorImpl.from_plain(torch.from_numpy(rec["codes"]),
                                                    bf16(rec["scale"]), None, lay)
    N, K = rec["codes"].shape
    return AffineQuantizedTensor(impl, [N, 1], (N, K), dtype=torch.bfloat16).to(DEV)


def test_fixture_set():
    assert len(FIXTURES) == 6


@pytest.mark.parametrize("name", FIXTURES)
def test_device_quantizer_and_dequantizer_equal_the_fixture(name):
    rec = load_golden(name)
    ebits, mbits = fmt_of(name)
    w = bf16(rec["w"]).to(DEV)
    packed, scale = T.fp6_quantize_rows(w, ebits, mbits)
    assert _last_kernel() == "fp6_quantize_rows_kernel"
    assert packed.dtype is torch.int32 and packed.shape == (w.shape[0], w.shape[1] * 6 // 32)
    assert scale.dtype is torch.bfloat16 and np.array_equal(bits(scale.cpu()), rec["scale"])
    assert np.array_equal(unpack_floatx_native(packed.cpu()).numpy(), rec["codes"])
    t = to_affine_quantized_fpx(w, FloatxTensorCoreLayout(ebits, mbits))
    assert _last_kernel() == "fp6_quantize_rows_kernel"
    assert torch.equal(t.tensor_impl.packed_floatx_data, packed)
    for w_hat in (T.fp6_dequantize(packed, scale, ebits, mbits), t.dequantize()):
        assert _last_kernel() == "fp6_dequant_kernel"
        assert w_hat.is_cuda and np.array_equal(bits(w_hat.cpu()), rec["w_hat"])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_device_quantizer_edges(fmt):
    """Ties, subnormals, saturation, the 1e-12 clamp and -0, every code and scale."""
    rec = load_golden("fp6_quant_edges.npz")
    ebits, mbits = FORMATS[fmt]
    w = bf16(rec[f"{fmt}_w"])
    assert torch.isfinite(w.float()).all()
    packed, scale = T.fp6_quantize_rows(w.to(DEV), ebits, mbits)
    assert np.array_equal(bits(scale.cpu()), rec[f"{fmt}_scale"])
    bad = np.argwhere(unpack_floatx_native(packed.cpu()).numpy() != rec[f"{fmt}_codes"])
    assert bad.size == 0, f"first differing (row, col): {bad[:5].tolist()}"
    w_hat = T.fp6_dequantize(packed, scale, ebits, mbits)
    assert np.array_equal(bits(w_hat.cpu()), rec[f"{fmt}_w_hat"])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_nan_weight_leaves_the_rest_of_its_row_alone(fmt):
    """Outside the bit-exactness claim, but contained: the HIP quantizer keeps a NaN out of the row
    maximum and inside its own six-bit field, so the scale and every other code of the row are
    those of the row with a zero in its place."""
    ebits, mbits = FORMATS[fmt]
    w = bf16(load_golden("fp6_quant_edges.npz")[f"{fmt}_w"]).clone()
    clean = w.clone()
    spots = [(5, 0), (5, 37), (20, 255), (33, 128)]
    for r, c in spots:
        w[r, c], clean[r, c] = float("nan"), 0.0
    p, s = T.fp6_quantize_rows(w.to(DEV), ebits, mbits)
    pc, sc = T.fp6_quantize_rows(clean.to(DEV), ebits, mbits)
    assert torch.equal(s, sc)
    q, qc = unpack_floatx_native(p.cpu()), unpack_floatx_native(pc.cpu())
    keep = torch.ones_like(q, dtype=torch.bool)
    for r, c in spots:
        keep[r, c] = False
    assert torch.equal(q[keep], qc[keep])


@pytest.mark.parametrize("name", FIXTURES)
def test_device_conversions(name):
    rec = load_golden(name)
    ebits, mbits = fmt_of(name)
    ref_bytes = torch.from_numpy(rec["packed"]).to(DEV)
    native = convert_from_floatx_tensor_core(ref_bytes, ebits, mbits)
    assert native.is_cuda and native.dtype is torch.int32
    assert np.array_equal(unpack_floatx_native(native.cpu()).numpy(), rec["codes"])
    back = convert_to_floatx_tensor_core(native, ebits, mbits)
    assert back.is_cuda and torch.equal(back, ref_bytes)


@pytest.mark.parametrize("route,kernel", ROUTES)
@pytest.mark.parametrize("name", FIXTURES)
def test_linear_meets_the_bars(name, route, kernel):
    """Through quantize_ + nn.Linear and through the op, with and without the bias."""
    rec = load_golden(name)
    ebits, mbits = fmt_of(name)
    N, K = rec["w"].shape
    m = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(bf16(rec["w"]))
        m.bias.copy_(bf16(rec["bias"]))
    m = m.to(DEV)
    quantize_(m, fpx_weight_only(ebits, mbits))
    impl = m.weight.tensor_impl
    assert np.array_equal(impl.get_plain()[0].cpu().numpy(), rec["codes"])
    y64_all, yref_all = torch.from_numpy(rec["y64"]), bf16(rec["y_ref"])
    nobias64 = y64_all - bf16(rec["bias"]).double()
    with tuning(fp6=(route, 0, 0, 0, 0, 0)):
        for M in MS:
            x = _rows(bf16(rec["x"]), M).to(DEV)
            y64, y_ref = _rows(y64_all, M), _rows(yref_all, M)
            y = m(x)
            assert _last_kernel() == kernel
            yo = T.fp6_weight_only_linear(x, impl.packed_floatx_data, impl.scale, ebits, mbits,
                                          m.bias)
            assert _last_kernel() == kernel
            assert y.dtype is torch.bfloat16 and y.shape == (M, N) and torch.equal(y, yo)
            e64, eref = rel_l2(y.cpu(), y64), rel_l2(y.cpu(), y_ref)
            print(f"{name} route {route} M={M}: rel_l2 vs y64 {e64:.3e}, vs y_ref {eref:.3e}")
            assert e64 <= BAR64, (name, route, M, e64)
            assert eref <= BAR_REF, (name, route, M, eref)
            yn = T.fp6_weight_only_linear(x, impl.packed_floatx_data, impl.scale, ebits, mbits)
            assert rel_l2(yn.cpu(), _rows(nobias64, M)) <= BAR64


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_llama_shapes_run_the_gemv(fmt):
    """quantize_ on bf16 linears of the four Llama-3-8B shapes: every one runs fp6wo_gemv_kernel
    up to the built-in boundary and the dequantizer above it."""
    ebits, mbits = FORMATS[fmt]
    boundary = max(mm for mm in range(1, 10) if _lib.lib().tao_fp6_linear_route(mm, 4096, 4096) == 1)
    torch.manual_seed(0)
    for N, K in ((4096, 4096), (6144, 4096), (14336, 4096), (4096, 14336)):
        m = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device=DEV)
        quantize_(m, fpx_weight_only(ebits, mbits))
        assert isinstance(m.weight, AffineQuantizedTensor)
        w_hat = m.weight.dequantize()
        for M in (1, boundary):
            x = torch.randn(M, K, dtype=torch.bfloat16, device=DEV)
            y = m(x)
            assert _last_kernel() == "fp6wo_gemv_kernel", (N, K, M, _last_kernel())
            assert rel_l2(y, x.double() @ w_hat.double().t()) <= BAR64
        m(torch.randn(boundary + 1, K, dtype=torch.bfloat16, device=DEV))
        assert _last_kernel() == "fp6_dequant_kernel"


def test_3d_input_empty_batch_and_fp16_fallback():
    rec = load_golden("fp6_e2m3_N256_K320.npz")
    wt = _weight(rec, 2, 3)
    x, bias = bf16(rec["x"]).to(DEV), bf16(rec["bias"]).to(DEV)
    y = F.linear(x, wt, bias)
    y3 = F.linear(x.reshape(5, 1, 320), wt, bias)
    assert y3.shape == (5, 1, 256) and torch.equal(y3.reshape(5, 256), y)
    y3 = F.linear(x[:4].reshape(2, 2, 320), wt, bias)
    assert y3.shape == (2, 2, 256) and torch.equal(y3.reshape(4, 256), F.linear(x[:4], wt, bias))
    ye = F.linear(x[:0], wt, bias)
    assert ye.shape == (0, 256) and ye.dtype is torch.bfloat16
    assert F.linear(x[:0].reshape(0, 3, 320), wt).shape == (0, 3, 256)
    # an fp16 model: quantized by the torch-op formulation, its linear is the dequantize fallback
    m = torch.nn.Linear(320, 256, dtype=torch.float16, device=DEV)
    w16 = m.weight.detach().clone()
    quantize_(m, fpx_weight_only(2, 3))
    assert m.weight.dtype is torch.float16 and m.weight.tensor_impl.scale.dtype is torch.float16
    x16 = torch.randn(3, 320, dtype=torch.float16, device=DEV)
    _lib.call("tao_tune_reset")
    y16 = m(x16)
    assert y16.dtype is torch.float16
    assert torch.equal(y16, F.linear(x16, m.weight.dequantize(), m.bias))
    assert rel_l2(y16, F.linear(x16, w16, m.bias)) < 0.05  # e2m3 quantization error ~ 0.03


def test_device_moves_and_reference_checkpoint():
    rec = load_golden("fp6_refckpt_e3m2_N256_K64.npz")
    sd = torch.load(os.path.join(GOLDEN, "fp6_refckpt_e3m2_N256_K64.pt"), weights_only=True)
    m = torch.nn.Linear(64, 256, dtype=torch.bfloat16)
    m.load_state_dict(sd, assign=True)
    m = m.to(DEV)
    impl = m.weight.tensor_impl
    assert impl.packed_floatx_data.is_cuda and impl.packed_floatx_data.dtype is torch.int32
    assert np.array_equal(impl.get_plain()[0].cpu().numpy(), rec["codes"])
    assert np.array_equal(bits(m.weight.dequantize().cpu()), rec["w_hat"])
    x = torch.randn(2, 64, dtype=torch.bfloat16, device=DEV)
    y = m(x)
    assert _last_kernel() == "fp6wo_gemv_kernel"
    ref = x.double() @ bf16(rec["w_hat"]).to(DEV).double().t() + bf16(rec["bias"]).to(DEV).double()
    assert rel_l2(y, ref) <= BAR64
    back = m.weight.cpu()
    assert np.array_equal(back.tensor_impl.get_plain()[0].numpy(), rec["codes"])
    # the device quantizer on the checkpoint's original weight gives the checkpoint's codes
    t = to_affine_quantized_fpx(bf16(rec["w"]).to(DEV), FloatxTensorCoreLayout(3, 2))
    assert torch.equal(t.tensor_impl.packed_floatx_data, impl.packed_floatx_data)


def test_argument_errors():
    rec = load_golden("fp6_e3m2_N256_K64.npz")
    wt = _weight(rec, 3, 2)
    codes, scale = wt.tensor_impl.packed_floatx_data, wt.tensor_impl.scale
    x = bf16(rec["x"]).to(DEV)
    with pytest.raises(RuntimeError, match="needs bf16 x"):
        T.fp6_weight_only_linear(x.float(), codes, scale, 3, 2, None)
    with pytest.raises(RuntimeError, match="codes must be a 2D int32"):
        T.fp6_weight_only_linear(x, codes.view(torch.uint8), scale, 3, 2, None)
    with pytest.raises(RuntimeError, match="codes must be a 2D int32"):
        T.fp6_weight_only_linear(x, codes.reshape(-1), scale, 3, 2, None)
    with pytest.raises(RuntimeError, match="whole 32-code groups"):
        T.fp6_weight_only_linear(x, codes[:, :10].contiguous(), scale, 3, 2, None)
    with pytest.raises(RuntimeError, match=r"K \(32\) must be a positive multiple of 64"):
        T.fp6_weight_only_linear(x[:, :32].contiguous(), codes[:, :6].contiguous(), scale, 3, 2,
                                 None)
    with pytest.raises(RuntimeError, match=r"K \(96\) must be a positive multiple of 64"):
        T.fp6_weight_only_linear(torch.zeros(1, 96, dtype=torch.bfloat16, device=DEV),
                                 torch.zeros(256, 18, dtype=torch.int32, device=DEV), scale, 3, 2,
                                 None)
    with pytest.raises(RuntimeError, match="x last dim 32 != K 64"):
        T.fp6_weight_only_linear(x[:, :32].contiguous(), codes, scale, 3, 2, None)
    with pytest.raises(RuntimeError, match="scale must have N = 256"):
        T.fp6_weight_only_linear(x, codes, scale[:8], 3, 2, None)
    with pytest.raises(RuntimeError, match="bias must have N = 256"):
        T.fp6_weight_only_linear(x, codes, scale, 3, 2, scale[:8])
    with pytest.raises(RuntimeError, match=r"\(2, 2\) is not served; served: \(3, 2\) and \(2, 3\)"):
        T.fp6_weight_only_linear(x, codes, scale, 2, 2, None)
    with pytest.raises(RuntimeError, match="is not served"):
        T.fp6_quantize_rows(bf16(rec["w"]).to(DEV), 3, 1)
    with pytest.raises(RuntimeError, match=r"K \(48\) must be a multiple of 32"):
        T.fp6_quantize_rows(torch.zeros(4, 48, dtype=torch.bfloat16, device=DEV), 3, 2)
    with pytest.raises(RuntimeError, match="needs a bf16 weight"):
        T.fp6_quantize_rows(bf16(rec["w"]).to(DEV).float(), 3, 2)
    with pytest.raises(RuntimeError, match="needs a bf16 scale"):
        T.fp6_dequantize(codes, scale.float(), 3, 2)
    # the C ABI refuses what the op checks before it
    lib = _lib.lib()
    rc = lib.tao_fp6_linear_bf16(None, None, None, None, None, 1, 8, 96, 3, 2, None)
    assert rc != 0 and "K (96) must be a multiple of 64" in lib.tao_last_error().decode()
    rc = lib.tao_fp6_linear_bf16(None, None, None, None, None, 1, 8, 64, 2, 2, None)
    assert rc != 0 and "is not served" in lib.tao_last_error().decode()
    # any N >= 1 with K % 64 == 0 is served by the op; the N % 256 rule is the config's alone
    y = T.fp6_weight_only_linear(x, codes[:3].contiguous(), scale[:3].contiguous(), 3, 2, None)
    assert y.shape == (5, 3)
    assert torch.equal(y, T.fp6_weight_only_linear(x, codes, scale, 3, 2, None)[:, :3])


@pytest.mark.parametrize("name", ["fp6_quantize_rows", "fp6_dequantize", "fp6_weight_only_linear"])
def test_opcheck(name):
    rec = load_golden("fp6_e3m2_N256_K64.npz")
    wt = _weight(rec, 3, 2)
    codes, scale = wt.tensor_impl.packed_floatx_data, wt.tensor_impl.scale
    args = {
        "fp6_quantize_rows": (bf16(rec["w"]).to(DEV), 3, 2),
        "fp6_dequantize": (codes, scale, 3, 2),
        "fp6_weight_only_linear": (bf16(rec["x"])[:3].to(DEV), codes, scale, 3, 2,
                                   bf16(rec["bias"]).to(DEV)),
    }[name]
    torch.library.opcheck(getattr(T, name).default, args)
