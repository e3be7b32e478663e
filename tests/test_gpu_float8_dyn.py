"""GPU tests of the float8 dynamic-activation x float8-weight workflow against the reference
fixtures (tests/golden/float8dq_*.npz, written by tools/gen_golden_float8_dyn.py): the two ops
against the float64 formula on the reference's codes, the device quantisation byte for byte,
quantize_ end to end, graph capture, the argument errors, opcheck, and the vendor scaled mm."""

import pytest
import torch

from conftest import bf16, golden_files, load_golden
from exact_inputs_fp8 import rel_l2_finite, same_bf16, same_codes

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, Float8Layout, Float8MMConfig
from torchao.kernel import tuning
from torchao.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    LinearActivationQuantizedTensor,
    PerRow,
    quantize_,
)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FIXTURES = golden_files("float8dq_N")
BAR = 4e-3  # the project's bar against float64 on the same codes


def _u8(t):
    return t.view(torch.uint8)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _operands(rec):
    return (torch.from_numpy(rec["xq"]).view(FP8).to(DEV), torch.from_numpy(rec["xs"]).to(DEV),
            torch.from_numpy(rec["wq"]).view(FP8).to(DEV), torch.from_numpy(rec["ws"]).to(DEV),
            bf16(rec["bias"]).to(DEV))


def _check_nan_pattern(y, rec, M):
    zr, zt = int(rec["zero_row"]), int(rec["zero_token"])
    nan = y.isnan()
    want = torch.zeros_like(nan)
    if zr >= 0:
        want[:, zr] = True
    if 0 <= zt < M:
        want[zt] = True
    assert torch.equal(nan, want), "NaN exactly in the zero token's row and the zero row's column"


@pytest.mark.parametrize("route", ("built-in", "mfma", "gemv"))
@pytest.mark.parametrize("M", (1, 3, 5))
@pytest.mark.parametrize("fname", FIXTURES)
def test_ops_against_float64_on_the_reference_codes(fname, M, route):
    rec = load_golden(fname)
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"])[:M].to(DEV)
    y64 = torch.from_numpy(rec["y64"])[:M]
    knobs = {"built-in": {}, "mfma": {"fp8dyn_mfma": 1}, "gemv": {"linear_crossover": 8}}[route]
    with tuning(**knobs):
        y = torch.ops.torchao.fp8_scaled_mm(xq[:M], xs[:M], wq, ws, bias).cpu()
        k1 = _last_kernel()
        yd = torch.ops.torchao.fp8_dyn_linear(x, wq, ws, bias).cpu()
        y0 = torch.ops.torchao.fp8_scaled_mm(xq[:M], xs[:M], wq, ws, None).cpu()
    if route != "built-in":
        assert ("gemm_mfma" if route == "mfma" else "fp8dyn_gemv") in k1
    else:
        assert ("fp8dyn_gemv" if M <= 4 else "gemm_mfma") in k1, k1
    assert y.dtype == torch.bfloat16 and y.shape == (M, int(rec["N"]))
    _check_nan_pattern(y, rec, M)
    _check_nan_pattern(yd, rec, M)
    e, ed = rel_l2_finite(y, y64), rel_l2_finite(yd, y64)
    e0 = rel_l2_finite(y0, y64 - bf16(rec["bias"]).double())
    print(f"{fname} M={M} {route} {k1}: rel-L2 vs float64 scaled_mm {e:.3e} dyn_linear {ed:.3e} "
          f"no bias {e0:.3e}")
    assert e <= BAR and ed <= BAR and e0 <= BAR


@pytest.mark.parametrize("fname", FIXTURES)
def test_device_activation_quantisation_matches_the_reference(fname):
    """fp8_quantize_rows with rows = tokens gives the reference's activation codes and scales byte
    for byte (zero token: scale 0.0, NaN codes), and so does _input_activation_quant_func_fp8."""
    from torchao.quantization.quant_api import _input_activation_quant_func_fp8

    rec = load_golden(fname)
    x = bf16(rec["x"]).to(DEV)
    q, s = torch.ops.torchao.fp8_quantize_rows(x)
    assert same_codes(_u8(q).cpu(), torch.from_numpy(rec["xq"]))
    assert torch.equal(s.cpu().reshape(-1), torch.from_numpy(rec["xs"]))
    aqt = _input_activation_quant_func_fp8(x.view(1, 5, -1), PerRow(), FP8)
    assert isinstance(aqt, AffineQuantizedTensor) and aqt.shape == (1, 5, x.shape[1])
    assert _last_kernel() == "fp8_quantize_rows_kernel"
    assert same_codes(_u8(aqt.tensor_impl.float8_data).cpu().view(5, -1), torch.from_numpy(rec["xq"]))
    assert torch.equal(aqt.tensor_impl.scale.cpu().reshape(-1), torch.from_numpy(rec["xs"]))
    zt = int(rec["zero_token"])
    if zt >= 0:
        assert float(s[zt]) == 0.0 and bool(((_u8(q)[zt] & 0x7F) == 0x7F).all())


def _mlp(K, H, N, bias):
    gen = torch.Generator().manual_seed(K + N)
    m = torch.nn.Sequential(torch.nn.Linear(K, H, bias=bias), torch.nn.Linear(H, N, bias=bias))
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 2 else 0.1))
    return m.to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("bias", (True, False))
def test_quantize_end_to_end_equals_the_ops(bias):
    K, H, N = 256, 96, 64
    m = _mlp(K, H, N, bias)
    quantize_(m, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
    for lin in m:
        w = lin.weight
        assert isinstance(w, LinearActivationQuantizedTensor)
        inner = w.original_weight_tensor
        assert isinstance(inner, AffineQuantizedTensor) and inner.device.type == "cuda"
        assert inner._layout == Float8Layout(mm_config=Float8MMConfig(use_fast_accum=True))
    gen = torch.Generator().manual_seed(3)

    def by_ops(x2, one_launch):
        h = x2
        for lin in m:
            impl = lin.weight.original_weight_tensor.tensor_impl
            wq, ws = impl.float8_data, impl.scale.reshape(-1)
            if one_launch:
                h = torch.ops.torchao.fp8_dyn_linear(h, wq, ws, lin.bias)
            else:
                q, s = torch.ops.torchao.fp8_quantize_rows(h)
                h = torch.ops.torchao.fp8_scaled_mm(q, s, wq, ws, lin.bias)
        return h

    for shape in ((1, K), (3, K), (40, K), (1, 1, K), (2, 20, K)):
        x = torch.randn(*shape, generator=gen).to(torch.bfloat16).to(DEV)
        with torch.no_grad():
            y = m(x)
        M = x.numel() // K
        assert y.shape == (*shape[:-1], N)
        assert torch.equal(y.reshape(M, N), by_ops(x.reshape(M, K), False))
        assert torch.equal(y.reshape(M, N), by_ops(x.reshape(M, K), True))
        if M == 1:  # the eager one-token path is the single launch
            assert _last_kernel() == "fp8dyn_gemv_kernel"
    # empty batch
    with torch.no_grad():
        assert m[0](torch.zeros(0, K, dtype=torch.bfloat16, device=DEV)).numel() == 0
    # fp32 activations: loud
    with pytest.raises((AssertionError, RuntimeError)):
        m(torch.randn(2, K, device=DEV))


def test_one_token_fast_path_skips_the_activation_tensor():
    from torchao.quantization.linear_activation_quantized_tensor import _fused_fp8_dyn_decode

    m = _mlp(256, 96, 64, True)
    quantize_(m, Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()))
    lin = m[0]
    for shape in ((1, 256), (1, 1, 256)):
        x = torch.randn(*shape, dtype=torch.bfloat16, device=DEV)
        assert _fused_fp8_dyn_decode(x, lin.weight, lin.bias) is not None
        w = lin.weight
        ref = torch.nn.functional.linear(w.input_quant_func(x, **w.quant_kwargs),
                                         w.original_weight_tensor, lin.bias)
        assert torch.equal(lin(x), ref)
    assert _fused_fp8_dyn_decode(torch.randn(4, 256, dtype=torch.bfloat16, device=DEV),
                                 lin.weight, None) is None


def test_graph_capture_replay_equals_eager():
    rec = load_golden("float8dq_N96_K1024.npz")
    _, _, wq, ws, bias = _operands(rec)
    gen = torch.Generator().manual_seed(5)
    x1 = torch.randn(1, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    x32 = torch.randn(32, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    op = torch.ops.torchao.fp8_dyn_linear
    e1, e32 = op(x1, wq, ws, bias), op(x32, wq, ws, None)
    assert _last_kernel() == "gemm_mfma_kernel"
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g1 = op(x1, wq, ws, bias)
        g32 = op(x32, wq, ws, None)
    g1.zero_()
    g32.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, e1) and torch.equal(g32, e32)
    x1.copy_(torch.randn(1, 1024, generator=gen).to(torch.bfloat16))
    x32.copy_(torch.randn(32, 1024, generator=gen).to(torch.bfloat16))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, op(x1, wq, ws, bias)) and torch.equal(g32, op(x32, wq, ws, None))


def test_argument_errors():
    rec = load_golden("float8dq_N64_K256.npz")
    xq, xs, wq, ws, bias = _operands(rec)
    mm, dyn = torch.ops.torchao.fp8_scaled_mm, torch.ops.torchao.fp8_dyn_linear
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        mm(xq.view(torch.uint8), xs, wq, ws, None)
    with pytest.raises(RuntimeError, match="2D float8_e4m3fn"):
        mm(xq, xs, wq.view(torch.uint8), ws, None)
    with pytest.raises(RuntimeError, match="last dim"):
        mm(xq[:, :128], xs, wq, ws, None)
    with pytest.raises(RuntimeError, match="one entry per row"):
        mm(xq, xs[:3], wq, ws, None)
    with pytest.raises(RuntimeError, match="N elements"):
        mm(xq, xs, wq, ws[:5], None)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        mm(xq[:, :40].contiguous(), xs, wq[:, :40].contiguous(), ws, None)
    with pytest.raises(RuntimeError, match="same device"):
        mm(xq, xs.cpu(), wq, ws, None)
    with pytest.raises(RuntimeError, match="bf16"):
        dyn(torch.zeros(2, 256, device=DEV), wq, ws, None)
    with pytest.raises(RuntimeError, match="last dim"):
        dyn(torch.zeros(2, 128, dtype=torch.bfloat16, device=DEV), wq, ws, None)
    # the C entry of the fused launch is one token
    x = torch.zeros(2, 256, dtype=torch.bfloat16, device=DEV)
    y = torch.empty(2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="one token"):
        _lib.call("tao_fp8_dyn_linear_bf16", x.data_ptr(), wq.data_ptr(), ws.data_ptr(), None,
                  y.data_ptr(), 2, 64, 256, None)
    # empty batch through the op
    assert mm(xq[:0], xs[:0], wq, ws, bias).shape == (0, 64)
    assert dyn(torch.zeros(0, 256, dtype=torch.bfloat16, device=DEV), wq, ws, bias).shape == (0, 64)


@pytest.mark.parametrize("name", ["fp8_scaled_mm", "fp8_dyn_linear"])
def test_opcheck(name):
    """As tests/test_gpu_float8.py::test_opcheck: both ops take float8 inputs, for which opcheck's
    schema test cannot run (torch.allclose is not implemented for float8), so the other three
    tests run and input mutation / output aliasing are checked by hand."""
    gen = torch.Generator().manual_seed(9)
    N, K = 256, 512
    w = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16).to(DEV)
    q, s = torch.ops.torchao.fp8_quantize_rows(w)
    x = torch.randn(3, K, generator=gen).to(torch.bfloat16).to(DEV)
    xq, xsc = torch.ops.torchao.fp8_quantize_rows(x)
    bias = torch.randn(N, generator=gen).to(torch.bfloat16).to(DEV)
    args = {"fp8_scaled_mm": (xq, xsc, q, s.reshape(-1), bias),
            "fp8_dyn_linear": (x, q, s.reshape(-1), bias)}[name]
    op = getattr(torch.ops.torchao, name).default
    torch.library.opcheck(op, args, test_utils=("test_faketensor", "test_aot_dispatch_dynamic",
                                                "test_autograd_registration"))
    before = [a.clone() for a in args]
    out = op(*args)
    torch.cuda.synchronize()
    for a, b in zip(args, before):
        assert torch.equal(a.view(torch.uint8) if a.dtype == FP8 else a,
                           b.view(torch.uint8) if b.dtype == FP8 else b)
        assert out.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()


@pytest.mark.parametrize("fname", FIXTURES)
def test_against_the_vendor_scaled_mm(fname):
    """torch._scaled_mm with row-wise scales, where this build runs it on the device. The bar is
    twice the worse of the two implementations' own distances to the float64 formula (different
    summation orders on the same codes). Measured on the MI355X: see DESIGN.md §4.10."""
    rec = load_golden(fname)
    xq, xs, wq, ws, bias = _operands(rec)
    try:
        yv = torch._scaled_mm(xq, wq.t(), scale_a=xs.view(-1, 1), scale_b=ws.view(1, -1),
                              bias=bias, out_dtype=torch.bfloat16, use_fast_accum=True).cpu()
    except (RuntimeError, NotImplementedError, ValueError) as e:
        pytest.skip(f"torch._scaled_mm with row-wise scales does not run here: {str(e)[:120]}")
    y = torch.ops.torchao.fp8_scaled_mm(xq, xs, wq, ws, bias).cpu()
    y64 = torch.from_numpy(rec["y64"])
    ok = ~y64.isnan()  # (what the vendor kernel writes where the formula is NaN is its own affair)
    e_own = rel_l2_finite(y, y64)
    e_vendor = float(torch.linalg.norm((yv.double() - y64)[ok]) / torch.linalg.norm(y64[ok]))
    d = float(torch.linalg.norm((y.double() - yv.double())[ok]) / torch.linalg.norm(y64[ok]))
    print(f"{fname}: rel-L2 to float64 own {e_own:.3e} vendor {e_vendor:.3e}; own vs vendor {d:.3e}")
    assert d <= 2 * max(e_own, e_vendor)
