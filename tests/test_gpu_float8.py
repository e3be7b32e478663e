"""GPU tests of the float8 (e4m3fn) weight-only workflow against the reference fixtures
(tests/golden/float8wo_*.npz, written by tools/gen_golden_float8.py): the fused quantizer and
the dequantizer byte for byte, the linear on both routes within the project's bars, quantize_
end to end, graph capture, and opcheck of the three ops."""

import pytest
import torch

from conftest import bf16, golden_files, load_golden
from exact_inputs_fp8 import rel_l2_finite, same_bf16, same_codes

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, Float8AQTTensorImpl
from torchao.quantization import Float8WeightOnlyConfig, quantize_
from torchao.quantization.quant_primitives import (
    _choose_scale_float8,
    _dequantize_affine_float8,
    _quantize_affine_float8,
)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FIXTURES = golden_files("float8wo_N")


def _u8(t):
    return t.view(torch.uint8)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_rows_matches_fixture_and_torch_ops(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    w = bf16(rec["w"]).to(DEV)
    q, s = torch.ops.torchao.fp8_quantize_rows(w)
    assert _last_kernel() == "fp8_quantize_rows_kernel"
    assert q.dtype == FP8 and q.shape == (N, K) and s.dtype == torch.float32 and s.shape == (N, 1)
    assert torch.equal(s.cpu().reshape(-1), torch.from_numpy(rec["s"]))
    assert same_codes(_u8(q).cpu(), torch.from_numpy(rec["q"]))
    # the torch-op formulation on the same device
    s_t = _choose_scale_float8(w, block_size=(1, K), float8_dtype=FP8)
    q_t = _quantize_affine_float8(w, s_t, FP8)
    assert torch.equal(s, s_t)
    assert same_codes(_u8(q).cpu(), _u8(q_t).cpu())
    zr = int(rec["zero_row"])
    if zr >= 0:
        assert float(s[zr]) == 0.0 and bool(((_u8(q)[zr] & 0x7F) == 0x7F).all())


def test_quantize_rows_cast_sweep():
    """Rows that contain 448 (so the scale is exactly 1) followed by every finite bf16 pattern
    with |v| <= 448: the codes must be what the CPU cast float -> float8_e4m3fn gives, ties,
    subnormals and the saturation edge included."""
    pos = torch.arange(0, 0x43E0 + 1, dtype=torch.int32)  # +0 .. +448
    pat = torch.cat([pos, pos | 0x8000]).to(torch.int16).view(torch.bfloat16)
    assert float(pat.float().abs().max()) == 448.0 and bool(pat.float().isfinite().all())
    per = 1016
    pad = (-pat.numel()) % per
    body = torch.cat([pat, torch.zeros(pad, dtype=torch.bfloat16)]).view(-1, per)
    head = torch.zeros(body.shape[0], 8, dtype=torch.bfloat16)
    head[:, 0] = 448.0
    w = torch.cat([head, body], 1).contiguous()
    q, s = torch.ops.torchao.fp8_quantize_rows(w.to(DEV))
    assert bool((s.cpu() == 1.0).all())
    want = _u8(w.float().to(FP8))
    got = _u8(q).cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, [(float(w[r, c]), int(got[r, c]), int(want[r, c])) for r, c in bad[:8]]


def test_dequantize_all_codes():
    codes = torch.arange(256, dtype=torch.uint8).repeat(3, 1)
    scale = torch.tensor([1.0, 0.013671875, 3.3e-3], dtype=torch.float32)
    want = (codes.view(FP8).float() * scale.view(3, 1)).to(torch.bfloat16)
    got = torch.ops.torchao.fp8_dequantize(codes.view(FP8).to(DEV), scale.to(DEV)).cpu()
    assert _last_kernel() == "fp8_dequant_kernel"
    assert got.dtype == torch.bfloat16 and same_bf16(got, want)
    assert bool(got[:, [0x7F, 0xFF]].isnan().all()) and int(got.isnan().sum()) == 6
    # and the torch-op formulation on the device
    dq_t = _dequantize_affine_float8(codes.view(FP8).to(DEV), scale.view(3, 1).to(DEV),
                                     torch.bfloat16).cpu()
    assert same_bf16(got, dq_t)


@pytest.mark.parametrize("fname", FIXTURES)
def test_dequantize_matches_fixture(fname):
    rec = load_golden(fname)
    q = torch.from_numpy(rec["q"]).view(FP8).to(DEV)
    s = torch.from_numpy(rec["s"]).to(DEV)
    assert same_bf16(torch.ops.torchao.fp8_dequantize(q, s).cpu(), bf16(rec["w_dequant"]))


@pytest.mark.parametrize("M", (1, 3, 5))
@pytest.mark.parametrize("fname", FIXTURES)
def test_linear_against_float64_and_reference(fname, M):
    """Built-in routing: the GEMV up to M = 4 at these weight sizes, the MFMA kernel at M = 5
    (asserted). Bars: rel-L2 <= 4e-3 against the float64
    x @ (f(q) s)^T (the project's int4-against-fp32 bar), <= 1e-2 against the reference module's
    recorded bf16 output (its bar against the dequant path). The all-zero row's column is NaN."""
    rec = load_golden(fname)
    q = torch.from_numpy(rec["q"]).view(FP8).to(DEV)
    s = torch.from_numpy(rec["s"]).to(DEV)
    x = bf16(rec["x"])[:M].to(DEV)
    bias = bf16(rec["bias"]).to(DEV)
    y = torch.ops.torchao.fp8_weight_only_linear(x, q, s, None).cpu()
    kernel = _last_kernel()
    assert kernel == ("fp8wo_gemv_kernel" if M <= 4 else "gemm_mfma_kernel"), kernel
    assert y.dtype == torch.bfloat16 and y.shape == (M, int(rec["N"]))
    y64 = torch.from_numpy(rec["y64"])[:M]
    e64 = rel_l2_finite(y, y64)
    yb = torch.ops.torchao.fp8_weight_only_linear(x, q, s, bias).cpu()
    eref = rel_l2_finite(yb, bf16(rec["y_ref"])[:M])
    e64b = rel_l2_finite(yb, y64 + bf16(rec["bias"]).double())
    print(f"{fname} M={M} {kernel}: rel-L2 vs float64 {e64:.3e} (bias {e64b:.3e}), "
          f"vs reference {eref:.3e}")
    assert e64 <= 4e-3 and e64b <= 4e-3
    assert eref <= 1e-2


@pytest.mark.parametrize("fname", FIXTURES)
def test_linear_mfma_route_on_fixtures(fname):
    """The same bars with the crossover forced down, so M = 3 and 5 both run the MFMA kernel."""
    from torchao.kernel import tuning

    rec = load_golden(fname)
    q = torch.from_numpy(rec["q"]).view(FP8).to(DEV)
    s = torch.from_numpy(rec["s"]).to(DEV)
    bias = bf16(rec["bias"]).to(DEV)
    for M in (3, 5):
        x = bf16(rec["x"])[:M].to(DEV)
        with tuning(linear_crossover=1):
            yb = torch.ops.torchao.fp8_weight_only_linear(x, q, s, bias).cpu()
            assert _last_kernel() == "gemm_mfma_kernel"
        y64 = torch.from_numpy(rec["y64"])[:M] + bf16(rec["bias"]).double()
        assert rel_l2_finite(yb, y64) <= 4e-3
        assert rel_l2_finite(yb, bf16(rec["y_ref"])[:M]) <= 1e-2


def _quantized_cuda_linear(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    lin = lin.to(DEV)
    quantize_(lin, Float8WeightOnlyConfig())
    return lin


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_cuda_model_end_to_end(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _quantized_cuda_linear(rec)
    w = lin.weight
    assert isinstance(w, AffineQuantizedTensor) and isinstance(w.tensor_impl, Float8AQTTensorImpl)
    assert w.device.type == "cuda" and w.block_size == (1, K)
    # the fused quantizer ran and reproduces the reference's codes and scales
    assert same_codes(_u8(w.tensor_impl.float8_data).cpu(), torch.from_numpy(rec["q"]))
    assert torch.equal(w.tensor_impl.scale.cpu().reshape(-1), torch.from_numpy(rec["s"]))
    assert same_bf16(w.dequantize().cpu(), bf16(rec["w_dequant"]))
    assert _last_kernel() == "fp8_dequant_kernel"
    x = bf16(rec["x"])
    with torch.no_grad():
        y = lin(x.to(DEV)).cpu()  # M = 5, with bias
        y3 = lin(x[:4].view(2, 2, K).to(DEV)).cpu()  # a 3-D input
    assert rel_l2_finite(y, bf16(rec["y_ref"])) <= 1e-2
    assert y3.shape == (2, 2, N)
    assert rel_l2_finite(y3.view(4, N), bf16(rec["y_ref"])[:4]) <= 1e-2
    # a quantized CPU module moved to the GPU is the same weight
    cpu = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        cpu.weight.copy_(bf16(rec["w"]))
        cpu.bias.copy_(bf16(rec["bias"]))
    quantize_(cpu, Float8WeightOnlyConfig())
    moved = cpu.to(DEV)
    with torch.no_grad():
        assert same_bf16(moved(x.to(DEV)).cpu(), y)
    # fp32 activations have no kernel: loud, no quiet dequantize -> F.linear
    with pytest.raises(RuntimeError, match="bf16"):
        lin(x.float().to(DEV))


def test_graph_capture_replay_equals_eager():
    rec = load_golden("float8wo_N96_K1024.npz")
    q = torch.from_numpy(rec["q"]).view(FP8).to(DEV)
    s = torch.from_numpy(rec["s"]).to(DEV)
    bias = bf16(rec["bias"]).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x1 = torch.randn(1, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    x32 = torch.randn(32, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    op = torch.ops.torchao.fp8_weight_only_linear
    e1, e32 = op(x1, q, s, bias), op(x32, q, s, None)
    assert _last_kernel() == "gemm_mfma_kernel"
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g1 = op(x1, q, s, bias)
        g32 = op(x32, q, s, None)
    g1.zero_()
    g32.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, e1) and torch.equal(g32, e32)
    # new inputs in the captured buffers, replayed
    x1.copy_(torch.randn(1, 1024, generator=gen).to(torch.bfloat16))
    x32.copy_(torch.randn(32, 1024, generator=gen).to(torch.bfloat16))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, op(x1, q, s, bias)) and torch.equal(g32, op(x32, q, s, None))


@pytest.mark.parametrize("name", ["fp8_weight_only_linear", "fp8_quantize_rows", "fp8_dequantize"])
def test_opcheck(name):
    """torch.library.opcheck: schema, fake impl against the real one, AOT dispatch, autograd
    registration. opcheck's schema test detects input mutation with torch.allclose, which torch
    does not implement for float8 tensors on any device ("mul_cuda" not implemented for
    'Float8_e4m3fn'); for the two ops that take float8 inputs the other three tests run and what
    the schema test would check is checked here by hand: no input changes, no output aliases an
    input."""
    gen = torch.Generator().manual_seed(9)
    N, K = 256, 512
    w = (torch.randn(N, K, generator=gen) * 0.05).to(torch.bfloat16).to(DEV)
    q, s = torch.ops.torchao.fp8_quantize_rows(w)
    x = torch.randn(3, K, generator=gen).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, generator=gen).to(torch.bfloat16).to(DEV)
    args = {"fp8_weight_only_linear": (x, q, s.reshape(-1), bias),
            "fp8_quantize_rows": (w,),
            "fp8_dequantize": (q, s.reshape(-1))}[name]
    op = getattr(torch.ops.torchao, name).default
    if not any(a.dtype == FP8 for a in args):
        torch.library.opcheck(op, args)
        return
    torch.library.opcheck(op, args, test_utils=("test_faketensor", "test_aot_dispatch_dynamic",
                                                "test_autograd_registration"))
    before = [a.clone() for a in args]
    out = op(*args)
    torch.cuda.synchronize()
    for a, b in zip(args, before):
        assert torch.equal(a.view(torch.uint8) if a.dtype == FP8 else a,
                           b.view(torch.uint8) if b.dtype == FP8 else b)
        assert out.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()
