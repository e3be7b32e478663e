"""GPU tests of the NVFP4 kernels (csrc/nvfp4.hip) against the reference fixtures
(tests/golden/nvfp4_*): the HIP quantizer, activation snap and dequantizer bit for bit in both scale
layouts, the linear through ``quantize_`` + ``nn.Linear`` and through the op on both routes and in
both modes within the project's float8 bars (tests/test_gpu_float8.py: 4e-3 against float64, 1e-2
against the reference's own output), the one-launch DYNAMIC decode against its two-launch form bit
for bit, a row of more than one wave slice, argument errors and opcheck of the four ops. The
fixtures hold no inf or NaN; such blocks are outside the bit-exactness claim."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import bf16, golden_files, load_golden

from torchao import _lib
from torchao.kernel.tuning import tuning
from torchao.prototype.mx_formats import NVFP4InferenceConfig, NVFP4MMConfig, NVFP4Tensor
from torchao.prototype.mx_formats.nvfp4_tensor import QuantizeTensorToNVFP4Kwargs
from torchao.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
FIXTURES = golden_files("nvfp4_N")
BAR64, BAR_REF = 4e-3, 1e-2
MS = (1, 2, 4, 5, 8, 11)  # 5 and up: above the built-in boundary; 11: two GEMV launches
ROUTES = ((1, "nvfp4_gemv_kernel"), (2, "nvfp4_dequant_kernel"))
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                    dtype=torch.float64)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(y, ref):
    y, ref = y.detach().cpu().double(), ref.detach().cpu().double()
    return float(torch.linalg.norm(y - ref) / torch.linalg.norm(ref))


def dev_scale(rec, key):
    return torch.from_numpy(rec[key]).to(DEV) if key in rec.files else None


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _rows(a, M):
    """M rows out of the fixture's 5 (rows wrap around beyond them)."""
    return a[np.arange(M) % a.shape[0]]


def _weight(rec, swizzled, dynamic):
    """The fixture's weight on the device, from its bytes (no quantizer involved)."""
    s = torch.from_numpy(rec["scales_swizzled" if swizzled else "scales_rowmajor"])
    return NVFP4Tensor(torch.from_numpy(rec["qdata"]).to(DEV),
                       s.view(torch.float8_e4m3fn).to(DEV), dev_scale(rec, "per_tensor_scale"),
                       dev_scale(rec, "act_per_tensor_scale"), 16, torch.bfloat16, swizzled, False,
                       QuantizeTensorToNVFP4Kwargs() if dynamic else None)


@pytest.mark.parametrize("swizzled", [False, True], ids=["rowmajor", "swizzled"])
@pytest.mark.parametrize("name", FIXTURES + ["nvfp4_quant_edges.npz", "nvfp4_quant_edges.npz:_pts"])
def test_quantizer_snap_and_dequantizer_equal_the_fixture(name, swizzled):
    name, _, tag = name.partition(":")
    rec = load_golden(name)
    edges = "quant_edges" in name
    src = bf16(rec["x" if edges else "w"]).to(DEV)
    pts = dev_scale(rec, "per_tensor_scale") if (tag or not edges) else None
    key = ("scales_swizzled" if swizzled else "scales_rowmajor") + tag
    q, s = T.nvfp4_quantize(src, pts, swizzled)
    assert _last_kernel() == "nvfp4_quantize_rows_kernel"
    assert np.array_equal(q.cpu().numpy(), rec["qdata" + tag])
    assert np.array_equal(s.cpu().numpy(), rec[key].reshape(-1))  # swizzled: the zero padding too
    t = NVFP4Tensor.to_nvfp4(src, per_tensor_scale=pts, is_swizzled_scales=swizzled)
    assert np.array_equal(bits(t.to_dtype(torch.bfloat16)), rec["w_hat" + tag])
    assert _last_kernel() == "nvfp4_dequant_kernel"
    x, apts = (src, pts) if edges else (bf16(rec["x"]).to(DEV), dev_scale(rec, "act_per_tensor_scale"))
    assert np.array_equal(bits(T.nvfp4_act_qdq(x, apts)), rec["x_dq" + tag])


@pytest.mark.parametrize("route,kernel", ROUTES, ids=["gemv", "dequant_mm"])
@pytest.mark.parametrize("dynamic", [False, True], ids=["wo", "dyn"])
@pytest.mark.parametrize("swizzled", [False, True], ids=["rowmajor", "swizzled"])
@pytest.mark.parametrize("name", FIXTURES)
def test_linear_op_on_both_routes(name, swizzled, dynamic, route, kernel):
    rec = load_golden(name)
    w = _weight(rec, swizzled, dynamic)
    bias = bf16(rec["bias"]).to(DEV)
    for M in MS:
        x = bf16(_rows(rec["x"], M)).to(DEV)
        with tuning(nvfp4=(route, 0, 0, 0, 0)):
            y = F.linear(x, w, bias)
            assert _last_kernel() == kernel
        assert y.shape == (M, w.shape[0]) and y.dtype is torch.bfloat16
        e64 = rel_l2(y, torch.from_numpy(_rows(rec["y64_dyn" if dynamic else "y64_wo"], M)))
        assert e64 <= BAR64, f"M={M}: {e64}"
        if not dynamic:
            eref = rel_l2(y, bf16(_rows(rec["y_ref"], M)))
            assert eref <= BAR_REF, f"M={M}: {eref}"


@pytest.mark.parametrize("mode", [NVFP4MMConfig.WEIGHT_ONLY, NVFP4MMConfig.DYNAMIC])
@pytest.mark.parametrize("name", [f for f in FIXTURES if "_pts" not in f])
def test_quantize_then_linear_module(name, mode):
    rec = load_golden(name)
    N, K = rec["w"].shape
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    lin = lin.to(DEV)
    quantize_(lin, NVFP4InferenceConfig(mm_config=mode, use_triton_kernel=False))
    assert isinstance(lin.weight, NVFP4Tensor) and lin.weight._is_swizzled_scales
    assert np.array_equal(lin.weight._scale_e4m3.view(torch.uint8).cpu().numpy(),
                          rec["scales_swizzled"])
    dyn = mode is NVFP4MMConfig.DYNAMIC
    for M in (1, 4, 5):  # built-in route: the GEMV, and beyond 4 tokens dequantize + matmul
        with torch.no_grad():
            y = lin(bf16(_rows(rec["x"], M)).to(DEV))
        assert _last_kernel() == ("nvfp4_gemv_kernel" if M <= 4 else "nvfp4_dequant_kernel")
        assert rel_l2(y, torch.from_numpy(_rows(rec["y64_dyn" if dyn else "y64_wo"], M))) <= BAR64


@pytest.mark.parametrize("swizzled", [False, True], ids=["rowmajor", "swizzled"])
@pytest.mark.parametrize("name", FIXTURES)
def test_dynamic_decode_is_one_launch_equal_to_snap_then_gemv(name, swizzled):
    rec = load_golden(name)
    w = _weight(rec, swizzled, True)
    s = w._scale_e4m3.view(torch.uint8).reshape(-1)
    bias = bf16(rec["bias"]).to(DEV)
    x = bf16(rec["x"][:1]).to(DEV)
    apts = w._act_per_tensor_scale
    with _lib.KernelTimer(4) as timer:
        fused = T.nvfp4_linear(x, w.qdata, s, w._per_tensor_scale, bias, swizzled, True, apts)
    assert len(timer.durations_ms) == 1 and _last_kernel() == "nvfp4_gemv_kernel"
    two = T.nvfp4_linear(T.nvfp4_act_qdq(x, apts), w.qdata, s, w._per_tensor_scale, bias, swizzled,
                         False, apts)
    assert torch.equal(fused, two)


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("dynamic", [False, True], ids=["wo", "dyn"])
def test_row_of_two_wave_slices(M, dynamic):
    # a lane chunk is 32 k, a wave slice 64 chunks: K = 2048 + 192 gives a row two slices, the
    # second one 6 chunks long (58 lanes past the row's end)
    N, K = 48, 2240
    g = torch.Generator().manual_seed(11)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    t = NVFP4Tensor.to_nvfp4(w.to(DEV), is_swizzled_scales=True,
                             act_quant_kwargs=QuantizeTensorToNVFP4Kwargs() if dynamic else None)
    plain = NVFP4Tensor(t.qdata.cpu(), t._scale_e4m3.cpu(), None, None, 16, torch.bfloat16, True)
    codes = torch.stack([plain.qdata >> 4, plain.qdata & 0xF], -1).reshape(N, K).long()
    wd = (E2M1[codes].view(N, -1, 16) * plain._plain_scales().double().unsqueeze(-1)).view(N, K)
    xq = T.nvfp4_act_qdq(x.to(DEV), None).cpu() if dynamic else x
    with tuning(nvfp4=(1, 0, 0, 0, 0)):
        y = F.linear(x.to(DEV), t)
    assert _last_kernel() == "nvfp4_gemv_kernel"
    assert rel_l2(y, xq.double() @ wd.t()) <= BAR64


def test_opcheck():
    rec = load_golden("nvfp4_N48_K64_pts.npz")
    w, x = bf16(rec["w"]).to(DEV), bf16(rec["x"]).to(DEV)
    pts, apts = dev_scale(rec, "per_tensor_scale"), dev_scale(rec, "act_per_tensor_scale")
    bias = bf16(rec["bias"]).to(DEV)
    utils = ("test_schema", "test_faketensor")
    for swizzled in (False, True):
        q, s = T.nvfp4_quantize(w, pts, swizzled)
        torch.library.opcheck(T.nvfp4_quantize.default, (w, pts, swizzled), test_utils=utils)
        torch.library.opcheck(T.nvfp4_dequantize.default, (q, s, pts, swizzled), test_utils=utils)
        for dynamic in (False, True):
            torch.library.opcheck(T.nvfp4_linear.default,
                                  (x, q, s, pts, bias, swizzled, dynamic, apts), test_utils=utils)
    torch.library.opcheck(T.nvfp4_act_qdq.default, (x, apts), test_utils=utils)


def test_argument_errors():
    lib = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 2)
    cases = [
        (lib.tao_nvfp4_quantize_rows_bf16, (p, p, p, None, 2, 24, 0, None), "multiple of 16"),
        (lib.tao_nvfp4_quantize_rows_bf16, (odd, p, p, None, 2, 32, 0, None), "16-byte aligned"),
        (lib.tao_nvfp4_quantize_rows_bf16, (p, p, p, None, 2, 32, 2, None), "swizzled must be 0 or 1"),
        (lib.tao_nvfp4_act_qdq_bf16, (p, p, None, 2, 8, None), "multiple of 16"),
        (lib.tao_nvfp4_dequant_bf16, (p, p, None, odd, 2, 32, 0, None), "16-byte aligned"),
        (lib.tao_nvfp4_linear_bf16, (p, p, p, None, None, None, p, 1, 16, 32, 0, 0, None),
         "multiple of 64"),
        (lib.tao_nvfp4_linear_bf16, (p, p, p, None, None, None, p, 1, 8, 64, 0, 0, None),
         "N \\(8\\) must be a multiple of 16"),
        (lib.tao_nvfp4_linear_bf16, (p, p, p, None, None, None, p, 2, 16, 64, 0, 1, None),
         "the fused snap is one token"),
        (lib.tao_tune_nvfp4, (3, 0, 0, 0, 0), "tune: nvfp4 route must be"),
    ]
    for fn, args, text in cases:
        assert fn(*args) != 0
        assert __import__("re").search(text, lib.tao_last_error().decode()), (fn, text)
    with pytest.raises(RuntimeError, match="scales must hold 64"):
        T.nvfp4_dequantize(buf[:512].view(16, 32), buf[:60], None, False)
    with pytest.raises(RuntimeError, match="one fp32 element"):
        T.nvfp4_act_qdq(torch.zeros(2, 32, dtype=torch.bfloat16, device=DEV),
                        torch.ones(2, device=DEV))
