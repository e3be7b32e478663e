"""GPU tests of the NF4 (QLoRA) weight-only workflow against the reference fixtures
(tests/golden/nf4_*, written by experiments/gen_golden_nf4.py): the block quantizer and the
dequantizer byte for byte, the linear on both routes within the project's bar and against the
reference's own output, quantize_ end to end, autograd, device moves, graph capture, argument
errors and opcheck of the three ops."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, bf16, golden_files, load_golden
from test_nf4_cpu import INNER, assert_stored, bits, from_fixture, mean_is_pinned, rel_l2

from torchao import _lib
from torchao.dtypes import NF4Tensor, to_nf4
from torchao.dtypes._nf4tensor_api import nf4_weight_only
from torchao.dtypes.nf4tensor import linear_nf4
from torchao.kernel import tuning
from torchao.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
FIXTURES = golden_files("nf4_N")
LINEAR_FIXTURES = [f for f in FIXTURES if int(f.split("_K")[1].split(".")[0]) % 64 == 0]
BAR = 4e-3
ROUTES = {"gemv": (1, "nf4_gemv_kernel"), "dequant_mm": (2, "nf4_dequant_kernel")}


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _parts(t: NF4Tensor):
    return (t.quantized_data, t.quantized_scalers, t.quantization_factor, t.scaler_mean, t.nf4)


def _dev_tensor(rec, shape=None) -> NF4Tensor:
    return from_fixture(rec, rec["w"].shape if shape is None else shape).cuda()


def test_fixture_sets():
    assert len(FIXTURES) == 6 and "nf4_N512_K96.npz" in FIXTURES and len(LINEAR_FIXTURES) == 5


@pytest.mark.parametrize("fname", FIXTURES)
def test_device_quantizer_equals_the_fixture(fname):
    rec = load_golden(fname)
    w = bf16(rec["w"])
    assert mean_is_pinned(w)
    t = to_nf4(w.to(DEV))
    assert _last_kernel() == "nf4_quantize_blocks_kernel"
    assert isinstance(t, NF4Tensor) and t.device.type == "cuda" and t.shape == w.shape
    assert all(getattr(t, n).device.type == "cuda" for n in INNER)
    assert_stored(t, rec)


def test_device_quantizer_edges():
    """Every byte of both edge tensors: the all-zero block, the negative absmax element, the
    block of equal values, the bf16 neighbours of every level midpoint, and the inf."""
    rec = load_golden("nf4_quant_edges.npz")
    for prefix in ("fin_", "inf_"):
        t = to_nf4(bf16(rec[prefix + "w"]).to(DEV))
        assert _last_kernel() == "nf4_quantize_blocks_kernel"
        assert_stored(t, rec, prefix)
    # the first stage alone: absmax of the inf block is inf, its codes 7 (0 / inf) but the inf's
    codes, absmax = T.nf4_quantize_blocks(bf16(rec["inf_w"]).to(DEV), t.nf4)
    assert float(absmax[5]) == float("inf") and float(absmax[0]) == 0.0


@pytest.mark.parametrize("fname", FIXTURES)
def test_device_dequantizer_equals_w_hat(fname):
    rec = load_golden(fname)
    t = _dev_tensor(rec)
    for out in (t.get_original_weight(), t.to(torch.bfloat16)):
        assert _last_kernel() == "nf4_dequant_kernel"
        assert out.is_cuda and out.shape == rec["w"].shape
        assert np.array_equal(bits(out.cpu()), rec["w_hat"])
    # 1-D, and a float32 request
    flat = _dev_tensor(rec, (rec["w"].size,))
    assert np.array_equal(bits(flat.get_original_weight().cpu()), rec["w_hat"].reshape(-1))
    assert torch.equal(t.to(torch.float32).cpu(), bf16(rec["w_hat"]).float())
    # the transposed view
    assert torch.equal(t.t().to(torch.bfloat16).cpu(), bf16(rec["w_hat"]).t())


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("fname", LINEAR_FIXTURES)
def test_linear_meets_the_bar_and_the_reference(fname, route):
    """Against the float64 formula at M = 1, 3, 5 (bar 4e-3, which the float32 formula meets:
    test_nf4_cpu.py), and against the reference's own CPU output: the distance is at most twice
    the worse of the two distances to float64 (different summation orders on the same w^)."""
    rec = load_golden(fname)
    t = _dev_tensor(rec)
    N = rec["w"].shape[0]
    x, bias = bf16(rec["x"]).to(DEV), bf16(rec["bias"]).to(DEV)
    y64 = torch.from_numpy(rec["y64"])
    y_ref = bf16(rec["y_ref"])
    force, kernel = ROUTES[route]
    with tuning(nf4=(force, 0, 0, 0, 0)):
        for M in (1, 3, 5):
            y = T.nf4_linear(x[:M], *_parts(t), N, bias).cpu()
            if kernel is not None:
                assert _last_kernel() == kernel
            else:
                assert _lib.lib().tao_nf4_linear_route(M, N, x.shape[1]) == 2
            e_own = rel_l2(y, y64[:M])
            e_ref = rel_l2(y_ref[:M], y64[:M])
            d = float(torch.linalg.norm(y.double() - y_ref[:M].double())
                      / torch.linalg.norm(y64[:M]))
            print(f"{fname} {route} M={M}: rel-L2 to float64 own {e_own:.3e} reference "
                  f"{e_ref:.3e}; own vs reference {d:.3e}")
            assert e_own <= BAR
            assert d <= 2 * max(e_own, e_ref)


@pytest.mark.parametrize("fname", ["nf4_N48_K1024.npz", "nf4_N512_K96.npz"])
def test_quantize_end_to_end(fname):
    rec = load_golden(fname)
    N, K = rec["w"].shape
    m = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(bf16(rec["w"]))
        m.bias.copy_(bf16(rec["bias"]))
    m = m.to(DEV)
    quantize_(m, nf4_weight_only())
    w = m.weight
    assert isinstance(w, NF4Tensor) and isinstance(w, torch.nn.Parameter) and not w.requires_grad
    assert_stored(w, rec)
    gen = torch.Generator().manual_seed(3)
    hip = K % 64 == 0
    for shape in ((1, K), (3, K), (1, 1, K), (2, 20, K), (0, K)):
        x = torch.randn(*shape, generator=gen).to(torch.bfloat16).to(DEV)
        with torch.no_grad():
            y = m(x)
        assert y.shape == (*shape[:-1], N) and y.dtype is torch.bfloat16
        if hip:
            want = T.nf4_linear(x, *_parts(w), N, m.bias)
            if x.numel():
                rows = x.numel() // K
                assert _last_kernel() == ("nf4_gemv_kernel" if rows <= 4 else "nf4_dequant_kernel")
        else:  # blocks straddle rows: the HIP dequantizer + the bf16 matmul, bias a second rounding
            want = F.linear(x, T.nf4_dequantize(*_parts(w), [N, K])) + m.bias
        assert torch.equal(y, want)
    if hip:
        with torch.no_grad():
            y5 = m(bf16(rec["x"]).to(DEV)).cpu()
        assert rel_l2(y5, torch.from_numpy(rec["y64"])) <= BAR


def test_autograd_grad_input_and_no_weight_grad():
    rec = load_golden("nf4_N40_K2048.npz")
    t = _dev_tensor(rec)
    w_hat = T.nf4_dequantize(*_parts(t), list(t.shape))
    lora_a = torch.nn.Parameter(torch.zeros(8, 2048, dtype=torch.bfloat16, device=DEV) + 0.01)
    for M in (3, 40):  # forward on the GEMV and on dequantize + matmul
        x = bf16(rec["x"])[:3].repeat(M // 3 + 1, 1)[:M].to(DEV).requires_grad_(True)
        y = linear_nf4(x, t) + (x @ lora_a.t()).sum(-1, keepdim=True)  # a QLoRA-style side branch
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16)
        g = g.to(DEV)
        (gx,) = torch.autograd.grad(linear_nf4(x, t), x, g)
        # (backward runs on the autograd engine's device thread: tao_last_kernel, which is per
        # thread, does not see its launches; the bits below are the HIP dequantizer's)
        assert torch.equal(gx, g @ w_hat)
        y.backward(g)
        assert x.grad is not None and lora_a.grad is not None
    assert t.grad is None and not t.requires_grad


def test_cuda_cpu_moves():
    rec = load_golden("nf4_N64_K256.npz")
    host = from_fixture(rec, rec["w"].shape)
    dev = host.cuda()
    assert isinstance(dev, NF4Tensor) and dev.device.type == "cuda" and dev.shape == host.shape
    assert all(getattr(dev, n).is_cuda for n in INNER)
    assert_stored(dev, rec)
    for back in (dev.cpu(), dev.to("cpu")):
        assert isinstance(back, NF4Tensor) and back.device.type == "cpu"
        assert_stored(back, rec)
        assert np.array_equal(bits(back.get_original_weight()), rec["w_hat"])
    dev2 = host.to(DEV)
    assert isinstance(dev2, NF4Tensor) and dev2.quantized_data.is_cuda
    assert np.array_equal(bits(dev2.to(torch.bfloat16).cpu()), rec["w_hat"])


def test_graph_capture_replay_equals_eager():
    rec = load_golden("nf4_N48_K1024.npz")
    t = _dev_tensor(rec)
    parts, N = _parts(t), 48
    bias = bf16(rec["bias"]).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x1 = torch.randn(1, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    x32 = torch.randn(32, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    x300 = torch.randn(300, 1024, generator=gen).to(torch.bfloat16).to(DEV)
    e1, e32 = T.nf4_linear(x1, *parts, N, bias), T.nf4_linear(x32, *parts, N, None)
    assert _last_kernel() == "nf4_dequant_kernel"
    e300 = T.nf4_linear(x300, *parts, N, bias)
    ew = T.nf4_dequantize(*parts, [48, 1024])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g1 = T.nf4_linear(x1, *parts, N, bias)
        g32 = T.nf4_linear(x32, *parts, N, None)
        g300 = T.nf4_linear(x300, *parts, N, bias)
        gw = T.nf4_dequantize(*parts, [48, 1024])
    for o in (g1, g32, g300, gw):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, e1) and torch.equal(g32, e32) and torch.equal(gw, ew)
    assert torch.equal(g300, e300)
    x1.copy_(torch.randn(1, 1024, generator=gen).to(torch.bfloat16))
    x32.copy_(torch.randn(32, 1024, generator=gen).to(torch.bfloat16))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, T.nf4_linear(x1, *parts, N, bias))
    assert torch.equal(g32, T.nf4_linear(x32, *parts, N, None))


def test_argument_errors():
    rec = load_golden("nf4_N64_K256.npz")
    t = _dev_tensor(rec)
    codes, qs, qf, mean, lv = _parts(t)
    x = bf16(rec["x"]).to(DEV)
    with pytest.raises(RuntimeError, match="needs bf16 x"):
        T.nf4_linear(x.float(), codes, qs, qf, mean, lv, 64, None)
    with pytest.raises(RuntimeError, match="multiple of the block size 64"):
        T.nf4_linear(x[:, :96], codes, qs, qf, mean, lv, 64, None)
    with pytest.raises(RuntimeError, match="codes must have numel / 2"):
        T.nf4_linear(x, codes, qs, qf, mean, lv, 32, None)
    with pytest.raises(RuntimeError, match="qscalers must be int8"):
        T.nf4_linear(x, codes, qs.to(torch.int16), qf, mean, lv, 64, None)
    with pytest.raises(RuntimeError, match="codes must be uint8"):
        T.nf4_dequantize(codes.to(torch.int8), qs, qf, mean, lv, [64, 256])
    with pytest.raises(RuntimeError, match="qfactor must have"):
        T.nf4_dequantize(codes, qs, qf.repeat(2), mean, lv, [64, 256])
    with pytest.raises(RuntimeError, match="levels must have 16"):
        T.nf4_dequantize(codes, qs, qf, mean, lv[:8], [64, 256])
    with pytest.raises(RuntimeError, match="same device"):
        T.nf4_dequantize(codes, qs.cpu(), qf, mean, lv, [64, 256])
    with pytest.raises(RuntimeError, match="bias must have N"):
        T.nf4_linear(x, codes, qs, qf, mean, lv, 64, x[0, :3])
    with pytest.raises(RuntimeError, match="needs a bf16 weight"):
        T.nf4_quantize_blocks(torch.zeros(64, 256, device=DEV), lv)
    with pytest.raises(RuntimeError, match="multiple of the block size 64"):
        T.nf4_quantize_blocks(torch.zeros(100, dtype=torch.bfloat16, device=DEV), lv)
    with pytest.raises(RuntimeError, match="tune: nf4 route"):
        _lib.call("tao_tune_nf4", 3, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="waves_k \\* row_groups"):
        _lib.call("tao_tune_nf4", 0, 0, 0, 4, 4)
    # M == 0 is a no-op with the right shape
    assert T.nf4_linear(x[:0], codes, qs, qf, mean, lv, 64, None).shape == (0, 64)


@pytest.mark.parametrize("name", ["nf4_quantize_blocks", "nf4_dequantize", "nf4_linear"])
def test_opcheck(name):
    rec = load_golden("nf4_N64_K256.npz")
    t = _dev_tensor(rec)
    args = {
        "nf4_quantize_blocks": (bf16(rec["w"]).to(DEV), t.nf4),
        "nf4_dequantize": (*_parts(t), [64, 256]),
        "nf4_linear": (bf16(rec["x"])[:3].to(DEV), *_parts(t), 64, bf16(rec["bias"]).to(DEV)),
    }[name]
    torch.library.opcheck(getattr(T, name).default, args)


def test_reference_checkpoint_on_the_device():
    rec = load_golden("nf4_refckpt_N32_K512.npz")
    sd = torch.load(os.path.join(GOLDEN, "nf4_refckpt_N32_K512.pt"), weights_only=True)
    w = sd["weight"].cuda()
    assert_stored(w, rec)
    assert np.array_equal(bits(w.get_original_weight().cpu()), rec["w_hat"])
    assert_stored(to_nf4(bf16(rec["w"]).to(DEV)), rec)
