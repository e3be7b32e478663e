"""GPU tests of the MXFP4-weight inference linear (csrc/mx_fp4.hip, the MxFp8Fp4 policy of
csrc/gemm_mfma_policy.h, torchao.prototype.mx_formats with e4m3fn activations and float4_e2m1fn_x2
weights) against the reference fixtures (tests/golden/mxfp4w_*.npz, mxfp4_quant_edges.npz, written by
experiments/gen_golden_mxfp4.py): the quantizer byte for byte, the scale map and the k map of the
mixed-format MFMA and of the GEMV on exact inputs, the ops against the float64 formula on the
reference's codes, K and N tails with guarded scale buffers, quantize_ end to end, graph replay,
opcheck and the argument errors."""

import numpy as np
import pytest
import torch

from conftest import bf16, golden_files, load_golden

from torchao import _lib
from torchao.kernel import tuning
from torchao.prototype.mx_formats import MXFPInferenceConfig
from torchao.prototype.mx_formats.mx_tensor import MXTensor, get_fp_scale, to_mx
from torchao.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
E8 = torch.float8_e8m0fnu
F4 = torch.float4_e2m1fn_x2
FIXTURES = golden_files("mxfp4w_N")
BAR = 4e-3      # the project's bar against float64 on the same codes
BAR_REF = 1e-2  # ... and against the reference's emulated output
T = torch.ops.torchao
# how each route is reached; the GEMV serves M <= 8 at most (tao_tune_linear_crossover)
ROUTES = {"built-in": {}, "mfma": {"mx_mfma": 1}, "gemv": {"linear_crossover": 8}}
F4_VALUES = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6],
                         dtype=torch.float64)


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _rel_l2(y, y64):
    return float((y.double().cpu() - y64).norm() / y64.norm())


def _pack(codes):
    """uint8 e2m1 codes [N, K] -> [N, K/2], element 2 j in the high nibble (the stored order)."""
    return (codes[:, ::2] << 4) | codes[:, 1::2]


def _unpack(wq):
    return torch.stack([wq >> 4, wq & 0xF], -1).reshape(wq.shape[0], -1)


def _y64(xq, xs, wq, ws, bias=None):
    """The formula of csrc/mx_fp4.hip in float64 on uint8 codes and scale bytes (CPU)."""
    def scaled(f, s):
        return (f.reshape(f.shape[0], -1, 32)
                * get_fp_scale(s.view(E8)).double()[..., None]).reshape(f.shape[0], -1)
    y = scaled(xq.view(E4).double(), xs) @ scaled(F4_VALUES[_unpack(wq).long()], ws).t()
    return y if bias is None else y + bias.double()[None, :]


def _operands(rec):
    return (torch.from_numpy(rec["xq"]).view(E4).to(DEV), torch.from_numpy(rec["xs"]).to(DEV),
            torch.from_numpy(rec["wq"]).to(DEV), torch.from_numpy(rec["ws"]).to(DEV),
            bf16(rec["bias"]).to(DEV))


def _route_kernel(route, k, M):
    """The kernel a forced route must have run."""
    if route == "mfma" or (route == "gemv" and M > 8):
        assert "gemm_mfma" in k, (route, k)
    elif route == "gemv":
        assert "mxw4_gemv" in k, (route, k)


# ---- quantizer -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FIXTURES)
def test_quantizer_matches_the_reference_fixtures(fname):
    rec = load_golden(fname)
    codes, scale = T.mxfp4_quantize_rows(bf16(rec["w"]).to(DEV))
    assert _last_kernel() == "mxfp4_quantize_rows_kernel"
    assert codes.dtype is torch.uint8 and scale.dtype is torch.uint8
    assert codes.shape == rec["wq"].shape
    assert np.array_equal(codes.cpu().numpy(), rec["wq"]), fname
    assert np.array_equal(scale.cpu().numpy(), rec["ws"]), fname


def test_quantizer_edge_blocks_and_random_rows():
    rec = load_golden("mxfp4_quant_edges.npz")
    # the nibble written for a NaN input element is compared without its sign bit; nothing else
    mask = np.full(rec["q"].shape, 0xFF, dtype=np.uint8)
    for r, k in rec["nan_elems"]:
        mask[r, k // 2] &= 0x7F if k % 2 == 0 else 0xF7
    assert int((mask != 0xFF).sum()) == 3
    codes, scale = T.mxfp4_quantize_rows(bf16(rec["x"]).to(DEV))
    assert np.array_equal(scale.cpu().numpy(), rec["s"])
    got = codes.cpu().numpy()
    bad = np.argwhere((got & mask) != (rec["q"] & mask))
    assert bad.size == 0, [(r, c, hex(got[r, c]), hex(rec["q"][r, c])) for r, c in bad[:8]]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(33, 2080, generator=g) * torch.exp2(torch.randint(-20, 20, (33, 1), generator=g))
         ).to(torch.bfloat16)
    s_cpu, q_cpu = to_mx(x, F4, 32)
    codes, scale = T.mxfp4_quantize_rows(x.to(DEV))
    assert torch.equal(scale.cpu(), _u8(s_cpu)) and torch.equal(codes.cpu(), q_cpu)
    # leading dimensions, and MXTensor.to_mx on the GPU is the same kernel
    codes3, scale3 = T.mxfp4_quantize_rows(x[:32].reshape(4, 8, 2080).to(DEV))
    assert codes3.shape == (4, 8, 1040) and scale3.shape == (4, 8, 65)
    assert torch.equal(codes3.cpu().reshape(32, -1), q_cpu[:32])
    mx = MXTensor.to_mx(x.to(DEV), F4, 32)
    assert _last_kernel() == "mxfp4_quantize_rows_kernel"
    assert mx.shape == (33, 2080) and mx.qdata.shape == (33, 1040)
    assert mx._scale_e8m0.dtype is E8 and torch.equal(_u8(mx._scale_e8m0).cpu(), _u8(s_cpu))
    assert torch.equal(mx.qdata.cpu(), q_cpu)


# ---- exact maps ------------------------------------------------------------------------------------
def _scales(M, N, nblk):
    m, n, b = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(nblk)[None, :]
    return (7 * m + 3 * b) % 13 - 6, (5 * n + 11 * b) % 17 - 8


def _scale_case(M, N, K):
    """Every w nibble is 1.0 (code 2) and every x code is 1.0 (0x38) in block b0(m) of token m,
    zero elsewhere; scale bytes distinct per (row, block). y[m][n] = 32 * 2^(a(m, b0) + c(n, b0))
    exactly: a byte taken from the wrong lane, row or block gives another power of two."""
    nblk = K // 32
    a, c = _scales(M, N, nblk)
    rows = torch.arange(M)
    b0 = (5 * rows + 3) % nblk
    xq = torch.zeros(M, nblk, 32, dtype=torch.uint8)
    xq[rows, b0] = 0x38
    wq = torch.full((N, K // 2), 0x22, dtype=torch.uint8)
    want = 32.0 * torch.exp2((a[rows, b0][:, None] + c[:, b0].t()).double())
    # the bf16 activation that quantises to this product: 2^a in block b0 (code 2^8, byte a + 119)
    x = torch.zeros(M, nblk, 32, dtype=torch.float64)
    x[rows, b0] = torch.exp2(a[rows, b0].double())[:, None]
    return (xq.reshape(M, K), (a + 127).to(torch.uint8), wq, (c + 127).to(torch.uint8),
            x.reshape(M, K).to(torch.bfloat16), want.to(torch.bfloat16))


def _k_case(M, N, K):
    """x is one-hot at k0(m) = (37 m + 5) % K with code 1.0; w[n][k] is an e2m1 code that depends
    on (n, k) over the seven nonzero magnitudes and both signs, and differs between k and k ^ 1;
    scale bytes distinct per (row, block). y[m][n] = e2m1(w[n][k0(m)]) * 2^(a + c) exactly: a
    swapped nibble pair or a k permutation between the fp8 and the fp4 side gives another value."""
    nblk = K // 32
    a, c = _scales(M, N, nblk)
    rows = torch.arange(M)
    k0 = (37 * rows + 5) % K
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    codes = (1 + (3 * n + 5 * k + (k >> 4)) % 7) | (((n + k + (k >> 5)) & 1) << 3)
    assert bool((codes != codes[:, torch.arange(K) ^ 1]).all())
    xq = torch.zeros(M, K, dtype=torch.uint8)
    xq[rows, k0] = 0x38
    a0 = a[rows, k0 // 32]
    want = F4_VALUES[codes[:, k0].t().long()] * torch.exp2((a0[:, None] + c[:, k0 // 32].t()).double())
    x = torch.zeros(M, K, dtype=torch.float64)
    x[rows, k0] = torch.exp2(a0.double())
    return (xq, (a + 127).to(torch.uint8), _pack(codes.to(torch.uint8)), (c + 127).to(torch.uint8),
            x.to(torch.bfloat16), want.to(torch.bfloat16))


@pytest.mark.parametrize("K", (32, 352, 1024))
@pytest.mark.parametrize("N", (40, 64))
@pytest.mark.parametrize("M", (1, 2, 4, 5, 16, 33))  # 2 and 4: the GEMV's other lane sets
@pytest.mark.parametrize("case", (_scale_case, _k_case))
def test_maps_exact(case, M, N, K):
    xq, xs, wq, ws, x, want = case(M, N, K)
    assert torch.equal(_y64(xq, xs, wq, ws).to(torch.bfloat16), want)  # the test's own algebra
    xq, xs, wq, ws, x = (t.to(DEV) for t in (xq.view(E4), xs, wq, ws, x))

    def check(y, what):
        bad = (_bits(y.cpu()) != _bits(want)).nonzero()
        assert bad.numel() == 0, (what, bad[:8].tolist(), y.cpu()[tuple(bad[0])].item(),
                                  want[tuple(bad[0])].item())

    for route, knobs in ROUTES.items():
        with tuning(**knobs):
            y = T.mxfp4w_scaled_mm(xq, xs, wq, ws, None)
            k = _last_kernel()
            yd = T.mxfp4w_dyn_linear(x, wq, ws, None)
        _route_kernel(route, k, M)
        check(y, (route, k))
        check(yd, (route, "mxfp4w_dyn_linear"))
    if M == 1:  # the one-launch entry
        yd = T.mxfp4w_dyn_linear(x, wq, ws, None)
        assert _last_kernel() == "mxw4_gemv_kernel"
        check(yd, "one launch")
    if K % 256 == 0:
        # the MFMA route reads 8-B words of scale bytes here: the op realigns a misaligned view
        def odd(t):
            buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)
            buf[1:] = t.reshape(-1)
            return buf[1:].view(t.shape)
        with tuning(mx_mfma=1):
            y = T.mxfp4w_scaled_mm(xq, odd(xs), wq, odd(ws), None)
            assert "gemm_mfma" in _last_kernel()
        check(y, "misaligned scales")
    if M == 1:  # leaving tuning() called tao_tune_reset: the forced MFMA route is cleared
        T.mxfp4w_scaled_mm(xq, xs, wq, ws, None)
        assert _last_kernel() == "mxw4_gemv_kernel"


# ---- fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", tuple(ROUTES))
@pytest.mark.parametrize("fname", FIXTURES)
def test_ops_against_float64_on_the_reference_codes(fname, route):
    rec = load_golden(fname)
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    y64 = torch.from_numpy(rec["y64"])
    y_ref = bf16(rec["y_ref"]).double()
    zt = int(rec["zero_token"])
    assert bool(y64.isfinite().all())
    with tuning(**ROUTES[route]):
        y = T.mxfp4w_scaled_mm(xq, xs, wq, ws, bias)
        k = _last_kernel()
        y0 = T.mxfp4w_scaled_mm(xq, xs, wq, ws, None)
        yd = T.mxfp4w_dyn_linear(x, wq, ws, bias)
        y1 = torch.cat([T.mxfp4w_scaled_mm(xq[m:m + 1], xs[m:m + 1], wq, ws, bias)
                        for m in range(5)])
        k1 = _last_kernel()
    assert ("mxw4_gemv" if route == "gemv" else "gemm_mfma") in k, k  # M = 5: above the crossover
    assert ("gemm_mfma" if route == "mfma" else "mxw4_gemv") in k1, k1
    e, e0, e1 = _rel_l2(y, y64), _rel_l2(y0, y64 - bf16(rec["bias"]).double()), _rel_l2(y1, y64)
    er, er1 = _rel_l2(y, y_ref), _rel_l2(y1, y_ref)
    print(f"{fname} {route} {k}: rel-L2 vs float64 M=5 {e:.3e} no bias {e0:.3e} M=1 x5 {e1:.3e}; "
          f"vs the reference's emulated output {er:.3e} / {er1:.3e}")
    assert e <= BAR and e0 <= BAR and e1 <= BAR
    assert er <= BAR_REF and er1 <= BAR_REF
    # the all-zero token: exactly bf16(bias), exactly 0 without it
    assert torch.equal(_bits(y[zt]), _bits(bias)) and torch.equal(_bits(y1[zt]), _bits(bias))
    assert not y0[zt].any() and not y0[zt].isnan().any()
    # the whole linear from bf16 equals quantizer -> scaled mm
    assert torch.equal(_bits(yd), _bits(y))


@pytest.mark.parametrize("fname", FIXTURES)
def test_one_launch_is_bit_identical_to_quantizer_then_scaled_mm(fname):
    rec = load_golden(fname)
    _, _, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    for m in range(5):
        for b in (bias, None):
            yd = T.mxfp4w_dyn_linear(x[m:m + 1], wq, ws, b)
            assert _last_kernel() == "mxw4_gemv_kernel"
            q, s = T.mx_quantize_rows(x[m:m + 1])
            assert torch.equal(_u8(q).cpu(), torch.from_numpy(rec["xq"][m:m + 1]))
            y = T.mxfp4w_scaled_mm(q, s, wq, ws, b)
            assert torch.equal(_bits(yd), _bits(y)), (fname, m)


# ---- tails -----------------------------------------------------------------------------------------
def _guarded(scale_bytes):
    """The scale bytes at the front of a larger allocation whose rest is 0xFF (E8M0 NaN): a read
    past K / 32 shows as NaN in the output and does not fault."""
    n = scale_bytes.numel()
    buf = torch.full((n + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[:n] = scale_bytes.reshape(-1).to(DEV)
    return buf[:n].view(scale_bytes.shape)


@pytest.mark.parametrize("N", (1, 17, 40))
@pytest.mark.parametrize("K", (32, 96, 352, 2080))
def test_tails_with_guarded_scale_buffers(K, N):
    g = torch.Generator().manual_seed(K + N)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    x = torch.randn(33, K, generator=g).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    ws, wq = to_mx(w, F4, 32)
    ws = _u8(ws)
    xs, xq = (_u8(t) for t in to_mx(x, E4, 32))
    y64 = _y64(xq, xs, wq, ws, bias)
    wq_d, ws_d, bias_d = wq.to(DEV), _guarded(ws), bias.to(DEV)
    for M, route in ((1, "built-in"), (1, "mfma"), (5, "gemv"), (5, "mfma"), (33, "built-in")):
        xs_d = _guarded(xs[:M])  # the last token's last block borders the guard
        with tuning(**ROUTES[route]):
            y = T.mxfp4w_scaled_mm(xq[:M].view(E4).to(DEV), xs_d, wq_d, ws_d, bias_d)
            k = _last_kernel()
        _route_kernel(route, k, M)
        assert bool(y.isfinite().all()), (M, route, k)
        e = _rel_l2(y, y64[:M])
        print(f"K={K} N={N} M={M} {route} {k}: {e:.3e}")
        assert e <= BAR, (M, route, k, e)
    yd = T.mxfp4w_dyn_linear(x[:1].to(DEV), wq_d, ws_d, bias_d)
    assert bool(yd.isfinite().all()) and _rel_l2(yd, y64[:1]) <= BAR


# ---- module ----------------------------------------------------------------------------------------
def _module(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    lin = lin.to(DEV)
    quantize_(lin, MXFPInferenceConfig(activation_dtype=E4, weight_dtype=F4))
    return lin


def test_quantized_module_reproduces_the_ops():
    rec = load_golden("mxfp4w_N96_K1024.npz")
    N, K = int(rec["N"]), int(rec["K"])
    lin = _module(rec)
    w = lin.weight
    assert isinstance(w, MXTensor) and w.qdata.is_cuda
    assert _last_kernel() == "mxfp4_quantize_rows_kernel"
    assert w.shape == (N, K) and w.qdata.shape == (N, K // 2) and w._elem_dtype is F4
    assert np.array_equal(w.qdata.cpu().numpy(), rec["wq"])
    assert np.array_equal(_u8(w._scale_e8m0).cpu().numpy(), rec["ws"])
    wq, ws, bias = w.qdata, _u8(w._scale_e8m0), lin.bias.detach()
    g = torch.Generator().manual_seed(9)
    xs = [bf16(rec["x"])[:1], bf16(rec["x"]), torch.randn(33, K, generator=g).to(torch.bfloat16),
          torch.randn(2, 3, K, generator=g).to(torch.bfloat16)]
    with torch.no_grad():
        for x in xs:
            x = x.to(DEV)
            y = lin(x)
            assert y.shape == (*x.shape[:-1], N) and y.dtype is torch.bfloat16
            q, s = T.mx_quantize_rows(x.reshape(-1, K))
            want = T.mxfp4w_scaled_mm(q, s, wq, ws, bias)
            assert torch.equal(_bits(y.reshape(-1, N)), _bits(want))
        y5 = lin(xs[1].to(DEV))
        assert _rel_l2(y5, torch.from_numpy(rec["y64"])) <= BAR
        assert _rel_l2(y5, bf16(rec["y_ref"]).double()) <= BAR_REF
        # an e4m3fn MXTensor activation goes to mxfp4w_scaled_mm
        ya = torch.nn.functional.linear(MXTensor.to_mx(xs[1].to(DEV), E4), w, bias)
        assert torch.equal(_bits(ya), _bits(y5))
        assert lin(torch.zeros(0, K, dtype=torch.bfloat16, device=DEV)).shape == (0, N)
        with pytest.raises(RuntimeError, match="bf16"):
            lin(torch.zeros(2, K, device=DEV))
        # fp4 activations are not served, as act_quant_kwargs or as an MXTensor
        with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
            torch.nn.functional.linear(MXTensor.to_mx(xs[1].to(DEV), F4), w, bias)
        w.act_quant_kwargs.elem_dtype = F4
        with pytest.raises(NotImplementedError, match="MXFP8 inference is served"):
            lin(xs[1].to(DEV))
        w.act_quant_kwargs.elem_dtype = E4
        deq = w.dequantize()
        assert deq.is_cuda and deq.shape == (N, K)
    # to("cpu") and back keeps the bytes; the CPU module refuses to run
    back = lin.to("cpu")
    assert np.array_equal(back.weight.qdata.numpy(), rec["wq"])
    with pytest.raises(NotImplementedError, match="GPU only"):
        back(bf16(rec["x"]))


@pytest.mark.parametrize("M", (1, 5, 33))
def test_graph_replay_equals_eager(M):
    rec = load_golden("mxfp4w_N96_K1024.npz")
    lin = _module(rec)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, int(rec["K"]), generator=g).to(torch.bfloat16).to(DEV)
    with torch.no_grad():
        want = lin(x)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            lin(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = lin(x)
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(want))


@pytest.mark.parametrize("name", ["mxfp4_quantize_rows", "mxfp4w_scaled_mm", "mxfp4w_dyn_linear"])
def test_opcheck(name):
    rec = load_golden("mxfp4w_N40_K352.npz")
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    args = {"mxfp4_quantize_rows": (x,), "mxfp4w_scaled_mm": (xq, xs, wq, ws, bias),
            "mxfp4w_dyn_linear": (x, wq, ws, bias)}[name]
    op = getattr(T, name).default
    if name != "mxfp4w_scaled_mm":
        torch.library.opcheck(op, args)
        return
    # As tests/test_gpu_mx.py::test_opcheck: with float8 inputs opcheck's schema test cannot run
    # (it multiplies its inputs; mul is not implemented for float8), so the other three tests run
    # and input mutation / output aliasing are checked by hand.
    torch.library.opcheck(op, args, test_utils=("test_faketensor", "test_aot_dispatch_dynamic",
                                                "test_autograd_registration"))
    before = [a.clone() for a in args]
    out = op(*args)
    torch.cuda.synchronize()
    for a, b in zip(args, before):
        assert torch.equal(_u8(a) if a.dtype == E4 else a, _u8(b) if b.dtype == E4 else b)
        assert out.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()


def test_argument_refusals():
    rec = load_golden("mxfp4w_N64_K256.npz")
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    mm, dyn, quant = T.mxfp4w_scaled_mm, T.mxfp4w_dyn_linear, T.mxfp4_quantize_rows
    # wrong dtype
    with pytest.raises(RuntimeError, match="bf16"):
        dyn(x.float(), wq, ws, bias)
    with pytest.raises(RuntimeError, match="bf16"):
        quant(x.float())
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        mm(_u8(xq), xs, wq, ws, bias)
    with pytest.raises(RuntimeError, match="packed e2m1"):
        mm(xq, xs, xq, ws, bias)
    with pytest.raises(RuntimeError, match="uint8"):
        mm(xq, xs, wq, ws.float(), bias)
    # scale shape
    with pytest.raises(RuntimeError, match="one byte per 32-element block"):
        mm(xq, xs, wq, ws[:, :4], bias)
    with pytest.raises(RuntimeError, match="one byte per 32-element block"):
        mm(xq, xs[:3], wq, ws, bias)
    with pytest.raises(RuntimeError, match="one byte per 32-element block"):
        dyn(x, wq, ws[:32], bias)
    # last dim: x is [.., K] against wq [N, K/2]
    with pytest.raises(RuntimeError, match="last dim"):
        dyn(x[:, :128], wq, ws, bias)
    with pytest.raises(RuntimeError, match="last dim"):
        mm(xq[:, :128], xs[:, :4], wq, ws, bias)
    # device mismatch
    with pytest.raises(RuntimeError, match="same device"):
        dyn(x, wq, ws.cpu(), bias)
    with pytest.raises(RuntimeError, match="same device"):
        mm(xq, xs, wq, ws, bias.cpu())
    # K not a multiple of 32
    with pytest.raises(RuntimeError, match="multiple of 32"):
        quant(x[:, :40].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 32"):
        mm(xq[:, :48].contiguous(), xs[:, :1], wq[:, :24].contiguous(), ws[:, :1], None)
    # the C entry of the fused launch is one token
    y = torch.empty(2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="one token"):
        _lib.call("tao_mxfp4w_dyn_linear_bf16", x.data_ptr(), wq.data_ptr(), ws.data_ptr(), None,
                  y.data_ptr(), 2, 64, 256, None)
    # empty batch through the ops
    assert mm(xq[:0], xs[:0], wq, ws, bias).shape == (0, 64)
    assert dyn(x[:0], wq, ws, bias).shape == (0, 64)
    q, s = quant(x[:0])
    assert q.shape == (0, 128) and s.shape == (0, 8)
