"""Bit-exact GPU tests of the W4A8 linear (Int8DynamicActivationInt4WeightConfig with
CutlassInt4PackedLayout): the two quantizer kernels,
torch.ops.torchao.rowwise_scaled_linear_cutlass_s8s4 on both routes (the int8 GEMV up to M = 2, or 4
on small weights; the Int8DynW4 policy of the MFMA kernel above) at every launch shape either can
take, the fused one-token w4a8_dyn_linear, and quantize_ end to end.

The oracle is the op's formula on the CPU (torchao/dtypes/uintx/cutlass_int4_packed_layout.py
_w4a8_linear_formula): an exact int32 product, two fp32 multiplications, the fp32 bias add and one
rounding to bf16. Every partial sum on the GPU is an integer too, so no route, reduction order or
split can change a bit: every check is torch.equal, there is no tolerance anywhere."""

import functools

import pytest
import torch

from conftest import bf16, load_golden

from torchao import _lib
from torchao.dtypes import CutlassInt4PackedLayout
from torchao.dtypes.uintx.cutlass_int4_packed_layout import _w4a8_linear_formula
from torchao.kernel import tuning
from torchao.quantization import Int8DynamicActivationInt4WeightConfig, MappingType, quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
FIXTURES = ["w4a8_N64_K256.npz", "w4a8_N96_K1024.npz", "w4a8_N40_K288.npz"]
GEMV, MFMA = "w4a8_gemv_kernel", "gemm_mfma_kernel"
LONG = (80, 8224)  # 33 k steps of 256 with a 32-k tail: split-K and several k-groups really run


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _config():
    return Int8DynamicActivationInt4WeightConfig(
        layout=CutlassInt4PackedLayout(), act_mapping_type=MappingType.SYMMETRIC)


@functools.lru_cache(maxsize=None)
def _fixture(fname):
    rec = load_golden(fname)
    out = {k: torch.from_numpy(rec[k]) for k in ("wq_packed", "ws", "xq", "xs")}
    out.update({k: bf16(rec[k]) for k in ("w", "x", "y_ref")})
    out["bias"] = bf16(rec["bias"]) if "bias" in rec.files else None
    return out


@functools.lru_cache(maxsize=None)
def _random_codes(M, N, K):
    """Codes generated directly, the extremes -128 and -8 included, with unrelated fp32 scales;
    the CPU oracle with and without bias, computed once."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int8)
    wq = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    xq[0, 0], xq[M - 1, K - 1], wq[0, 0], wq[N - 1, K - 1], wq[N - 1, K - 2] = -128, -128, -8, -8, -8
    xq[M // 2, : K // 2] = 127
    wq[N // 2, K // 2:] = 7
    packed = ((wq[:, 1::2] & 0xF) << 4) | (wq[:, 0::2] & 0xF)
    xs = (0.5 + torch.rand(M, generator=g)) * 2.0 ** -6
    ws = (0.5 + torch.rand(N, generator=g)) * 2.0 ** -4
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    want = _w4a8_linear_formula(xq, xs, packed, ws, None)
    want_b = _w4a8_linear_formula(xq, xs, packed, ws, bias)
    return tuple(t.to(DEV) for t in (xq, xs, packed, ws, bias)), want, want_b


def _check_mm(where, M, N, K, kernel):
    (xq, xs, w, ws, bias), want, want_b = _random_codes(M, N, K)
    for b, ref in ((None, want), (bias, want_b)):
        got = T.rowwise_scaled_linear_cutlass_s8s4(xq, xs, w, ws, b, torch.bfloat16).cpu()
        assert _last_kernel() == kernel, (where, _last_kernel())
        bad = (got.view(torch.int16) != ref.view(torch.int16)).nonzero()
        assert torch.equal(got, ref), (
            f"{where} M={M} N={N} K={K} bias={'on' if b is not None else 'off'}: {len(bad)} of "
            f"{ref.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]} want "
            f"{ref[tuple(bad[0])]}")


# ---- the quantizer ops ----------------------------------------------------------------------------

@pytest.mark.parametrize("fname", FIXTURES)
def test_quantizer_ops_match_fixtures(fname):
    f = _fixture(fname)
    q, s = T.int8_quantize_per_token_f32(f["x"].to(DEV))
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and tuple(s.shape) == (6,)
    assert torch.equal(q.cpu(), f["xq"]) and torch.equal(s.cpu(), f["xs"])
    assert not q[1].any() and float(s[1]) == 2.0 ** -23 and int(q[2].min()) == -128
    q3, s3 = T.int8_quantize_per_token_f32(f["x"].reshape(2, 3, -1).to(DEV))
    assert tuple(q3.shape) == (2, 3, f["x"].shape[1]) and tuple(s3.shape) == (2, 3)
    assert torch.equal(q3.reshape(q.shape), q) and torch.equal(s3.reshape(-1), s)
    p, ws = T.int4_quantize_rows_packed(f["w"].to(DEV))
    assert p.dtype == torch.int8 and ws.dtype == torch.float32
    assert torch.equal(p.cpu(), f["wq_packed"]) and torch.equal(ws.cpu(), f["ws"])
    assert not p[1].any()


def test_token_quantizer_block_kernel_for_long_k():
    """K > 8192 leaves the one-wave-per-token kernel for the one-workgroup-per-token kernel; both
    equal the torch-op formulation on the CPU."""
    from torchao.quantization.quant_api import _int8_symm_cutlass_quant

    g = torch.Generator().manual_seed(3)
    for K in (8192, 8200):
        x = torch.randn(3, K, generator=g).to(torch.bfloat16)
        x[1] = 0
        ref = _int8_symm_cutlass_quant(x).tensor_impl
        q, s = T.int8_quantize_per_token_f32(x.to(DEV))
        want = "w4a8_quant_row_kernel" if K > 8192 else "w4a8_quant_per_token_wave_kernel"
        assert _last_kernel() == want
        assert torch.equal(q.cpu(), ref.int_data) and torch.equal(s.cpu(), ref.scale)


# ---- rowwise_scaled_linear_cutlass_s8s4 -------------------------------------------------------------

@pytest.mark.parametrize("fname", FIXTURES)
def test_scaled_mm_on_fixtures(fname):
    f = _fixture(fname)
    w, ws = f["wq_packed"].to(DEV), f["ws"].to(DEV)
    b = None if f["bias"] is None else f["bias"].to(DEV)
    for M in (1, 2, 4, 5, 6):
        xq, xs = f["xq"][:M].to(DEV), f["xs"][:M].to(DEV)
        got = T.rowwise_scaled_linear_cutlass_s8s4(xq, xs, w, ws, b, torch.bfloat16).cpu()
        assert _last_kernel() == (GEMV if M <= 4 else MFMA)
        assert torch.equal(got, f["y_ref"][:M]), (fname, M)
        # the oracle itself against the fixture
        assert torch.equal(_w4a8_linear_formula(f["xq"][:M], f["xs"][:M], f["wq_packed"], f["ws"],
                                                f["bias"]), f["y_ref"][:M])


@pytest.mark.parametrize("N,K", [(16, 32), (40, 288), (80, 1056), (272, 4128)])
def test_scaled_mm_random_codes_both_routes(N, K):
    """A single chunk, both K tails, N below and across the 64-column tile, the row-group edges of
    the GEMV, and both routes."""
    for M in (1, 3, 4, 5, 16, 17, 33, 130):
        _check_mm("built-in", M, N, K, GEMV if M <= 4 else MFMA)


def test_route_boundary_moved_both_ways():
    """The built-in route is the GEMV up to M = 2, and up to M = 4 for weights of at most 32 Mi
    elements; the crossover knob moves it, and each M near it gives the same bits on both kernels
    (the MFMA kernel then runs with most of its 16-row tile past M)."""
    N, K = 80, 1056
    for M in (2, 3, 4):
        with tuning(linear_crossover=1):
            _check_mm("crossover 1", M, N, K, MFMA)
        with tuning(linear_crossover=8):
            _check_mm("crossover 8", M, N, K, GEMV)
    with tuning(linear_crossover=2):
        _check_mm("crossover 2", 2, N, K, GEMV)
        _check_mm("crossover 2", 3, N, K, MFMA)
    with tuning(linear_crossover=8):  # the GEMV ends at 4 tokens whatever the knob says
        _check_mm("crossover 8", 5, N, K, MFMA)
    # a weight above 32 Mi elements: M = 3 leaves the GEMV (zero codes: the route is the subject)
    Nb, Kb = 4104, 8192
    w = torch.zeros(Nb, Kb // 2, dtype=torch.int8, device=DEV)
    ws = torch.ones(Nb, device=DEV)
    for M, kernel in ((2, GEMV), (3, MFMA), (4, MFMA)):
        xq = torch.ones(M, Kb, dtype=torch.int8, device=DEV)
        y = T.rowwise_scaled_linear_cutlass_s8s4(xq, torch.ones(M, device=DEV), w, ws, None, None)
        assert _last_kernel() == kernel and not y.any()


MFMA_TILES = [(16, 1, 1), (16, 2, 1), (16, 4, 1), (16, 1, 2), (32, 1, 1), (32, 2, 3), (32, 4, 2),
              (64, 1, 3), (64, 2, 2), (128, 1, 1), (128, 1, 2)]


@pytest.mark.parametrize("bm,kg,splits", MFMA_TILES)
def test_mfma_every_launch_shape(bm, kg, splits):
    """Every (BM, k-groups, split-K slices) instance of Int8DynW4: uneven slices, idle k-groups in
    the last slice and the K tail in the last step."""
    with tuning(gemm=(bm, kg, splits)):
        for M in (17, 130):
            _check_mm(f"mfma bm={bm} kg={kg} splits={splits}", M, *LONG, MFMA)


@pytest.mark.parametrize("bm,kg,splits", [(16, 1, 1), (16, 2, 2), (32, 1, 3), (32, 2, 1),
                                          (64, 1, 2), (64, 2, 1)])
def test_mfma_two_column_blocks_per_wave(bm, kg, splits):
    with tuning(gemm=(bm, kg, splits), gemm_nw=2):
        for M in (17, 130):
            _check_mm(f"mfma nw=2 bm={bm} kg={kg} splits={splits}", M, *LONG, MFMA)


def test_mfma_fenced_split_k():
    with tuning(gemm=(32, 2, 3), splitk_fenced=1):
        _check_mm("mfma fenced", 33, *LONG, MFMA)


GEMV_SHAPES = [(rpw, wk, g) for rpw in (2, 4, 8) for wk, g in ((1, 1), (2, 2), (4, 2), (8, 1), (1, 8))]


@pytest.mark.parametrize("rpw,wk,g", GEMV_SHAPES)
def test_gemv_every_launch_shape(rpw, wk, g):
    """Every rows-per-wave x waves-along-K x row-groups shape of the M == 1 GEMV, plain and fused
    (5 slices of 2048 k: more slices than waves, and as many), then M = 2, 3, 4 on theirs."""
    N, K = LONG
    (xq, xs, w, ws, bias), want, want_b = _random_codes(4, N, K)
    g1 = torch.Generator().manual_seed(rpw * 100 + wk * 10 + g)
    x = torch.randn(1, K, generator=g1).to(torch.bfloat16).to(DEV)
    q, s = T.int8_quantize_per_token_f32(x)
    ref = _w4a8_linear_formula(q.cpu(), s.cpu(), w.cpu(), ws.cpu(), bias.cpu())
    with tuning(int8_gemv=(rpw, wk, g)):
        got = T.rowwise_scaled_linear_cutlass_s8s4(xq[:1], xs[:1], w, ws, bias, None).cpu()
        assert _last_kernel() == GEMV and torch.equal(got, want_b[:1])
        got = T.rowwise_scaled_linear_cutlass_s8s4(q, s, w, ws, bias, None).cpu()
        assert torch.equal(got, ref)
        got = T.w4a8_dyn_linear(x, w, ws, bias).cpu()
        assert _last_kernel() == GEMV and torch.equal(got, ref)
    for M in (2, 3, 4):
        _check_mm("gemv", M, N, K, GEMV)


# ---- w4a8_dyn_linear ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fname", FIXTURES)
def test_dyn_linear_equals_quantizer_then_scaled_mm(fname):
    f = _fixture(fname)
    w, ws = f["wq_packed"].to(DEV), f["ws"].to(DEV)
    b = None if f["bias"] is None else f["bias"].to(DEV)
    x = f["x"].to(DEV)
    for m in range(6):  # token 1 is all zeros, token 2 holds the code -128
        one = T.w4a8_dyn_linear(x[m:m + 1], w, ws, b)
        assert _last_kernel() == GEMV
        q, s = T.int8_quantize_per_token_f32(x[m:m + 1])
        two = T.rowwise_scaled_linear_cutlass_s8s4(q, s, w, ws, b, None)
        assert torch.equal(one, two) and torch.equal(one.cpu(), f["y_ref"][m:m + 1]), (fname, m)
    want1 = (f["bias"] if f["bias"] is not None else torch.zeros(w.shape[0])).float()
    assert torch.equal(T.w4a8_dyn_linear(x[1:2], w, ws, b).cpu().float().reshape(-1), want1)
    y5 = T.w4a8_dyn_linear(x[:5], w, ws, b)
    assert _last_kernel() == MFMA
    q, s = T.int8_quantize_per_token_f32(x[:5])
    assert torch.equal(y5, T.rowwise_scaled_linear_cutlass_s8s4(q, s, w, ws, b, None))
    assert torch.equal(y5.cpu(), f["y_ref"][:5])
    y3 = T.w4a8_dyn_linear(x.reshape(2, 3, -1), w, ws, b)
    assert tuple(y3.shape) == (2, 3, w.shape[0])
    assert torch.equal(y3.cpu().reshape(6, -1), f["y_ref"])
    y111 = T.w4a8_dyn_linear(x[3].reshape(1, 1, -1), w, ws, b)
    assert tuple(y111.shape) == (1, 1, w.shape[0]) and _last_kernel() == GEMV
    assert torch.equal(y111.cpu().reshape(1, -1), f["y_ref"][3:4])


@pytest.mark.parametrize("K", [32, 4096, 4128, 8224, 16416, 32800])
def test_dyn_linear_every_token_piece_count(K):
    """The fused launch's token pieces per thread (1, 2, 4, 8, 16 over this K list, and 16 again
    at 32800 with the row groups doubled to 512 threads so that the token fits) against the two
    ops."""
    N = 24
    g = torch.Generator().manual_seed(K)
    wq = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    w = (((wq[:, 1::2] & 0xF) << 4) | (wq[:, 0::2] & 0xF)).to(DEV)
    ws = ((0.5 + torch.rand(N, generator=g)) * 2.0 ** -4).to(DEV)
    x = torch.randn(1, K, generator=g).to(torch.bfloat16).to(DEV)
    one = T.w4a8_dyn_linear(x, w, ws, None)
    assert _last_kernel() == GEMV
    q, s = T.int8_quantize_per_token_f32(x)
    assert torch.equal(one, T.rowwise_scaled_linear_cutlass_s8s4(q, s, w, ws, None, None))
    assert torch.equal(one.cpu(), _w4a8_linear_formula(q.cpu(), s.cpu(), w.cpu(), ws.cpu(), None))


# ---- end to end ----------------------------------------------------------------------------------------

def _linear(f):
    N, K = f["w"].shape
    lin = torch.nn.Linear(K, N, bias=f["bias"] is not None, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(f["w"])
        if f["bias"] is not None:
            lin.bias.copy_(f["bias"])
    return lin


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_and_forward_end_to_end(fname):
    f = _fixture(fname)
    on_gpu = _linear(f).to(DEV)
    quantize_(on_gpu, _config())
    assert _last_kernel() == "w4a8_quant_row_kernel"  # the fused weight quantizer ran
    impl = on_gpu.weight.original_weight_tensor.tensor_impl
    assert impl.int_data.is_cuda and torch.equal(impl.int_data.cpu(), f["wq_packed"])
    assert torch.equal(impl.scale.cpu(), f["ws"])
    moved = _linear(f)
    quantize_(moved, _config())
    moved = moved.to(DEV)
    assert moved.weight.original_weight_tensor.tensor_impl.int_data.is_cuda
    x = f["x"].to(DEV)
    for lin in (on_gpu, moved):
        y = lin(x)
        assert _last_kernel() == MFMA
        assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), f["y_ref"])
        y1 = lin(x[2:3])
        assert _last_kernel() == GEMV and torch.equal(y1.cpu(), f["y_ref"][2:3])
        assert torch.equal(lin(x[:3]).cpu(), f["y_ref"][:3])
        assert torch.equal(lin(x.reshape(3, 2, -1)).cpu().reshape(6, -1), f["y_ref"])


# ---- registration, capture, errors ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rowwise_scaled_linear_cutlass_s8s4", "int8_quantize_per_token_f32",
                                  "int4_quantize_rows_packed", "w4a8_dyn_linear"])
def test_opcheck(name):
    f = _fixture(FIXTURES[0])
    d = {k: (None if v is None else v.to(DEV)) for k, v in f.items()}
    args = {
        "rowwise_scaled_linear_cutlass_s8s4": (d["xq"][:3], d["xs"][:3], d["wq_packed"], d["ws"],
                                               d["bias"], torch.bfloat16),
        "int8_quantize_per_token_f32": (d["x"],),
        "int4_quantize_rows_packed": (d["w"],),
        "w4a8_dyn_linear": (d["x"][:3], d["wq_packed"], d["ws"], d["bias"]),
    }[name]
    torch.library.opcheck(getattr(T, name).default, args)


def test_graph_capture_replay_equals_eager():
    f = _fixture(FIXTURES[1])
    w, ws = f["wq_packed"].to(DEV), f["ws"].to(DEV)
    x1 = f["x"][3:4].to(DEV)
    x5 = f["x"][:5].to(DEV)
    e1, e5 = T.w4a8_dyn_linear(x1, w, ws, None), T.w4a8_dyn_linear(x5, w, ws, None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g1 = T.w4a8_dyn_linear(x1, w, ws, None)
        g5 = T.w4a8_dyn_linear(x5, w, ws, None)
    g1.zero_()
    g5.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1, e1) and torch.equal(g5, e5)
    x1.copy_(f["x"][2:3])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g1.cpu(), _w4a8_linear_formula(f["xq"][2:3], f["xs"][2:3], f["wq_packed"],
                                                      f["ws"], None))


def test_argument_errors():
    f = _fixture(FIXTURES[0])
    d = {k: (None if v is None else v.to(DEV)) for k, v in f.items()}
    mm, dyn = T.rowwise_scaled_linear_cutlass_s8s4, T.w4a8_dyn_linear
    xq, xs, w, ws = d["xq"], d["xs"], d["wq_packed"], d["ws"]
    with pytest.raises(RuntimeError, match="bfloat16 output only"):
        mm(xq, xs, w, ws, None, torch.float16)
    with pytest.raises(RuntimeError, match="input must be int8"):
        mm(d["x"], xs, w, ws, None, None)
    with pytest.raises(RuntimeError, match="last dim"):
        mm(xq[:, :128], xs, w, ws, None, None)
    with pytest.raises(RuntimeError, match="one entry per row"):
        mm(xq, xs[:3], w, ws, None, None)
    with pytest.raises(RuntimeError, match="weight_scale must be"):
        mm(xq, xs, w, ws[:5], None, None)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        mm(xq[:, :48].contiguous(), xs, w[:, :24].contiguous(), ws, None, None)
    with pytest.raises(RuntimeError, match="same device"):
        mm(xq, xs.cpu(), w, ws, None, None)
    with pytest.raises(RuntimeError, match="bf16"):
        dyn(torch.zeros(2, 256, device=DEV), w, ws, None)
    assert mm(xq[:0], xs[:0], w, ws, d["bias"], None).shape == (0, 64)
    assert dyn(d["x"][:0], w, ws, d["bias"]).shape == (0, 64)
