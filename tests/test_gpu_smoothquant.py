"""GPU tests of SmoothQuant over the int8 dynamic / static linear: the whole flow (insert,
calibrate on the GPU, convert, forward) against the reference's recorded results
(tests/golden/smoothquant_*.npz, experiments/gen_golden_smoothquant.py), and the four ops
(int8_smooth_quantize_per_token / _static, int8_smooth_dyn_linear / _static_linear) against the
plain-torch oracle of tests/smoothquant_oracle.py, which tests/test_smoothquant_cpu.py pins to the
reference. Everything is compared bit for bit: the division, the quantization and the epilogue are
each a fixed sequence of bf16 roundings and the integer dot products are exact.

Kernel cases. K: 16 (smallest), 272 (tail past one wave's pieces), 1024 / 2048 / 4096 (1 / 1 / 2
pieces per thread in the one-token prologue), 4112 (clamped tail chunk), 8192 (8 rows per wave, 4
pieces), 14336 (8 pieces), 28672 (past the prologue: two launches). M: 1 (one launch), 2 and 4
(GEMV), 5, 17 and 130 (quantizer + MFMA). N = 24 with a bias and N = 40 without: neither is a
multiple of the rows per workgroup. The factor is log-uniform in [0.05, 20] and rounded to bf16,
so it is no power of two and every quotient rounds.

Routing at M = 1: the dynamic op takes the one launch up to K = 14336 here (it serves to 16384).
The static op takes it up to K = 8192 only: measured on the MI355X the static one launch is slower
than the static quantizer + GEMV past that (4096 x 14336: 14.5 against 13.2 us), so
at 14336 the op is asserted to take the two launches and the one-launch entry is called directly
(tao_int8_smooth_linear_bf16), which runs the 8-piece static prologue all the same."""

import functools

import pytest
import torch

import smoothquant_oracle as O
from conftest import bf16, load_golden

from torchao import _lib
from torchao.prototype.smoothquant import (
    SmoothQuantConfig,
    SmoothQuantObservedLinear,
    insert_smooth_quant_observer_,
)
from torchao.quantization import quantize_

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
FIXTURES = ["smoothquant_N48_K512.npz", "smoothquant_N64_K256.npz", "smoothquant_N96_K1024.npz"]
KS = [16, 272, 1024, 2048, 4096, 4112, 8192, 14336, 28672]
MS = [1, 2, 4, 5, 17, 130]
ONE_LAUNCH_MAX_K = 14336          # the largest K of KS the one launch serves (it serves to 16384)
STATIC_ONE_LAUNCH_MAX_K = 8192    # the static op's routing boundary
ROWS = 130
# rows of the test activation with a purpose (the rest are ordinary tokens)
ZERO_ROW, CLAMP_ROW, BIG_ROW = 1, 2, 3


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=None)
def _case(K):
    """Inputs and oracle results of one K, computed once on the CPU and shared by its tests:
    x [ROWS, K], factor [K], act_scale, and per N in (24, 40) the weight, scale, bias, and the
    oracle's codes, scales and outputs in both modes."""
    gen = torch.Generator().manual_seed(1000 + K)
    lo, hi = torch.tensor(0.05).log(), torch.tensor(20.0).log()
    factor = torch.exp(lo + (hi - lo) * torch.rand(K, generator=gen)).to(torch.bfloat16)
    pow2 = (factor.float().log2() % 1) == 0  # a draw that rounded to a power of two: next bf16 up
    factor = torch.where(pow2, factor * 1.0078125, factor)
    assert not ((factor.float().log2() % 1) == 0).any()
    assert 0.05 <= float(factor.min()) and float(factor.max()) <= 20.125
    x = (torch.randn(ROWS, K, generator=gen) * 2).to(torch.bfloat16)
    x[ZERO_ROW] = 0
    x[CLAMP_ROW] = (factor.float() * 0.05 * torch.randn(K, generator=gen)).to(torch.bfloat16)
    x[BIG_ROW] = (factor.float() * 10 * torch.randn(K, generator=gen)).to(torch.bfloat16)
    act_scale = torch.tensor(0.0371, dtype=torch.bfloat16)  # 127 * 0.0371 = 4.7: |t| > 4.7 saturates
    case = {"x": x, "factor": factor, "act_scale": act_scale, "K": K}
    for mode, act in (("dynamic", None), ("static", act_scale)):
        xq, xs = O.quant(x, factor, act)
        case[mode] = (xq, xs)
    xq, xs = case["dynamic"]
    assert float(xs[ZERO_ROW]) == 2.0 ** -7 and float(xs[CLAMP_ROW]) == 2.0 ** -7
    assert xq[CLAMP_ROW].any() and float(xs[0]) > 2.0 ** -7
    xq, _ = case["static"]
    assert (xq[BIG_ROW].abs() == 127).any() and (xq[BIG_ROW].abs() < 127).any()
    for N, has_bias in ((24, True), (40, False)):
        wq = torch.randint(-127, 128, (N, K), generator=gen, dtype=torch.int8)
        ws = (0.001 + 0.02 * torch.rand(N, generator=gen)).to(torch.bfloat16)
        bias = torch.randn(N, generator=gen).to(torch.bfloat16) if has_bias else None
        case[N] = {"wq": wq, "ws": ws, "bias": bias}
        for mode in ("dynamic", "static"):
            xq, xs = case[mode]
            case[N][mode] = O.int8_linear(xq, xs, wq, ws, bias)
    return case


def _dev(t):
    return None if t is None else t.to(DEV)


def _linear_op(mode, x, factor, act_scale, wq, ws, bias):
    if mode == "dynamic":
        return T.int8_smooth_dyn_linear(x, factor, wq, ws, bias)
    return T.int8_smooth_static_linear(x, factor, act_scale, wq, ws, bias)


def _quant_op(mode, x, factor, act_scale):
    if mode == "dynamic":
        return T.int8_smooth_quantize_per_token(x, factor)
    return T.int8_smooth_quantize_static(x, factor, act_scale)


@pytest.mark.parametrize("mode", ["dynamic", "static"])
@pytest.mark.parametrize("K", KS)
def test_quantizers_match_the_oracle(K, mode):
    case = _case(K)
    x, factor, act = _dev(case["x"]), _dev(case["factor"]), _dev(case["act_scale"])
    want_q, want_s = case[mode]
    for M in (1, 5, ROWS):
        q, s = _quant_op(mode, x[:M], factor, act)
        if mode == "static":
            assert _last_kernel() == "int8_smooth_quant_static_kernel"
        else:
            assert _last_kernel() == ("int8_smooth_quant_wave_kernel" if K <= 8192
                                      else "int8_smooth_quant_block_kernel")
        assert q.dtype == torch.int8 and q.shape == (M, K)
        assert s.dtype == torch.bfloat16 and s.shape == (M,)
        assert torch.equal(s.cpu(), want_s[:M]), (K, mode, M)
        assert torch.equal(q.cpu(), want_q[:M]), (K, mode, M)
    # a 3-D activation keeps its shape; the scale is one per token
    if K <= 1024:
        q, s = _quant_op(mode, x[:6].reshape(2, 3, K), factor, act)
        assert q.shape == (2, 3, K) and s.shape == (6,)
        assert torch.equal(q.cpu().reshape(6, K), want_q[:6])


@pytest.mark.parametrize("mode", ["dynamic", "static"])
@pytest.mark.parametrize("K", KS)
def test_linears_match_the_oracle_on_every_route(K, mode):
    case = _case(K)
    x, factor, act = _dev(case["x"]), _dev(case["factor"]), _dev(case["act_scale"])
    fused_name = ("int8dyn_gemv_smooth_kernel" if mode == "dynamic"
                  else "int8dyn_gemv_smooth_static_kernel")
    one_launch_max = ONE_LAUNCH_MAX_K if mode == "dynamic" else STATIC_ONE_LAUNCH_MAX_K
    for N in (24, 40):
        wq, ws, bias = (_dev(case[N][k]) for k in ("wq", "ws", "bias"))
        want = case[N][mode]
        if K <= ONE_LAUNCH_MAX_K:
            # the one launch itself, whatever the op's routing says (static K = 14336: 8 pieces)
            for row in (0, ZERO_ROW, CLAMP_ROW, BIG_ROW):
                y = torch.empty((1, N), dtype=torch.bfloat16, device=DEV)
                _lib.call("tao_int8_smooth_linear_bf16", x[row].data_ptr(), factor.data_ptr(),
                          act.data_ptr() if mode == "static" else None, wq.data_ptr(),
                          ws.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
                          1, N, K, torch.cuda.current_stream().cuda_stream)
                assert _last_kernel() == fused_name
                assert torch.equal(y.cpu(), want[row:row + 1]), (K, mode, N, row)
        for M in MS:
            y = _linear_op(mode, x[:M], factor, act, wq, ws, bias)
            last = _last_kernel()
            if M == 1:
                # K = 28672 is past the prologue's registers: the two launches, and no error;
                # the static recipe goes to the two launches past K = 8192 (measured faster)
                assert (last == fused_name) == (K <= one_launch_max), (K, last)
                assert bool(_lib.lib().tao_int8_smooth_linear_fused(
                    1, N, K, int(mode == "static"))) == (K <= one_launch_max)
            if M > 1 or K > one_launch_max:
                assert ("gemv" in last and "smooth" not in last) if M <= 4 else "gemv" not in last, (
                    K, M, last)
            assert y.dtype == torch.bfloat16 and y.shape == (M, N)
            assert torch.equal(y.cpu(), want[:M]), (K, mode, N, M, last)
        # single tokens with a purpose, each through the one launch (or its fallback), and the
        # same token through the two ops: bit-identical to each other and to the oracle
        for row in (ZERO_ROW, CLAMP_ROW, BIG_ROW, 7):
            tok = x[row:row + 1]
            y1 = _linear_op(mode, tok, factor, act, wq, ws, bias)
            q, s = _quant_op(mode, tok, factor, act)
            y2 = T.int8_scaled_mm(q, s, wq, ws, bias)
            assert torch.equal(y1, y2), (K, mode, N, row)
            assert torch.equal(y1.cpu(), want[row:row + 1]), (K, mode, N, row)
        if bias is not None:  # the all-zero token gives bf16(bias)
            y0 = _linear_op(mode, x[ZERO_ROW:ZERO_ROW + 1], factor, act, wq, ws, bias)
            assert torch.equal(y0[0], bias)
        # a 1-D token and a 3-D batch keep their leading shape
        if K == 1024:
            assert _linear_op(mode, x[0], factor, act, wq, ws, bias).shape == (N,)
            y3 = _linear_op(mode, x[:6].reshape(2, 3, K), factor, act, wq, ws, bias)
            assert y3.shape == (2, 3, N) and torch.equal(y3.cpu().reshape(6, N), want[:6])


def test_op_argument_checks():
    case = _case(272)
    x, factor, act = _dev(case["x"][:2]), _dev(case["factor"]), _dev(case["act_scale"])
    wq, ws = _dev(case[24]["wq"]), _dev(case[24]["ws"])
    with pytest.raises(RuntimeError, match="bf16 x"):
        T.int8_smooth_quantize_per_token(x.float(), factor)
    with pytest.raises(RuntimeError, match="bf16 scale"):
        T.int8_smooth_dyn_linear(x, factor.float(), wq, ws, None)
    with pytest.raises(RuntimeError, match="K % 16"):
        T.int8_smooth_quantize_per_token(x[:, :264].contiguous(), factor[:264].contiguous())
    with pytest.raises(RuntimeError, match="act_scale of one element"):
        T.int8_smooth_static_linear(x, factor, factor[:2], wq, ws, None)
    with pytest.raises(RuntimeError, match="same device"):
        T.int8_smooth_quantize_static(x, factor, act.cpu())
    empty = T.int8_smooth_dyn_linear(x[:0], factor, wq, ws, None)
    assert empty.shape == (0, 24)


def test_opcheck():
    case = _case(272)
    factor, act = _dev(case["factor"]), _dev(case["act_scale"])
    wq, ws, bias = (_dev(case[24][k]) for k in ("wq", "ws", "bias"))
    for M in (1, 5):
        x = _dev(case["x"][:M])
        torch.library.opcheck(T.int8_smooth_quantize_per_token.default, (x, factor))
        torch.library.opcheck(T.int8_smooth_quantize_static.default, (x, factor, act))
        torch.library.opcheck(T.int8_smooth_dyn_linear.default, (x, factor, wq, ws, bias))
        torch.library.opcheck(T.int8_smooth_static_linear.default,
                              (x, factor, act, wq, ws, None))


@pytest.mark.parametrize("M", [1, 17])
def test_graph_replay(M):
    case = _case(2048)
    x, factor, act = _dev(case["x"][:M]), _dev(case["factor"]), _dev(case["act_scale"])
    wq, ws, bias = (_dev(case[24][k]) for k in ("wq", "ws", "bias"))

    def run():
        q, s = T.int8_smooth_quantize_per_token(x, factor)
        q2, s2 = T.int8_smooth_quantize_static(x, factor, act)
        return [q, s, q2, s2, T.int8_smooth_dyn_linear(x, factor, wq, ws, bias),
                T.int8_smooth_static_linear(x, factor, act, wq, ws, bias)]

    want = [t.clone() for t in run()]  # eager warm-up
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = run()
    torch.cuda.current_stream().wait_stream(side)
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, ref in zip(outs, want):
        assert torch.equal(got, ref)
    assert torch.equal(outs[4].cpu(), case[24]["dynamic"][:M])
    assert torch.equal(outs[5].cpu(), case[24]["static"][:M])


# ---- module level ------------------------------------------------------------------------------------
def _float_model(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias="bias" in rec.files, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if lin.bias is not None:
            lin.bias.copy_(bf16(rec["bias"]))
    return torch.nn.Sequential(lin).to(DEV)


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_flow_matches_the_reference_bit_for_bit(name):
    rec = load_golden(name)
    calib, x = bf16(rec["calib"]).to(DEV), bf16(rec["x"]).to(DEV)
    for alpha in (None, 0.5, 0.75):
        for mode in ("dynamic", "static"):
            tag = f"a{alpha}_{mode}"
            model = _float_model(rec)
            insert_smooth_quant_observer_(model, alpha, mode)
            model(calib[:40])
            model(calib[40:])
            assert model[0].obs.act_ic_obs.min_val.is_cuda  # the statistics stay on the device
            quantize_(model, SmoothQuantConfig(),
                      lambda m, fqn: isinstance(m, SmoothQuantObservedLinear))
            outer = model[0].weight
            mid = outer.original_weight_tensor
            impl = mid.original_weight_tensor.tensor_impl
            assert outer.scale.is_cuda and impl.int_data.is_cuda
            assert torch.equal(outer.scale.cpu(), bf16(rec[f"smoothing_factor_{tag}"])), tag
            assert torch.equal(impl.int_data.cpu(), torch.from_numpy(rec[f"wq_{tag}"])), tag
            assert torch.equal(impl.scale.reshape(-1).cpu(), bf16(rec[f"ws_{tag}"])), tag
            if mode == "static":
                assert torch.equal(mid.scale.cpu(), bf16(rec[f"act_scales_{tag}"]).reshape(())), tag
            y_ref = bf16(rec[f"y_ref_{tag}"])
            y = model(x)
            assert "smooth" in _last_kernel() or "gemm" in _last_kernel(), _last_kernel()
            assert torch.equal(y.cpu(), y_ref), tag
            for i in range(5):  # each token on its own: the one launch
                yi = model(x[i:i + 1])
                assert _last_kernel() == ("int8dyn_gemv_smooth_kernel" if mode == "dynamic"
                                          else "int8dyn_gemv_smooth_static_kernel")
                assert torch.equal(yi.cpu(), y_ref[i:i + 1]), (tag, i)
            assert torch.equal(model(x.reshape(5, 1, -1)).cpu(), y_ref.reshape(5, 1, -1)), tag


def test_other_inner_weights_keep_the_generic_path():
    """A wrapper around an inner weight that is not SmoothQuant's (here: the plain int8 dynamic
    config's recipe, whose quantizer clamps the scale at 1e-5) takes act_prescale and the inner
    weight's own dispatch, as before."""
    from torchao.quantization import (
        Int8DynamicActivationInt8WeightConfig,
        to_weight_tensor_with_linear_activation_scale_metadata,
    )

    rec = load_golden(FIXTURES[1])
    model = _float_model(rec)
    quantize_(model, Int8DynamicActivationInt8WeightConfig())
    inner = model[0].weight
    factor = _dev(_case(272)["factor"][:256].contiguous())
    wrapped = to_weight_tensor_with_linear_activation_scale_metadata(inner, factor)
    x = bf16(rec["x"]).to(DEV)
    bias = model[0].bias
    y = torch.nn.functional.linear(x[2:3], wrapped, bias)
    assert "smooth" not in _last_kernel()
    assert torch.equal(y, torch.nn.functional.linear(x[2:3] / factor, inner, bias))
