"""GPU tests of AWQ over the int4 weight-only linear: the activation pre-scale kernel against
torch's bf16 division, the fused one-token launch against its two-launch form, the op's routing at
more tokens, the converted module against the reference's outputs (tests/golden/awq_*.npz,
experiments/gen_golden_awq.py), opcheck, graph replay, a generic (int8) inner weight, and the
observer's search against the reference's chosen scales.

Shapes whose K the issue's list gives as no multiple of the group size are rounded up to one, as
tests/exact_inputs.py does (2080 -> 2112 at 64, 8224 -> 8320 at 128)."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
from conftest import bf16, load_golden

from torchao.kernel import tuning
from torchao.prototype.awq import AWQConfig, AWQObserver
from torchao.quantization import (
    Int4WeightOnlyConfig,
    Int8WeightOnlyConfig,
    WeightTensorWithLinearActivationScaleMetadata,
    quantize_,
)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
TOL_REF = 1e-2   # tests/test_gpu_int4.py
TOL_FP32 = 4e-3
FIXTURES = ["awq_N64_K256_g32.npz", "awq_N96_K1024_g64.npz", "awq_N48_K512_g128.npz"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _from_bits(v):
    return torch.tensor(np.asarray(v, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def assert_same_bf16(got, want, what):
    """torch.equal on the bit patterns, with NaN compared as NaN (torch.equal is false for any NaN;
    the payload of a NaN is not pinned)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.bfloat16, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ at {(gn != wn).nonzero()[:6].tolist()}"
    g = torch.where(gn, torch.zeros_like(got), got)
    w = torch.where(wn, torch.zeros_like(want), want)
    bad = (_bits(g) != _bits(w)).nonzero()
    assert bad.numel() == 0, (
        f"{what}: {bad.shape[0]} differ, first {bad[:6].tolist()}: got "
        f"{[hex(int(_bits(got)[tuple(i)]) & 0xFFFF) for i in bad[:6]]} want "
        f"{[hex(int(_bits(want)[tuple(i)]) & 0xFFFF) for i in bad[:6]]}")


# ---- act_prescale against torch -----------------------------------------------------------------
SPECIAL_X = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x007F, 0x8003, 0x7F7F, 0xFF7F, 0x0080,
             0x3F80, 0xC2C8]
# 1e-4, 0, inf, nan, subnormals, -1e-4, the smallest normal, the largest finite, 1, a large one
SPECIAL_S = [0x38D2, 0x0000, 0x7F80, 0x7FC0, 0x0001, 0x0040, 0xB8D2, 0x0080, 0x7F7F, 0x3F80, 0x4F00,
             0x8000, 0x38D2, 0x38D2, 0x0002, 0x3F80]


def _prescale_inputs(M, K):
    g = torch.Generator().manual_seed(M * 7 + K)
    x = (torch.randn(M, K, generator=g) * 3).to(torch.bfloat16)
    s = (0.05 + 20 * torch.rand(K, generator=g)).to(torch.bfloat16)
    sx, ss = _from_bits(SPECIAL_X), _from_bits(SPECIAL_S)
    s[:16] = ss
    s[100] = 1e-4
    for m in range(M):
        # every special x over every special scale (13 and 16 are coprime), and over ordinary ones
        x[m, :16] = sx[(torch.arange(16) + m * 16) % len(sx)]
        x[m, 16:K:5] = sx[(torch.arange(len(range(16, K, 5))) + m) % len(sx)]
        x[m, 100] = _from_bits([0x7F7F, 0xFF7F, 0x4F00])[m % 3]  # overflows over 1e-4
    return x, s


@pytest.mark.parametrize("K", [352, 2080])
@pytest.mark.parametrize("M", [1, 3, 70])
def test_act_prescale_equals_torch_division(M, K):
    x, s = _prescale_inputs(M, K)
    xd, sd = x.to(DEV), s.to(DEV)
    got = T.act_prescale(xd, sd)
    assert got.shape == x.shape and got.dtype == torch.bfloat16
    assert_same_bf16(got, xd / sd, f"act_prescale vs torch on the GPU M={M} K={K}")
    assert_same_bf16(got, x / s, f"act_prescale vs torch on the CPU M={M} K={K}")
    # leading dimensions, and an input that is a strided view
    if M == 70:
        y3 = T.act_prescale(xd.view(7, 10, K), sd)
        assert y3.shape == (7, 10, K)
        assert_same_bf16(y3.view(M, K), got, "3-D input")
        wide = torch.zeros(M, K + 8, dtype=torch.bfloat16, device=DEV)
        wide[:, 8:] = xd
        assert_same_bf16(T.act_prescale(wide[:, 8:], sd), got, "strided input")


def test_ops_refuse_other_dtypes():
    x = torch.ones(2, 64, device=DEV)
    s = torch.ones(64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bf16"):
        T.act_prescale(x, s)
    with pytest.raises(RuntimeError, match="bf16"):
        T.act_prescale(x.bfloat16(), s.float())
    packed, sz = _weight(8, 64, 32, 0)
    with pytest.raises(RuntimeError, match="bf16"):
        T.int4_prescaled_linear(x, s, packed, sz, 32, None)
    with pytest.raises(RuntimeError, match="bf16"):
        T.int4_prescaled_linear(x.half(), s, packed, sz, 32, None)
    with pytest.raises(RuntimeError):
        T.act_prescale(x.bfloat16(), s[:32])


# ---- the fused one-token op ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weight(N, K, g, seed):
    gen = torch.Generator().manual_seed(seed * 131 + N + K)
    q = torch.randint(0, 16, (N, K), generator=gen, dtype=torch.int32)
    s = (0.002 + 0.01 * torch.rand(N, K // g, generator=gen)).to(torch.bfloat16)
    z = (0.05 * torch.randn(N, K // g, generator=gen)).to(torch.bfloat16)
    return T.int4_pack(q.to(DEV)), torch.stack([s, z], -1).contiguous().to(DEV)


def _acts(M, K, seed):
    gen = torch.Generator().manual_seed(seed * 17 + M + K)
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16).to(DEV)
    s = (0.1 + 4 * torch.rand(K, generator=gen)).to(torch.bfloat16).to(DEV)
    return x, s


def _one_launch(x, s, packed, sz, g):
    """tao_int4wo_prescaled_linear_bf16 itself (the op routes K > 4096 to the two launches)."""
    from torchao import _lib

    N, K = packed.shape[0], packed.shape[1] * 8
    y = torch.empty(1, N, dtype=torch.bfloat16, device=DEV)
    _lib.call("tao_int4wo_prescaled_linear_bf16", x.data_ptr(), s.data_ptr(), packed.data_ptr(),
              sz.data_ptr(), None, y.data_ptr(), 1, N, K, g,
              torch.cuda.current_stream().cuda_stream)
    assert _lib.lib().tao_last_kernel().decode() == "int4wo_gemv_prescale_kernel"
    return y


def _two_step(x, s, packed, sz, g, bias=None):
    return T.int4_weight_only_linear(T.act_prescale(x, s), packed, sz, g, bias)


FUSED = [(40, 352, 32), (37, E.round_up(2080, 64), 64), (24, E.round_up(8224, 128), 128),
         (16, 16384, 256)]


@pytest.mark.parametrize("N,K,g", FUSED)
def test_fused_one_token_equals_two_launches_on_the_same_shape(N, K, g):
    """One launch == act_prescale then the plain linear with x staged in LDS (tao_tune_int4_xlds 1:
    the same launch shape, so the same summation order), bit for bit."""
    from torchao import _lib

    packed, sz = _weight(N, K, g, 1)
    x, s = _acts(1, K, 1)
    with tuning(int4_xlds=1):  # resets the tuning in its finally
        got = _one_launch(x, s, packed, sz, g)
        want = _two_step(x, s, packed, sz, g)
        torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max()
    if not _lib.lib().tao_int4wo_prescaled_linear_fused(1, N, K, 0):
        # K > 4096: the op takes the two launches (test_one_token_routing)
        assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, g, None),
                           _two_step(x, s, packed, sz, g))
        return
    # the op takes that launch; leading dimensions: a [1, 1, K] and a [K] token take it too
    with tuning(int4_xlds=1):
        assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, g, None), want)
        assert _lib.lib().tao_last_kernel().decode() == "int4wo_gemv_prescale_kernel"
        assert torch.equal(T.int4_prescaled_linear(x.view(1, 1, K), s, packed, sz, g, None),
                           want.view(1, 1, N))
        assert torch.equal(T.int4_prescaled_linear(x.view(K), s, packed, sz, g, None), want.view(N))


def test_one_token_past_the_prologue_limit_takes_two_launches():
    N, K, g = 9, 16416, 32
    packed, sz = _weight(N, K, g, 2)
    x, s = _acts(1, K, 2)
    assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, g, None),
                       _two_step(x, s, packed, sz, g))
    from torchao import _lib

    y = torch.empty(1, N, dtype=torch.bfloat16, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="K <= 16384"):
        _lib.call("tao_int4wo_prescaled_linear_bf16", x.data_ptr(), s.data_ptr(), packed.data_ptr(),
                  sz.data_ptr(), None, y.data_ptr(), 1, N, K, g, st)
    with pytest.raises(RuntimeError, match="one token"):
        _lib.call("tao_int4wo_prescaled_linear_bf16", x.data_ptr(), s.data_ptr(), packed.data_ptr(),
                  sz.data_ptr(), None, y.data_ptr(), 2, N, 352, g, st)


def test_one_token_routing():
    """The op takes the one launch up to K = 4096 and N * K = 2^24 weights, the two launches past
    either (where they measured faster: experiments/bench_awq.py); either way the numbers are
    those of its route's two-step form."""
    from torchao import _lib

    fused = _lib.lib().tao_int4wo_prescaled_linear_fused
    assert fused(1, 4096, 4096, 0) == 1 and fused(1, 4104, 4096, 0) == 0
    assert fused(1, 16, 4128, 0) == 0
    g = 32
    for N, K, one in ((4096, 4096, True), (4104, 4096, False), (16, 4128, False)):
        x, s = _acts(1, K, 9)
        packed, sz = _weight(N, K, g, 9)
        got = T.int4_prescaled_linear(x, s, packed, sz, g, None)
        last = _lib.lib().tao_last_kernel().decode()
        assert (last == "int4wo_gemv_prescale_kernel") == one, (N, last)
        with tuning(int4_xlds=1 if one else 0):
            assert torch.equal(got, _two_step(x, s, packed, sz, g))


@pytest.mark.parametrize("N,K,g", FUSED[:2])
def test_one_token_with_a_bias_equals_the_two_steps(N, K, g):
    packed, sz = _weight(N, K, g, 3)
    x, s = _acts(1, K, 3)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(DEV)
    assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, g, bias),
                       _two_step(x, s, packed, sz, g, bias))
    with tuning(int4_xlds=1):
        assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, g, bias),
                           _two_step(x, s, packed, sz, g, bias))


@pytest.mark.parametrize("N,K", [(200, 352), (72, 1056)])
@pytest.mark.parametrize("M", [2, 3, 5, 17, 70])
def test_more_tokens_equal_the_two_steps(M, N, K):
    packed, sz = _weight(N, K, 32, 4)
    x, s = _acts(M, K, 4)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16).to(DEV)
    for b in (None, bias):
        assert torch.equal(T.int4_prescaled_linear(x, s, packed, sz, 32, b),
                           _two_step(x, s, packed, sz, 32, b))


# ---- opcheck, graph replay ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5])
def test_opcheck(M):
    packed, sz = _weight(40, 352, 32, 7)
    x, s = _acts(M, 352, 7)
    bias = torch.ones(40, dtype=torch.bfloat16, device=DEV)
    torch.library.opcheck(T.act_prescale.default, (x, s))
    torch.library.opcheck(T.int4_prescaled_linear.default, (x, s, packed, sz, 32, None))
    torch.library.opcheck(T.int4_prescaled_linear.default, (x, s, packed, sz, 32, bias))


def test_graph_replay_of_the_one_token_op():
    N, K, g = 37, 2112, 64
    packed, sz = _weight(N, K, g, 8)
    x, s = _acts(1, K, 8)
    want = T.int4_prescaled_linear(x, s, packed, sz, g, None).clone()  # eager warm-up
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = T.int4_prescaled_linear(x, s, packed, sz, g, None)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ---- module level ------------------------------------------------------------------------------------
def _float_linear(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    return lin.to(DEV)


@functools.lru_cache(maxsize=None)
def _observed(name, n):
    """The observer of fixture `name` after calibration and a search over n candidates, with the
    scale it returned; made once and shared (never modified)."""
    rec = load_golden(name)
    lin = _float_linear(rec)
    obs = AWQObserver(lin.weight, lin.bias, Int4WeightOnlyConfig(group_size=int(rec["g"])), n)
    obs(bf16(rec["calib"]).to(DEV), None)
    with torch.no_grad():
        scale = obs.calculate_qparams()
    return obs, scale


@functools.lru_cache(maxsize=None)
def _converted(name):
    """prepare -> calibrate -> convert through quantize_, 5 candidates."""
    rec = load_golden(name)
    model = torch.nn.Sequential(_float_linear(rec))
    base = Int4WeightOnlyConfig(group_size=int(rec["g"]))
    quantize_(model, AWQConfig(base, step="prepare", scale_search_space_size=5))
    with torch.no_grad():
        model(bf16(rec["calib"]).to(DEV))
    quantize_(model, AWQConfig(base, step="convert", scale_search_space_size=5))
    return model


def _rel_l2(y, ref):
    y, ref = y.detach().cpu().double(), ref.double()
    return float((y - ref).norm() / ref.norm())


@pytest.mark.parametrize("name", FIXTURES)
def test_converted_module_against_the_reference(name):
    rec = load_golden(name)
    model = _converted(name)
    w = model[0].weight
    assert type(model[0]) is torch.nn.Linear
    assert isinstance(w, WeightTensorWithLinearActivationScaleMetadata)
    assert torch.equal(w.scale.cpu(), bf16(rec["scale_5"]))
    q, s, z = w.original_weight_tensor.tensor_impl.get_plain()
    assert torch.equal(q.cpu(), torch.from_numpy(rec["q"].astype("int32")))
    assert torch.equal(s.cpu(), bf16(rec["s"])) and torch.equal(z.cpu(), bf16(rec["z"]))
    x = bf16(rec["x"]).to(DEV)
    with torch.no_grad():
        y = model(x)
        by_hand = F.linear(x / w.scale, w.original_weight_tensor, model[0].bias)
        one = model(x[:1])
    e_ref, e64 = _rel_l2(y, bf16(rec["y_ref"])), _rel_l2(y, torch.from_numpy(rec["y64"]))
    print(f"{name}: rel-L2 vs the reference's forward {e_ref:.3e}, vs float64 {e64:.3e}")
    assert e_ref <= TOL_REF
    assert e64 <= TOL_FP32
    assert torch.equal(y, by_hand)
    # one token takes the fused launch (with a bias: the two launches); same numbers within TOL
    assert _rel_l2(one, torch.from_numpy(rec["y64"][:1])) <= TOL_FP32


@pytest.mark.parametrize("name", FIXTURES)
def test_awq_halves_the_error_of_plain_int4(name):
    """The point of the feature: on the calibration tokens the mean squared error against the float
    linear of the 5-candidate AWQ module is at most half that of plain Int4WeightOnlyConfig (the
    fixture's inputs give the reference a factor of 3)."""
    rec = load_golden(name)
    calib = bf16(rec["calib"]).to(DEV)
    flt = _float_linear(rec)
    plain = torch.nn.Sequential(_float_linear(rec))
    quantize_(plain, Int4WeightOnlyConfig(group_size=int(rec["g"])))
    with torch.no_grad():
        ref = flt(calib).double()
        mse_awq = float((_converted(name)(calib).double() - ref).pow(2).mean())
        mse_plain = float((plain(calib).double() - ref).pow(2).mean())
    print(f"{name}: mse plain int4 {mse_plain:.4e}, awq {mse_awq:.4e}, "
          f"ratio {mse_plain / mse_awq:.2f}")
    assert mse_awq <= 0.5 * mse_plain


def test_generic_inner_weight_goes_through_act_prescale():
    """Int8WeightOnlyConfig as the base config: act_prescale, then the int8 weight-only linear,
    equal to the hand-done form bit for bit, at one and at several tokens."""
    rec = load_golden(FIXTURES[0])
    model = torch.nn.Sequential(_float_linear(rec))
    base = Int8WeightOnlyConfig()
    quantize_(model, AWQConfig(base, step="prepare", scale_search_space_size=3))
    with torch.no_grad():
        model(bf16(rec["calib"]).to(DEV))
    quantize_(model, AWQConfig(base, step="convert", scale_search_space_size=3))
    w = model[0].weight
    assert isinstance(w, WeightTensorWithLinearActivationScaleMetadata)
    assert w.original_weight_tensor.tensor_impl.int_data.dtype == torch.int8
    x = bf16(rec["x"]).to(DEV)
    with torch.no_grad():
        for xs in (x, x[:1]):
            y = model(xs)
            assert torch.equal(y, F.linear(xs / w.scale, w.original_weight_tensor, model[0].bias))
            assert torch.equal(y, F.linear(T.act_prescale(xs, w.scale), w.original_weight_tensor,
                                           model[0].bias))
        ref = F.linear(x, bf16(rec["w"]).to(DEV), model[0].bias)
    assert _rel_l2(model(x), ref.cpu()) < 2e-2


# ---- the observer's search ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("name", FIXTURES)
def test_search_returns_the_reference_scale(name, n):
    """3 and 5 candidates: the candidate vectors are bf16 and deterministic, the fixture's inputs
    put the minimum 1.3 times or more clear of the runner-up, the bf16 loss resolves 0.4 %."""
    rec = load_golden(name)
    obs, scale = _observed(name, n)
    assert scale.dtype == torch.bfloat16 and tuple(scale.shape) == (int(rec["K"]),)
    assert len(obs.losses) == n and all(type(v) is float for v in obs.losses)
    print(f"{name} n={n}: losses {obs.losses} reference {rec[f'losses_{n}'].tolist()}")
    assert obs.losses.index(min(obs.losses)) == int(rec[f"index_{n}"])
    assert torch.equal(scale.cpu(), bf16(rec[f"scale_{n}"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_search_over_20_candidates_is_as_good_as_the_reference(name):
    """The loss curve is flat near its minimum at 20 candidates, so the argmin is not pinned. The
    returned scale is one of the 20 candidates; with d = max_i |losses[i] / reference loss[i] - 1|,
    the reference loss of the chosen candidate is at most (1 + d) / (1 - d) times the reference's
    minimum (both tables rank their own minimum first)."""
    n = 20
    rec = load_golden(name)
    obs, scale = _observed(name, n)
    mean = bf16(rec["calib"]).to(DEV).abs().view(-1, int(rec["K"])).mean(0)
    cands = []
    for i in range(n):
        s = mean.pow(i / n).to(torch.bfloat16).clamp(min=1e-4).view(-1)
        cands.append(s / (s.max() * s.min()).sqrt())
    hits = [i for i, c in enumerate(cands) if torch.equal(c, scale)]
    assert hits, "the returned scale is none of the 20 candidates"
    ref = rec["losses_20"]
    ours = np.asarray(obs.losses)
    assert len(ours) == n
    d = float(np.abs(ours / ref - 1).max())
    chosen = hits[0]
    print(f"{name}: d = {d:.4f}; chosen candidate {chosen} (reference {int(rec['index_20'])}), "
          f"reference loss there {ref[chosen]:.6g} vs its minimum {ref.min():.6g}")
    assert d < 1
    assert ref[chosen] <= (1 + d) / (1 - d) * ref.min()
