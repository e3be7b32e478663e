"""GPU tests of the blockwise float8 inference linear (csrc/block_fp8.hip, the BlockFp8 policy of
csrc/gemm_mfma_policy.h, torchao.prototype.blockwise_fp8_inference) against the fixtures of
experiments/gen_golden_blockfp8.py and the plain-torch CPU functions: the quantizers byte for byte,
the scale mapping of the MFMA route and of the GEMV on exact inputs, the ops against the float64
formula on the fixture codes, K and N tails with guarded scale buffers, the module, opcheck, the
argument errors and the quantize-dequantize round trip."""

import numpy as np
import pytest
import torch

from conftest import bf16, golden_files, load_golden

from torchao import _lib
from torchao.kernel import tuning
from torchao.prototype.blockwise_fp8_inference import (
    BlockwiseQuantLinear,
    blockwise_fp8_gemm,
    fp8_blockwise_act_quant,
    fp8_blockwise_weight_dequant,
    fp8_blockwise_weight_quant,
)

pytestmark = pytest.mark.gpu
DEV = "cuda"
E4 = torch.float8_e4m3fn
FIXTURES = golden_files("blockfp8_N")
BAR = 4e-3  # the project's bar against float64 on the same codes
T = torch.ops.torchao
# how each route is reached; the GEMV serves M <= 8 at most (tao_tune_linear_crossover)
ROUTES = {"built-in": {}, "mfma": {"blockfp8_mfma": 1}, "gemv": {"linear_crossover": 8}}


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


def _rel_l2(y, y64):
    return float((y.double().cpu() - y64).norm() / y64.norm())


def _route_kernel(route, M, N, K):
    """The kernel family a scaled mm of this shape must report (fp8_dyn_host.h's rule)."""
    if route == "mfma":
        return "gemm_mfma"
    if route == "gemv":
        return "blockfp8_gemv"
    return "blockfp8_gemv" if M <= 1 or (M <= 4 and N * K <= (32 << 20)) else "gemm_mfma"


def _y64(xq, xs, wq, ws, bias=None):
    """The formula of csrc/block_fp8.hip in float64 on uint8 codes and fp32 scales (CPU)."""
    N, K = wq.shape
    xf = xq.view(E4).double().reshape(-1, K // 128, 128)
    wf = wq.view(E4).double().reshape(N, K // 128, 128)
    P = torch.einsum("mbk,nbk->mnb", xf, wf)
    f = xs.double().reshape(-1, 1, K // 128) * ws.double().repeat_interleave(128, 0)[:N][None]
    y = (P * f).sum(-1)
    return y if bias is None else y + bias.double()[None, :]


def _assert_codes(q, ref, what=""):
    """NaN codes compare as "is NaN"; every other byte must be equal."""
    q = _u8(q).cpu().numpy()
    ref = np.asarray(ref)
    nan = (ref & 0x7F) == 0x7F
    assert bool(((q & 0x7F) == 0x7F)[nan].all()), what
    assert np.array_equal(q[~nan], ref[~nan]), what


def _operands(rec):
    return (torch.from_numpy(rec["xq"]).view(E4).to(DEV), torch.from_numpy(rec["xs"]).to(DEV),
            torch.from_numpy(rec["wq"]).view(E4).to(DEV), torch.from_numpy(rec["ws"]).to(DEV),
            bf16(rec["bias"]).to(DEV))


# ---- quantizers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", FIXTURES)
def test_quantizers_match_the_fixtures(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    wq, ws = T.blockfp8_quantize_weight(bf16(rec["w"]).to(DEV))
    assert _last_kernel() == "blockfp8_quantize_weight_kernel"
    xq, xs = T.blockfp8_quantize_act(bf16(rec["x"]).to(DEV))
    assert _last_kernel() == "blockfp8_quantize_act_kernel"
    assert wq.dtype is E4 and xq.dtype is E4
    assert ws.dtype is torch.float32 and ws.shape == ((N + 127) // 128, K // 128)
    assert xs.dtype is torch.float32 and xs.shape == (5, K // 128)
    _assert_codes(wq, rec["wq"], (fname, "wq"))
    _assert_codes(xq, rec["xq"], (fname, "xq"))
    assert np.array_equal(ws.cpu().numpy(), rec["ws"]), fname
    assert np.array_equal(xs.cpu().numpy(), rec["xs"]), fname


def test_quantizer_edge_blocks_random_rows_and_leading_dimensions():
    rec = load_golden("blockfp8_quant_edges.npz")
    x = bf16(rec["x"])
    q, s = T.blockfp8_quantize_act(x.to(DEV))
    _assert_codes(q, rec["q"], "edges")
    assert np.array_equal(s.cpu().numpy(), rec["s"])  # inf == inf; no NaN scale in the file
    # the same rows as a ragged weight tile: one amax over the 6 rows per k block
    wq_cpu, ws_cpu = fp8_blockwise_weight_quant(x)
    wq, ws = T.blockfp8_quantize_weight(x.to(DEV))
    _assert_codes(wq, _u8(wq_cpu).numpy(), "edges as a weight")
    assert np.array_equal(ws.cpu().numpy(), ws_cpu.numpy())
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(33, 2176, generator=g) * torch.exp2(torch.randint(-20, 20, (33, 1), generator=g))
         ).to(torch.bfloat16)
    q_cpu, s_cpu = fp8_blockwise_act_quant(x)
    q, s = fp8_blockwise_act_quant(x.to(DEV))  # the Python function calls the op on a HIP tensor
    assert _last_kernel() == "blockfp8_quantize_act_kernel"
    assert torch.equal(s.cpu(), s_cpu) and torch.equal(_u8(q).cpu(), _u8(q_cpu))
    q3, s3 = T.blockfp8_quantize_act(x[:32].reshape(4, 8, 2176).to(DEV))
    assert q3.shape == (4, 8, 2176) and s3.shape == (4, 8, 17)
    assert torch.equal(_u8(q3).cpu().reshape(32, -1), _u8(q_cpu)[:32])
    assert torch.equal(s3.cpu().reshape(32, -1), s_cpu[:32])
    # a weight [272, 384] with rows of very different magnitude: ragged N, 3 scale rows
    w = (torch.randn(272, 384, generator=g) * torch.exp2(torch.randint(-20, 20, (272, 1), generator=g))
         ).to(torch.bfloat16)
    wq_cpu, ws_cpu = fp8_blockwise_weight_quant(w)
    wq, ws = fp8_blockwise_weight_quant(w.to(DEV))
    assert _last_kernel() == "blockfp8_quantize_weight_kernel"
    assert ws.shape == (3, 3) and torch.equal(ws.cpu(), ws_cpu)
    assert torch.equal(_u8(wq).cpu(), _u8(wq_cpu))


def test_dequant_and_round_trip():
    rec = load_golden("blockfp8_N272_K384.npz")
    wq, ws = torch.from_numpy(rec["wq"]).view(E4), torch.from_numpy(rec["ws"])
    want = fp8_blockwise_weight_dequant(wq, ws)
    d = fp8_blockwise_weight_dequant(wq.to(DEV), ws.to(DEV))
    assert _last_kernel() == "blockfp8_dequant_weight_kernel"
    assert d.dtype is torch.float32 and torch.equal(d.cpu(), want)
    d16 = T.blockfp8_dequantize_weight(wq.to(DEV), ws.to(DEV), True)
    assert d16.dtype is torch.bfloat16 and torch.equal(_bits(d16.cpu()), _bits(want.to(torch.bfloat16)))
    # the reference test's own criterion: rel-L2 < 0.1 on randn
    g = torch.Generator().manual_seed(0)
    x = torch.randn(512, 128, generator=g).to(torch.bfloat16).to(DEV)
    q, s = fp8_blockwise_weight_quant(x)
    assert q.shape == (512, 128) and s.shape == (4, 1)
    back = fp8_blockwise_weight_dequant(q, s)
    e = float((back.double() - x.double()).norm() / x.double().norm())
    print(f"quantize-dequantize round trip [512, 128]: rel-L2 {e:.3e}")
    assert e < 0.1


# ---- scale mapping, exact ------------------------------------------------------------------------
def _exact_case(M, N, K, all_live):
    """Scaled mm operands: every x and w code is 1.0 (0x38) and every scale a power of two,
    2^a(m, b) for x and 2^c(n / 128, b) for w.
      (a) all_live False: token m is zero outside block b0(m), so y[m][n] = 128 * 2^(a + c) of that
          block exactly, a power of two within bf16: a scale taken from the wrong row, lane, n-block
          or k-block gives another power of two.
      (b) all_live True: every block is live and a + c spans at most 12 binades, so every fp32 sum
          of the terms (and of the 16-code partial sums of the GEMV) is exact in any order and y is
          bf16(float64 sum) bit for bit.
    The bf16 activation of the dyn_linear leg cannot quantize to all-1.0 codes (the block's amax
    becomes 448), so a live block of it is [448, 64, 64, ...] * 2^a: it quantizes to the codes
    [0x7E, 0x68, 0x68, ...] with the scale 2^a exactly, P = 448 + 127 * 64 = 67 * 128 (7 significant
    bits: with 12 binades and up to 8 blocks still exact in fp32), and the quantizer's bytes are
    checked on the way."""
    nblk, NB = K // 128, (N + 127) // 128
    m, nb, b = torch.arange(M)[:, None], torch.arange(NB)[:, None], torch.arange(nblk)[None, :]
    if all_live:
        a = (7 * m + 3 * b) % 7 - 3
        c = (5 * nb + 11 * b) % 7 - 3
        live = torch.ones(M, nblk, dtype=torch.bool)
    else:
        a = (7 * m + 3 * b) % 13 - 6
        c = (5 * nb + 11 * b) % 17 - 8
        live = torch.zeros(M, nblk, dtype=torch.bool)
        live[torch.arange(M), (5 * torch.arange(M) + 3) % nblk] = True
    xs, ws = torch.exp2(a.float()), torch.exp2(c.float())
    xq = torch.zeros(M, nblk, 128, dtype=torch.uint8)
    xq[live] = 0x38
    wq = torch.full((N, K), 0x38, dtype=torch.uint8)
    blk = torch.full((128,), 64.0, dtype=torch.float64)
    blk[0] = 448.0
    x = torch.where(live[..., None], xs.double()[..., None] * blk, torch.zeros(1, dtype=torch.float64))
    xq_dyn = torch.zeros(M, nblk, 128, dtype=torch.uint8)
    xq_dyn[live] = 0x68
    xq_dyn[..., 0][live] = 0x7E
    cn = c.repeat_interleave(128, 0)[:N]  # [N, nblk]
    e = torch.where(live[:, None, :], torch.exp2((a[:, None, :] + cn[None]).double()),
                    torch.zeros(1, dtype=torch.float64)).sum(-1)
    # zero scales where the token's block is dead: what the quantizer stores for an all-zero block
    xs_dyn = torch.where(live, xs, torch.zeros(1))
    return dict(xq=xq.reshape(M, K), xs=xs.contiguous(), wq=wq, ws=ws.contiguous(),
                want=(128.0 * e).to(torch.bfloat16), x=x.reshape(M, K).to(torch.bfloat16),
                xq_dyn=xq_dyn.reshape(M, K), xs_dyn=xs_dyn.contiguous(),
                want_dyn=(8576.0 * e).to(torch.bfloat16), e=e)


@pytest.mark.parametrize("K", (128, 384, 1024))
@pytest.mark.parametrize("N", (40, 272))
@pytest.mark.parametrize("M", (1, 5, 16, 33, 130))
def test_scale_mapping_exact(M, N, K):
    for all_live in (False, True):
        c = _exact_case(M, N, K, all_live)
        # the test's own algebra, on the CPU
        y64 = _y64(c["xq"], c["xs"], c["wq"], c["ws"])
        assert torch.equal(y64, 128.0 * c["e"]) and torch.equal(y64.to(torch.bfloat16), c["want"])
        if not all_live:  # a power of two within bf16
            assert torch.equal(c["want"].double(), y64) and bool((torch.frexp(y64)[0] == 0.5).all())
        q_cpu, s_cpu = fp8_blockwise_act_quant(c["x"])
        assert torch.equal(_u8(q_cpu), c["xq_dyn"]) and torch.equal(s_cpu, c["xs_dyn"])
        y64d = _y64(c["xq_dyn"], c["xs_dyn"], c["wq"], c["ws"])
        assert torch.equal(y64d, 8576.0 * c["e"])
        xq, xs, wq, ws, x = (t.to(DEV) for t in (c["xq"].view(E4), c["xs"], c["wq"].view(E4),
                                                 c["ws"], c["x"]))
        q, s = T.blockfp8_quantize_act(x)
        assert torch.equal(_u8(q).cpu(), c["xq_dyn"]) and torch.equal(s.cpu(), c["xs_dyn"])
        for route, knobs in ROUTES.items():
            if route == "gemv" and M > 8:
                continue
            with tuning(**knobs):
                y = T.blockfp8_scaled_mm(xq, xs, wq, ws, None)
                k = _last_kernel()
                yd = T.blockfp8_dyn_linear(x, wq, ws, None)
                kd = _last_kernel()
            assert _route_kernel(route, M, N, K) in k, (route, k)
            # one token is always the one-launch GEMV; more are quantizer -> the route's scaled mm
            assert ("blockfp8_gemv" if M == 1 else _route_kernel(route, M, N, K)) in kd, (route, kd)
            bad = (_bits(y.cpu()) != _bits(c["want"])).nonzero()
            assert bad.numel() == 0, (all_live, route, k, bad[:8].tolist(),
                                      y.cpu()[tuple(bad[0])].item(),
                                      c["want"][tuple(bad[0])].item())
            bad = (_bits(yd.cpu()) != _bits(c["want_dyn"])).nonzero()
            assert bad.numel() == 0, (all_live, route, kd, "dyn", bad[:8].tolist(),
                                      yd.cpu()[tuple(bad[0])].item(),
                                      c["want_dyn"][tuple(bad[0])].item())
    if M == 1:  # leaving tuning() called tao_tune_reset: the forced MFMA route is cleared
        T.blockfp8_scaled_mm(xq, xs, wq, ws, None)
        assert _last_kernel() == "blockfp8_gemv_kernel"


# ---- fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", tuple(ROUTES))
@pytest.mark.parametrize("fname", FIXTURES)
def test_ops_against_float64_on_the_fixture_codes(fname, route):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    y64 = torch.from_numpy(rec["y64"])
    zt = int(rec["zero_token"])
    assert bool(y64.isfinite().all())
    with tuning(**ROUTES[route]):
        y = T.blockfp8_scaled_mm(xq, xs, wq, ws, bias)
        k = _last_kernel()
        y0 = T.blockfp8_scaled_mm(xq, xs, wq, ws, None)
        yd = T.blockfp8_dyn_linear(x, wq, ws, bias)
        y1 = torch.cat([T.blockfp8_scaled_mm(xq[m:m + 1], xs[m:m + 1], wq, ws, bias)
                        for m in range(5)])
        k1 = _last_kernel()
        yg = blockwise_fp8_gemm(xq, xs, wq, ws)  # the reference-named function calls the same op
    assert _route_kernel(route, 5, N, K) in k, k
    assert _route_kernel(route, 1, N, K) in k1, k1
    e, e0, e1 = _rel_l2(y, y64), _rel_l2(y0, y64 - bf16(rec["bias"]).double()), _rel_l2(y1, y64)
    print(f"{fname} {route} {k}: rel-L2 vs float64 M=5 {e:.3e} no bias {e0:.3e} M=1 x5 {e1:.3e}")
    assert e <= BAR and e0 <= BAR and e1 <= BAR
    # the all-zero token: exactly bf16(bias), exactly 0 without it
    assert torch.equal(_bits(y[zt]), _bits(bias)) and torch.equal(_bits(y1[zt]), _bits(bias))
    assert not y0[zt].any() and not y0[zt].isnan().any()
    assert torch.equal(_bits(yg), _bits(y0))
    # the whole linear from bf16 equals quantizer -> scaled mm
    assert torch.equal(_bits(yd), _bits(y))


@pytest.mark.parametrize("fname", FIXTURES)
def test_one_launch_is_bit_identical_to_quantizer_then_scaled_mm(fname):
    rec = load_golden(fname)
    _, _, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    for m in range(5):
        for b in (bias, None):
            yd = T.blockfp8_dyn_linear(x[m:m + 1], wq, ws, b)
            assert _last_kernel() == "blockfp8_gemv_kernel"
            q, s = T.blockfp8_quantize_act(x[m:m + 1])
            assert torch.equal(_u8(q).cpu(), torch.from_numpy(rec["xq"][m:m + 1]))
            y = T.blockfp8_scaled_mm(q, s, wq, ws, b)
            assert _last_kernel() == "blockfp8_gemv_kernel"
            assert torch.equal(_bits(yd), _bits(y)), (fname, m)


# ---- tails -----------------------------------------------------------------------------------------
def _guarded(scales):
    """The scales inside a larger allocation filled with NaN on both sides: a read outside the
    array shows as NaN in the output and does not fault."""
    n = scales.numel()
    buf = torch.full((64 + n + 4096,), float("nan"), dtype=torch.float32, device=DEV)
    buf[64:64 + n] = scales.reshape(-1).to(DEV)
    return buf[64:64 + n].view(scales.shape)


@pytest.mark.parametrize("N", (1, 17, 40, 129))
@pytest.mark.parametrize("K", (128, 384, 2176))
def test_tails_with_guarded_scale_buffers(K, N):
    g = torch.Generator().manual_seed(K + N)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    x = torch.randn(33, K, generator=g).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    wq, ws = fp8_blockwise_weight_quant(w)
    xq, xs = fp8_blockwise_act_quant(x)
    y64 = _y64(_u8(xq), xs, _u8(wq), ws, bias)
    wq_d, ws_d, bias_d = wq.to(DEV), _guarded(ws), bias.to(DEV)
    for M, route in ((1, "built-in"), (1, "mfma"), (5, "gemv"), (5, "mfma"), (33, "built-in")):
        xs_d = _guarded(xs[:M])  # the first and the last token's scales border the guards
        with tuning(**ROUTES[route]):
            y = T.blockfp8_scaled_mm(xq[:M].to(DEV), xs_d, wq_d, ws_d, bias_d)
            k = _last_kernel()
        assert _route_kernel(route, M, N, K) in k, (route, k)
        assert not bool(y.isnan().any()) and bool(y.isfinite().all()), (M, route, k)
        e = _rel_l2(y, y64[:M])
        print(f"K={K} N={N} M={M} {route} {k}: {e:.3e}")
        assert e <= BAR, (M, route, k, e)
    yd = T.blockfp8_dyn_linear(x[:1].to(DEV), wq_d, ws_d, bias_d)
    assert bool(yd.isfinite().all()) and _rel_l2(yd, y64[:1]) <= BAR


# ---- module ----------------------------------------------------------------------------------------
def test_module_reproduces_the_ops():
    rec = load_golden("blockfp8_N272_K384.npz")
    N, K = 272, 384
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    mod = BlockwiseQuantLinear.from_float(lin.to(DEV))
    assert _last_kernel() == "blockfp8_quantize_weight_kernel"
    assert mod.weight.is_cuda and mod.scale.is_cuda and mod.weight.scale is mod.scale
    assert np.array_equal(_u8(mod.weight).cpu().numpy(), rec["wq"])
    assert np.array_equal(mod.scale.cpu().numpy(), rec["ws"])
    wq, ws, bias = mod.weight.detach(), mod.scale.detach(), mod.bias.detach()
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for x in (torch.randn(2, 3, K, generator=g).to(torch.bfloat16),
                  torch.randn(1, K, generator=g).to(torch.bfloat16)):
            y = mod(x.to(DEV))
            assert y.shape == (*x.shape[:-1], N) and y.dtype is torch.bfloat16
            q, s = T.blockfp8_quantize_act(x.reshape(-1, K).to(DEV))
            want = T.blockfp8_scaled_mm(q, s, wq, ws, bias)
            assert torch.equal(_bits(y.reshape(-1, N)), _bits(want))
            y64 = _y64(_u8(q).cpu(), s.cpu(), _u8(wq).cpu(), ws.cpu(), bias.cpu())
            e = _rel_l2(y.reshape(-1, N), y64)
            print(f"module {tuple(x.shape)}: rel-L2 vs float64 on its own codes {e:.3e}")
            assert e <= BAR
        # a module built on the CPU and moved, loaded from a checkpoint with the reference's keys
        other = BlockwiseQuantLinear(K, N, bias=True)
        other.load_state_dict({k: v.cpu() for k, v in mod.state_dict().items()})
        other = other.to(DEV)
        x = bf16(rec["x"]).to(DEV)
        assert torch.equal(_bits(other(x)), _bits(mod(x)))
        assert _rel_l2(mod(x), torch.from_numpy(rec["y64"])) <= BAR
        with pytest.raises(RuntimeError, match="bf16"):
            mod(torch.zeros(2, K, device=DEV))


# ---- opcheck and refusals --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blockfp8_quantize_act", "blockfp8_quantize_weight",
                                  "blockfp8_dequantize_weight", "blockfp8_scaled_mm",
                                  "blockfp8_dyn_linear"])
def test_opcheck(name):
    rec = load_golden("blockfp8_N272_K384.npz")
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    args = {"blockfp8_quantize_act": (x,), "blockfp8_quantize_weight": (bf16(rec["w"]).to(DEV),),
            "blockfp8_dequantize_weight": (wq, ws, True),
            "blockfp8_scaled_mm": (xq, xs, wq, ws, bias),
            "blockfp8_dyn_linear": (x, wq, ws, bias)}[name]
    op = getattr(T, name).default
    if name in ("blockfp8_quantize_act", "blockfp8_quantize_weight"):
        torch.library.opcheck(op, args)
        return
    # As tests/test_gpu_mx.py::test_opcheck: with float8 inputs opcheck's schema test cannot run (it
    # multiplies its inputs; mul is not implemented for float8), so the other three tests run and
    # input mutation / output aliasing are checked by hand.
    torch.library.opcheck(op, args, test_utils=("test_faketensor", "test_aot_dispatch_dynamic",
                                                "test_autograd_registration"))
    tensors = [a for a in args if isinstance(a, torch.Tensor)]
    before = [a.clone() for a in tensors]
    out = op(*args)
    torch.cuda.synchronize()
    for a, b in zip(tensors, before):
        assert torch.equal(_u8(a) if a.dtype == E4 else a, _u8(b) if b.dtype == E4 else b)
        assert out.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()


def test_argument_refusals():
    rec = load_golden("blockfp8_N272_K384.npz")
    xq, xs, wq, ws, bias = _operands(rec)
    x = bf16(rec["x"]).to(DEV)
    mm, dyn = T.blockfp8_scaled_mm, T.blockfp8_dyn_linear
    qa, qw, dq = T.blockfp8_quantize_act, T.blockfp8_quantize_weight, T.blockfp8_dequantize_weight
    # wrong dtype: bf16 activations and bias, e4m3fn codes, fp32 scales
    with pytest.raises(RuntimeError, match="bf16"):
        dyn(x.float(), wq, ws, bias)
    with pytest.raises(RuntimeError, match="bf16"):
        qa(x.float())
    with pytest.raises(RuntimeError, match="bf16"):
        qw(x.float())
    with pytest.raises(RuntimeError, match="bias must be bfloat16"):
        dyn(x, wq, ws, bias.float())
    with pytest.raises(RuntimeError, match="bias must be bfloat16"):
        mm(xq, xs, wq, ws, bias[:8])
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        mm(_u8(xq), xs, wq, ws, bias)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        dq(_u8(wq), ws, False)
    with pytest.raises(RuntimeError, match="float32"):
        mm(xq, xs, wq, ws.double(), bias)
    with pytest.raises(RuntimeError, match="float32"):
        mm(xq, xs.to(torch.bfloat16), wq, ws, bias)
    # scale shape
    with pytest.raises(RuntimeError, match="128x128 block"):
        mm(xq, xs, wq, ws[:, :2], bias)
    with pytest.raises(RuntimeError, match="128x128 block"):
        dyn(x, wq, ws[:2], bias)
    with pytest.raises(RuntimeError, match="128x128 block"):
        dq(wq, ws.reshape(-1), False)
    with pytest.raises(RuntimeError, match="1x128 block"):
        mm(xq, xs[:3], wq, ws, bias)
    # last dim
    with pytest.raises(RuntimeError, match="last dim"):
        dyn(x[:, :128], wq, ws, bias)
    with pytest.raises(RuntimeError, match="last dim"):
        mm(xq[:, :128], xs[:, :1], wq, ws, bias)
    # device mismatch
    with pytest.raises(RuntimeError, match="same device"):
        dyn(x, wq, ws.cpu(), bias)
    with pytest.raises(RuntimeError, match="same device"):
        mm(xq, xs, wq, ws, bias.cpu())
    # K not a multiple of 128
    with pytest.raises(RuntimeError, match="multiple of 128"):
        qa(x[:, :192].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 128"):
        qw(x[:, :64].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 128"):
        mm(xq[:, :192].contiguous(), xs[:, :1], wq[:, :192].contiguous(), ws[:, :1], None)
    # the Python functions refuse what is not served before reaching the device
    with pytest.raises(NotImplementedError, match="block_size"):
        fp8_blockwise_act_quant(x, 64)
    with pytest.raises(NotImplementedError, match="e5m2"):
        fp8_blockwise_weight_quant(x, 128, torch.float8_e5m2)
    # the C entry of the fused launch is one token
    y = torch.empty(2, 272, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="one token"):
        _lib.call("tao_blockfp8_dyn_linear_bf16", x.data_ptr(), wq.data_ptr(), ws.data_ptr(), None,
                  y.data_ptr(), 2, 272, 384, None)
    # empty batch through the ops
    assert mm(xq[:0], xs[:0], wq, ws, bias).shape == (0, 272)
    assert dyn(x[:0], wq, ws, bias).shape == (0, 272)
    q, s = qa(x[:0])
    assert q.shape == (0, 384) and s.shape == (0, 3)
