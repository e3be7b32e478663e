"""CPU tests of the blockwise float8 inference linear (torchao.prototype.blockwise_fp8_inference):
the plain-torch CPU functions against the fixtures of experiments/gen_golden_blockfp8.py byte for
byte, the ragged weight quantizer, dequantization, the emulated product against float64, the
module (state_dict keys, from_float, load_state_dict, forward), the refusals, the op set and its
fragment, the fake impls and the C-ABI symbols."""

import ctypes

import numpy as np
import pytest
import torch

from conftest import bf16, golden_files, load_golden

from torchao import _lib, ops
from torchao.prototype.blockwise_fp8_inference import (
    BlockwiseQuantLinear,
    blockwise_fp8_gemm,
    fp8_blockwise_act_quant,
    fp8_blockwise_weight_dequant,
    fp8_blockwise_weight_quant,
)

E4 = torch.float8_e4m3fn
FIXTURES = golden_files("blockfp8_N")
BAR = 4e-3  # the project's bar against float64 on the same codes
OPS = {"blockfp8_quantize_act", "blockfp8_quantize_weight", "blockfp8_dequantize_weight",
       "blockfp8_scaled_mm", "blockfp8_dyn_linear"}
ABI = ("tao_blockfp8_quantize_act_bf16", "tao_blockfp8_quantize_weight_bf16",
       "tao_blockfp8_dequant_weight", "tao_blockfp8_scaled_mm_bf16",
       "tao_blockfp8_dyn_linear_bf16", "tao_tune_blockfp8_mfma")


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16)


def assert_codes(q, ref, what=""):
    """NaN codes (S.1111.111) compare as "is NaN"; every other byte must be equal."""
    q = _u8(q).numpy()
    nan = (ref & 0x7F) == 0x7F
    assert bool(((q & 0x7F) == 0x7F)[nan].all()), what
    assert np.array_equal(q[~nan], ref[~nan]), what


def test_fixture_set():
    assert FIXTURES == ["blockfp8_N128_K128.npz", "blockfp8_N272_K384.npz",
                        "blockfp8_N384_K1024.npz"]


@pytest.mark.parametrize("fname", FIXTURES)
def test_cpu_quantizers_reproduce_the_fixtures(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    wq, ws = fp8_blockwise_weight_quant(bf16(rec["w"]))
    xq, xs = fp8_blockwise_act_quant(bf16(rec["x"]))
    assert wq.dtype is E4 and xq.dtype is E4 and ws.dtype is torch.float32
    assert ws.shape == ((N + 127) // 128, K // 128) and xs.shape == (5, K // 128)
    assert ws.is_contiguous() and xs.is_contiguous()
    assert_codes(wq, rec["wq"], (fname, "wq"))
    assert_codes(xq, rec["xq"], (fname, "xq"))
    assert np.array_equal(ws.numpy(), rec["ws"]) and np.array_equal(xs.numpy(), rec["xs"])
    zt, st, sb = int(rec["zero_token"]), int(rec["subnormal_token"]), int(rec["subnormal_block"])
    assert not _u8(xq[zt]).any() and not xs[zt].any()       # zero codes and scale 0, not NaN
    assert 0.0 < float(xs[st, sb]) < 2.0 ** -126            # a subnormal scale, not flushed
    # a float32 input gives the same bytes as its bf16 values
    xq32, xs32 = fp8_blockwise_act_quant(bf16(rec["x"]).float())
    assert torch.equal(_u8(xq32), _u8(xq)) and torch.equal(xs32, xs)


def test_cpu_quantizer_edge_blocks():
    rec = load_golden("blockfp8_quant_edges.npz")
    x = bf16(rec["x"])
    q, s = fp8_blockwise_act_quant(x)
    assert_codes(q, rec["q"])
    assert np.array_equal(s.numpy(), rec["s"])
    q8, ref = _u8(q), rec["q"]
    # NaN in a block: only that element's code is NaN, the scale comes from the rest
    assert int(((ref[0, :128] & 0x7F) == 0x7F).sum()) == 1 and (ref[0, 5] & 0x7F) == 0x7F
    rest = x[0, :128].float().abs()
    rest[5] = 0
    assert float(s[0, 0]) == float(rest.max() / 448.0)
    # +inf: s = inf, the finite elements are zero codes, the infinite one NaN
    assert np.isinf(rec["s"][0, 1]) and (ref[0, 128 + 9] & 0x7F) == 0x7F
    assert not (np.delete(ref[0, 128:], 9) & 0x7F).any()
    # all zero with a -0: scale 0, zero codes, the sign kept
    assert rec["s"][1, 0] == 0 and int(q8[1, 17]) == 0x80 and not np.delete(ref[1, :128], 17).any()
    # all subnormal: a subnormal scale, the amax element at 448 (0x7E)
    assert 0 < rec["s"][1, 1] < 2.0 ** -126 and int(q8[1, 255]) == 0x7E
    # amax exactly 448 and 448 * 2^k
    assert rec["s"][2, 0] == 1.0 and int(q8[2, 3]) == 0x7E
    assert rec["s"][2, 1] == 32.0 and int(q8[2, 128 + 3]) == 0xFE
    assert rec["s"][3, 0] == 2.0 ** -10 and int(q8[3, 1]) == 0x7E
    # NaN and zeros only: amax 0, the NaN stays NaN, zeros stay signed zeros
    assert rec["s"][4, 0] == 0 and (ref[4, 2] & 0x7F) == 0x7F and ref[4, 3] == 0x80
    assert bool(np.isfinite(rec["s"][3, 1]))  # the largest bf16 exponents: a finite scale
    # as a weight the same rows are one ragged 6 x 128 tile per k block: one amax over the rows
    wq, ws = fp8_blockwise_weight_quant(x[1:4])
    assert ws.shape == (1, 2)
    assert float(ws[0, 0]) == 1.0 and float(ws[0, 1]) == float(x[1:4, 128:].float().abs().max() / 448.0)


@pytest.mark.parametrize("N", (1, 127, 129, 272))
def test_cpu_weight_quantizer_ragged_rows(N):
    g = torch.Generator().manual_seed(N)
    w = (torch.randn(N, 256, generator=g) * torch.exp2(torch.randint(-8, 8, (N, 1), generator=g))
         ).to(torch.bfloat16)
    q, s = fp8_blockwise_weight_quant(w)
    NB = (N + 127) // 128
    assert q.shape == (N, 256) and s.shape == (NB, 2)
    for i in range(NB):
        for b in range(2):
            blk = w[i * 128:(i + 1) * 128, b * 128:(b + 1) * 128].float()
            sc = blk.abs().max() / torch.tensor(448.0)
            assert float(s[i, b]) == float(sc)
            assert torch.equal(_u8(q[i * 128:(i + 1) * 128, b * 128:(b + 1) * 128]),
                               _u8((blk / sc).to(E4)))


def test_cpu_dequant_and_round_trip():
    rec = load_golden("blockfp8_N272_K384.npz")
    wq, ws = torch.from_numpy(rec["wq"]).view(E4), torch.from_numpy(rec["ws"])
    d = fp8_blockwise_weight_dequant(wq, ws)
    assert d.dtype is torch.float32 and d.shape == (272, 384)
    want = wq.float() * ws.repeat_interleave(128, 0)[:272].repeat_interleave(128, 1)
    assert torch.equal(d, want)
    w = bf16(rec["w"]).float()
    assert float((d - w).norm() / w.norm()) < 0.1  # the reference test's criterion
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.bfloat16)
        d16 = fp8_blockwise_weight_dequant(wq, ws)
    finally:
        torch.set_default_dtype(old)
    assert d16.dtype is torch.bfloat16 and torch.equal(_bits(d16), _bits(want.to(torch.bfloat16)))


@pytest.mark.parametrize("fname", FIXTURES)
def test_cpu_gemm_against_float64(fname):
    rec = load_golden(fname)
    xq, xs = torch.from_numpy(rec["xq"]).view(E4), torch.from_numpy(rec["xs"])
    wq, ws = torch.from_numpy(rec["wq"]).view(E4), torch.from_numpy(rec["ws"])
    y64 = torch.from_numpy(rec["y64"])
    assert bool(y64.isfinite().all())
    y = blockwise_fp8_gemm(xq, xs, wq, ws)
    assert y.dtype is torch.bfloat16 and y.shape == y64.shape
    ref = y64 - bf16(rec["bias"]).double()
    e = float((y.double() - ref).norm() / ref.norm())
    print(f"{fname}: emulated gemm vs float64 {e:.3e}")
    assert e <= BAR
    assert not y[int(rec["zero_token"])].any()
    y3 = blockwise_fp8_gemm(xq.reshape(5, 1, -1), xs.reshape(5, 1, -1), wq, ws)
    assert y3.shape == (5, 1, wq.shape[0]) and torch.equal(_bits(y3.reshape(y.shape)), _bits(y))


def test_module_state_dict_from_float_and_forward():
    rec = load_golden("blockfp8_N272_K384.npz")
    N, K = 272, 384
    mod = BlockwiseQuantLinear(K, N, bias=True)
    sd = mod.state_dict()
    assert list(sd) == ["weight", "scale", "bias"]
    assert sd["weight"].shape == (N, K) and sd["weight"].dtype is E4
    assert sd["scale"].shape == (3, 3) and sd["scale"].dtype is torch.float32
    assert sd["bias"].shape == (N,)
    assert mod.weight.scale is mod.scale
    assert list(BlockwiseQuantLinear(K, N).state_dict()) == ["weight", "scale"]
    # a checkpoint with the reference's keys (a Hugging Face weight + weight_scale_inv pair)
    ck = {"weight": torch.from_numpy(rec["wq"]).view(E4), "scale": torch.from_numpy(rec["ws"]),
          "bias": bf16(rec["bias"])}
    mod.load_state_dict(ck)
    assert np.array_equal(_u8(mod.weight).numpy(), rec["wq"])
    assert np.array_equal(mod.scale.numpy(), rec["ws"]) and mod.weight.scale is mod.scale
    # from_float quantizes an nn.Linear to the same bytes
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    qm = BlockwiseQuantLinear.from_float(lin)
    assert np.array_equal(_u8(qm.weight).numpy(), rec["wq"])
    assert np.array_equal(qm.scale.numpy(), rec["ws"]) and qm.weight.scale is qm.scale
    assert list(qm.state_dict()) == ["weight", "scale", "bias"]
    assert BlockwiseQuantLinear.from_float(torch.nn.Linear(K, N, bias=False)).bias is None
    # CPU forward: the fixture's codes, so the fixture's float64 product
    x = bf16(rec["x"])
    y64 = torch.from_numpy(rec["y64"])
    for m in (mod, qm):
        y = m(x)
        assert y.dtype is torch.bfloat16 and y.shape == (5, N)
        assert float((y.double() - y64).norm() / y64.norm()) <= BAR
        assert torch.equal(_bits(y[int(rec["zero_token"])]), _bits(bf16(rec["bias"])))
    assert mod(x.reshape(5, 1, K)).shape == (5, 1, N)


def test_refusals():
    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    q, s = fp8_blockwise_act_quant(x)
    wq, ws = fp8_blockwise_weight_quant(x)
    for fn, args in ((fp8_blockwise_act_quant, (x, 64)), (fp8_blockwise_weight_quant, (x, 64)),
                     (fp8_blockwise_weight_dequant, (wq, ws, 64)),
                     (blockwise_fp8_gemm, (q, s, wq, ws, 64))):
        with pytest.raises(NotImplementedError, match="block_size"):
            fn(*args)
    with pytest.raises(NotImplementedError, match="e5m2"):
        fp8_blockwise_act_quant(x, 128, torch.float8_e5m2)
    with pytest.raises(NotImplementedError, match="e5m2"):
        fp8_blockwise_weight_quant(x, 128, torch.float8_e5m2)
    with pytest.raises(NotImplementedError, match="block_size"):
        BlockwiseQuantLinear(256, 8, block_size=64)
    with pytest.raises(NotImplementedError, match="e5m2"):
        BlockwiseQuantLinear(256, 8, dtype=torch.float8_e5m2)
    with pytest.raises(ValueError, match="multiple of 128"):
        fp8_blockwise_act_quant(x[:, :192])
    with pytest.raises(ValueError, match="multiple of 128"):
        fp8_blockwise_weight_quant(x[:, :64].contiguous())
    with pytest.raises(ValueError, match="multiple of 128"):
        BlockwiseQuantLinear(192, 8)
    with pytest.raises(ValueError, match="scale must be"):
        fp8_blockwise_weight_dequant(wq, ws[:, :1])


def test_op_set_and_fragment():
    for name in OPS:
        assert hasattr(torch.ops.torchao, name)
    assert ops.native_dispatch_blockfp8() == OPS, ops._native_error
    assert {d.split("::")[-1] for d in ops.lib_blockfp8._op_defs} == OPS
    for other in (ops.lib, ops.lib_float8, ops.lib_float8_dyn, ops.lib_mx, ops.lib_mxfp4):
        assert not any("blockfp8" in d for d in other._op_defs)
    for served in (ops.native_dispatch(), ops.native_dispatch_float8(),
                   ops.native_dispatch_float8_dyn(), ops.native_dispatch_mx(),
                   ops.native_dispatch_mxfp4()):
        assert not (served & OPS)
    assert not any("mx_" in n or "mxfp4" in n for n in OPS)


def test_cpu_ops_raise():
    x = torch.zeros(1, 128, dtype=torch.bfloat16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.blockfp8_quantize_act(x)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.blockfp8_dyn_linear(x, torch.zeros(8, 128).to(E4), torch.zeros(1, 1), None)


def test_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode

    T = torch.ops.torchao
    with FakeTensorMode():
        x = torch.empty(2, 3, 384, dtype=torch.bfloat16)
        w = torch.empty(272, 384, dtype=torch.bfloat16)
        q, s = T.blockfp8_quantize_act(x)
        assert q.shape == (2, 3, 384) and q.dtype is E4
        assert s.shape == (2, 3, 3) and s.dtype is torch.float32
        wq, ws = T.blockfp8_quantize_weight(w)
        assert wq.shape == (272, 384) and wq.dtype is E4
        assert ws.shape == (3, 3) and ws.dtype is torch.float32
        d = T.blockfp8_dequantize_weight(wq, ws)
        assert d.shape == (272, 384) and d.dtype is torch.float32
        assert T.blockfp8_dequantize_weight(wq, ws, True).dtype is torch.bfloat16
        y = T.blockfp8_scaled_mm(q, s, wq, ws, None)
        assert y.shape == (2, 3, 272) and y.dtype is torch.bfloat16
        y = T.blockfp8_dyn_linear(x, wq, ws, torch.empty(272, dtype=torch.bfloat16))
        assert y.shape == (2, 3, 272) and y.dtype is torch.bfloat16
        with pytest.raises(RuntimeError, match="multiple of 128"):
            T.blockfp8_quantize_act(torch.empty(2, 192, dtype=torch.bfloat16))
        with pytest.raises(RuntimeError, match="128x128 block"):
            T.blockfp8_scaled_mm(q, s, wq, ws[:2], None)


def _call(name, *args):
    fn = getattr(_lib.lib(), name)
    return fn(*args), _lib.lib().tao_last_error().decode()


def test_c_abi_symbols_and_validation():
    """The symbols are exported and bound; bad arguments return 1 with tao_last_error set before any
    device work (the pointers are host buffers here and never dereferenced)."""
    raw = ctypes.CDLL(_lib.library_path())
    for name in ABI:
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc, msg = _call("tao_blockfp8_quantize_act_bf16", p, p, p, 1, 192, None)
    assert rc == 1 and "multiple of 128" in msg
    rc, msg = _call("tao_blockfp8_quantize_weight_bf16", p, p, p, 8, 64, None)
    assert rc == 1 and "multiple of 128" in msg
    rc, msg = _call("tao_blockfp8_dequant_weight", p, p, p, 8, 128, 2, None)
    assert rc == 1 and "out_bf16" in msg
    rc, msg = _call("tao_blockfp8_scaled_mm_bf16", p, p, p, p, None, p, 1, 8, 320, None)
    assert rc == 1 and "multiple of 128" in msg
    rc, msg = _call("tao_blockfp8_scaled_mm_bf16", p, p, p, p, None, p, -1, 8, 128, None)
    assert rc == 1 and "negative" in msg
    rc, msg = _call("tao_blockfp8_dyn_linear_bf16", p, p, p, None, p, 2, 8, 128, None)
    assert rc == 1 and "one token" in msg
    rc, msg = _call("tao_blockfp8_dyn_linear_bf16", p, p, p, None, p, 1, 8, 65536 + 128, None)
    assert rc == 1 and "65536" in msg
    odd = ctypes.c_void_p(p.value + 1)
    rc, msg = _call("tao_blockfp8_scaled_mm_bf16", odd, p, p, p, None, p, 1, 8, 128, None)
    assert rc == 1 and "xq" in msg
    rc, msg = _call("tao_blockfp8_scaled_mm_bf16", p, odd, p, p, None, p, 1, 8, 128, None)
    assert rc == 1 and "xs" in msg
    for name, args in (("tao_blockfp8_quantize_act_bf16", (p, p, p, 0, 128, None)),
                       ("tao_blockfp8_quantize_weight_bf16", (p, p, p, 0, 128, None)),
                       ("tao_blockfp8_scaled_mm_bf16", (p, p, p, p, None, p, 0, 8, 128, None)),
                       ("tao_blockfp8_dyn_linear_bf16", (p, p, p, None, p, 0, 8, 128, None))):
        assert _call(name, *args)[0] == 0
    rc, msg = _call("tao_tune_blockfp8_mfma", 2)
    assert rc == 1 and "blockfp8 mfma" in msg
    assert _call("tao_tune_blockfp8_mfma", 1)[0] == 0 and _call("tao_tune_reset")[0] == 0
