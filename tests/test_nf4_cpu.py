"""CPU tests of the NF4 (QLoRA) weight format against the reference fixtures (tests/golden/nf4_*,
written by experiments/gen_golden_nf4.py): the plain-torch quantizer and dequantizer byte for byte,
the linear and its grad_input, the tensor plumbing, the reference's checkpoint, the FSDP refusals,
and the float32 formula against the project's bar."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao.dtypes import NF4Tensor, to_nf4
from torchao.dtypes._nf4tensor_api import NF4WeightOnlyConfig, nf4_weight_only
from torchao.dtypes.nf4tensor import (
    NF4_LEVELS,
    LinearNF4,
    SubclassTensorArgs,
    get_block_absmax,
    linear_nf4,
    nf4_constructor,
)
from torchao.quantization import quantize_

FIXTURES = golden_files("nf4_N")
CKPT = "nf4_refckpt_N32_K512"
INNER = ("quantized_data", "quantized_scalers", "quantization_factor", "scaler_mean", "nf4")
BAR = 4e-3


def bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def rel_l2(y, ref):
    return float(torch.linalg.norm(y.double() - ref) / torch.linalg.norm(ref))


def assert_stored(t: NF4Tensor, rec, prefix=""):
    """Every stored tensor of t equals the fixture's, byte for byte."""
    for name in INNER:
        got, want = getattr(t, name).cpu(), rec[prefix + name]
        if got.dtype is torch.bfloat16:
            got = bits(got)
        else:
            got = got.numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert np.array_equal(got, want), f"{prefix}{name} differs"


def from_fixture(rec, shape, prefix="") -> NF4Tensor:
    numel = int(np.prod(shape))
    meta = SubclassTensorArgs(torch.Size(shape), torch.empty(shape, device="meta").stride(), 0,
                              torch.bfloat16, torch.device("cpu"), False)
    return nf4_constructor(
        meta, 64, numel // 64, 256,
        torch.from_numpy(rec[prefix + "quantized_scalers"]),
        bf16(rec[prefix + "quantization_factor"]),
        bf16(rec[prefix + "scaler_mean"]).reshape(()),
        torch.from_numpy(rec[prefix + "quantized_data"]),
        bf16(rec[prefix + "nf4"]))


def mean_is_pinned(w: torch.Tensor) -> bool:
    """The generator's condition: the fp32 and float64 means of the block absmaxes round to the
    same bf16 and lie >= 2^-20 (relative) from a bf16 rounding boundary, so the unpinned
    summation order of the mean cannot change a byte."""
    a = get_block_absmax(w.flatten(), 64)
    m64 = a.double().mean().item()
    r = torch.tensor(m64, dtype=torch.float64).to(torch.bfloat16)
    if torch.tensor(a.float().mean().item()).to(torch.bfloat16) != r:
        return False
    rb = r.view(torch.int16).item()
    for nb in (rb - 1, rb + 1):
        other = torch.tensor(nb, dtype=torch.int16).view(torch.bfloat16).double().item()
        if abs(m64 - (r.double().item() + other) / 2) < abs(m64) * 2.0 ** -20:
            return False
    return True


def test_config_alias_and_fields():
    assert nf4_weight_only is NF4WeightOnlyConfig
    c = NF4WeightOnlyConfig()
    assert (c.block_size, c.scaler_block_size) == (64, 256)
    c = NF4WeightOnlyConfig(block_size=32, scaler_block_size=128)
    assert (c.block_size, c.scaler_block_size) == (32, 128)
    import torchao.dtypes as dt

    assert dt.NF4Tensor is NF4Tensor and dt.to_nf4 is to_nf4


@pytest.mark.parametrize("fname", FIXTURES)
def test_to_nf4_equals_the_fixture(fname):
    rec = load_golden(fname)
    w = bf16(rec["w"])
    assert mean_is_pinned(w)
    t = to_nf4(w)
    assert isinstance(t, NF4Tensor) and t.shape == w.shape and t.dtype is torch.bfloat16
    assert (t.block_size, t.scaler_block_size, t.n_blocks) == (64, 256, w.numel() // 64)
    assert_stored(t, rec)
    assert np.array_equal(bits(t.nf4), bits(torch.tensor(NF4_LEVELS).to(torch.bfloat16)))


def test_to_nf4_edges():
    """An all-zero block (code 0 everywhere: NaN wins), a negative absmax element, a block of
    equal values, bf16 neighbours of every midpoint of adjacent levels; and the same tensor with
    an inf, whose scalers all stop being finite."""
    rec = load_golden("nf4_quant_edges.npz")
    fin = bf16(rec["fin_w"])
    assert mean_is_pinned(fin)
    t = to_nf4(fin)
    assert_stored(t, rec, "fin_")
    assert bool((t.quantized_data[:32] == 0).all())  # block 0: all zero -> code 0
    assert_stored(to_nf4(bf16(rec["inf_w"])), rec, "inf_")


@pytest.mark.parametrize("fname", FIXTURES)
def test_dequantize_equals_w_hat(fname):
    rec = load_golden(fname)
    t = from_fixture(rec, rec["w"].shape)
    for out in (t.get_original_weight(), t.to(torch.bfloat16)):
        assert out.dtype is torch.bfloat16 and np.array_equal(bits(out), rec["w_hat"])
    assert torch.equal(t.to(torch.float32), bf16(rec["w_hat"]).float())


def test_dequantize_1d():
    rec = load_golden(FIXTURES[0])
    numel = rec["w"].size
    t = from_fixture(rec, (numel,))
    assert np.array_equal(bits(t.get_original_weight()), rec["w_hat"].reshape(-1))
    t2 = to_nf4(bf16(rec["w"]).flatten())
    assert t2.shape == (numel,)
    assert_stored(t2, rec)


@pytest.mark.parametrize("fname", FIXTURES)
def test_linear_forward_and_grad_input(fname):
    rec = load_golden(fname)
    t = from_fixture(rec, rec["w"].shape)
    w_hat = bf16(rec["w_hat"])
    x = bf16(rec["x"]).clone().requires_grad_(True)
    bias = bf16(rec["bias"])
    y = F.linear(x, t, bias)
    assert np.array_equal(bits(y), rec["y_ref"])
    assert torch.equal(linear_nf4(x, t), F.linear(x, w_hat))
    g = torch.ones_like(y) * 0.5
    y.backward(g)
    assert torch.equal(x.grad, g @ w_hat)
    assert LinearNF4.apply(x.detach(), t).requires_grad is False


def test_t_copy_to_and_state_dict(tmp_path):
    rec = load_golden("nf4_N64_K256.npz")
    w = bf16(rec["w"])
    t = to_nf4(w)
    w_hat = bf16(rec["w_hat"])
    # t(): strides swapped, data shared
    tt = t.t()
    assert tt.shape == (256, 64) and tt.stride() == (1, 256) and not tt.is_contiguous()
    assert tt.quantized_data.data_ptr() == t.quantized_data.data_ptr()
    assert torch.equal(tt.to(torch.bfloat16), w_hat.t())
    x = bf16(rec["x"])
    assert torch.equal(torch.mm(x, tt), F.linear(x, w_hat))
    # detach / clone
    d, c = t.detach(), t.clone()
    assert d.quantized_data.data_ptr() == t.quantized_data.data_ptr()
    assert c.quantized_data.data_ptr() != t.quantized_data.data_ptr()
    assert_stored(c, rec)
    # copy_: same metadata, and from a plain tensor by re-quantizing
    other = to_nf4(torch.zeros_like(w) + 0.25)
    other.copy_(t)
    assert_stored(other, rec)
    other = to_nf4(torch.zeros_like(w) + 0.25)
    other.copy_(w)
    assert_stored(other, rec)
    coarse = to_nf4(w, 32, 128)
    assert coarse.n_blocks == w.numel() // 32
    other = to_nf4(torch.zeros_like(w) + 0.25)
    other.copy_(coarse)  # another blocking: through its dequantized weight
    assert torch.equal(other.quantized_data,
                       to_nf4(coarse.get_original_weight()).quantized_data)
    # .to(dtype) dequantizes; .to(device) keeps NF4
    assert t.to(torch.float16).dtype is torch.float16
    assert isinstance(t.to("cpu"), NF4Tensor) and isinstance(t.cpu(), NF4Tensor)
    # state_dict round trip through torch.save / torch.load(weights_only=True)
    m = torch.nn.Linear(256, 64, dtype=torch.bfloat16)
    with torch.no_grad():
        m.weight.copy_(w)
    quantize_(m, nf4_weight_only())
    assert isinstance(m.weight, torch.nn.Parameter) and isinstance(m.weight, NF4Tensor)
    assert not m.weight.requires_grad
    assert_stored(m.weight, rec)
    path = tmp_path / "sd.pt"
    torch.save(m.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    m2 = torch.nn.Linear(256, 64, dtype=torch.bfloat16)
    quantize_(m2, nf4_weight_only())
    m2.load_state_dict(sd)
    assert_stored(m2.weight, rec)
    assert torch.equal(m2(x), m(x))


def test_other_dtypes_and_block_sizes_run_the_formulas():
    rec = load_golden("nf4_N64_K256.npz")
    w = bf16(rec["w"]).float()
    t = to_nf4(w)
    assert t.dtype is torch.float32 and t.quantization_factor.dtype is torch.float32
    err = rel_l2(t.get_original_weight(), w.double())
    assert err < 0.15, err
    t16 = to_nf4(w.half(), 32, 64)
    assert t16.n_blocks == w.numel() // 32 and t16.quantization_factor.numel() == t16.n_blocks // 64
    assert rel_l2(t16.get_original_weight(), w.double()) < 0.15
    with pytest.raises(AssertionError, match="not a multiple of block_size = 64"):
        to_nf4(torch.zeros(100, dtype=torch.bfloat16))
    with pytest.raises(AssertionError, match="not whole groups of 256"):
        to_nf4(torch.zeros(64, 64, dtype=torch.bfloat16))  # 64 blocks: not a multiple of 256
    with pytest.raises(AssertionError, match="1-D and 2-D"):
        to_nf4(torch.zeros(2, 64, 256, dtype=torch.bfloat16))
    # copy_ between different shapes is refused, whatever the block sizes
    small, big = to_nf4(w.bfloat16()), to_nf4(torch.cat([w, w]).bfloat16())
    for src in (big, to_nf4(torch.cat([w, w]).bfloat16(), 32, 64), torch.cat([w, w])):
        with pytest.raises(RuntimeError, match="copy_: source shape"):
            small.copy_(src)


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    w = sd["weight"]
    assert isinstance(w, NF4Tensor) and w.shape == (32, 512) and w.dtype is torch.bfloat16
    assert (w.block_size, w.scaler_block_size, w.n_blocks) == (64, 256, 256)
    assert_stored(w, rec)
    assert np.array_equal(bits(w.get_original_weight()), rec["w_hat"])
    m = torch.nn.Linear(512, 32, dtype=torch.bfloat16)
    quantize_(m, nf4_weight_only())
    m.load_state_dict(sd)
    assert_stored(m.weight, rec)
    assert np.array_equal(bits(m.bias), rec["bias"])
    # and this build's quantizer forms the same bytes from the original weight
    assert_stored(to_nf4(bf16(rec["w"])), rec)


@pytest.mark.parametrize("call", [
    lambda t: t.split(32), lambda t: t.new_zeros(t.shape), lambda t: t[:32],
    lambda t: t.view(-1), lambda t: t.as_strided(t.shape, t.stride()),
    lambda t: torch.cat([t, t]), lambda t: t.pin_memory(),
    lambda t: t.fsdp_pre_all_gather(None),
    lambda t: t.fsdp_post_all_gather((), None, torch.bfloat16),
], ids=["split", "new_zeros", "slice", "view", "as_strided", "cat", "pin_memory",
        "fsdp_pre_all_gather", "fsdp_post_all_gather"])
def test_fsdp_ops_raise(call):
    t = to_nf4(torch.ones(64, 256, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="FSDP2.*served: detach, clone"):
        call(t)


def test_collectives_raise():
    from torchao.dtypes.nf4tensor import _ATEN_HANDLERS

    t = to_nf4(torch.ones(64, 256, dtype=torch.bfloat16))
    ops = [op for op in _ATEN_HANDLERS if "c10d" in str(op)]
    if torch.distributed.is_available():
        assert any("all_gather_into_tensor" in str(op) for op in ops)
        assert any("wait_tensor" in str(op) for op in ops)
    for op in ops:
        with pytest.raises(NotImplementedError, match="FSDP2"):
            _ATEN_HANDLERS[op](op, (t,), {})
    with pytest.raises(NotImplementedError, match="does not serve aten.add.Tensor"):
        torch.ops.aten.add.Tensor(t, t)


@pytest.mark.parametrize("fname", FIXTURES)
def test_float32_formula_meets_the_bar_on_the_fixtures(fname):
    """y = sum_k x w^ + bias evaluated in float32 on the bf16 w^ is within the project's bar of
    4e-3 rel-L2 of its float64 evaluation, and so is its bf16 rounding (one rounding of the sum,
    one of the bias add): the format leaves the bar room, tests/test_gpu_nf4.py may hold the
    kernels to it."""
    rec = load_golden(fname)
    x, w_hat, bias = bf16(rec["x"]).float(), bf16(rec["w_hat"]).float(), bf16(rec["bias"]).float()
    y64 = torch.from_numpy(rec["y64"])
    assert torch.equal(y64, bf16(rec["x"]).double() @ bf16(rec["w_hat"]).double().t()
                       + bf16(rec["bias"]).double())
    y32 = x @ w_hat.t()
    y16 = ((y32.to(torch.bfloat16).float() + bias).to(torch.bfloat16))
    e32, e16 = rel_l2(y32 + bias, y64), rel_l2(y16, y64)
    e_ref = rel_l2(bf16(rec["y_ref"]), y64)
    print(f"{fname}: float32 formula vs float64 {e32:.3e}, rounded to bf16 {e16:.3e}, "
          f"reference CPU linear {e_ref:.3e}")
    assert e32 <= BAR and e16 <= BAR and e_ref <= BAR


@pytest.mark.parametrize("M,N,K", [(1, 16, 1024), (3, 256, 1088), (2, 256, 4160)])
def test_exact_inputs_on_the_torch_formulation(M, N, K):
    """The exact-input maker's conditions hold, and the plain-torch path (the GPU tests' oracle
    elsewhere) equals the float64 formula bit for bit on them, bias or not."""
    import exact_inputs_nf4 as E

    codes, qs, qf, mean, levels, bias, x = E.make_nf4_exact(M, N, K, seed=M + N + K)
    meta = SubclassTensorArgs(torch.Size((N, K)), (K, 1), 0, torch.bfloat16, torch.device("cpu"),
                              False)
    t = NF4Tensor(meta, 64, N * K // 64, 256, qs, qf, mean, codes, levels)
    w = E.dequant64(codes, qs, qf, mean, levels, (N, K))
    assert torch.equal(t.get_original_weight().double(), w)
    for b in (None, bias):
        assert torch.equal(F.linear(x, t, b), E.ref_nf4(x, codes, qs, qf, mean, levels, N, b))
