"""CPU tests of the 2:4 sparse int4 weight-only workflow (Int4WeightOnlyConfig with
MarlinSparseLayout): the quantize_ swap, the stored format, the plain-torch linear, the refusals
and the C entries' argument checks."""

import pytest
import torch
import torch.nn.functional as F

from torchao import _lib
from torchao.dtypes import MarlinSparseAQTTensorImpl, MarlinSparseLayout
from torchao.quantization import Int4WeightOnlyConfig, quantize_

T = torch.ops.torchao


def _config(group_size=128, **kw):
    return Int4WeightOnlyConfig(group_size=group_size, layout=MarlinSparseLayout(), **kw)


@pytest.mark.parametrize("group_size", [128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantize_swaps_the_weight_and_the_cpu_linear_is_its_definition(group_size, dtype):
    torch.manual_seed(3)
    m = torch.nn.Linear(256, 24).to(dtype)
    quantize_(m, _config(group_size))
    impl = m.weight.tensor_impl
    assert isinstance(impl, MarlinSparseAQTTensorImpl) and m.weight.shape == (24, 256)
    assert impl.int_data.shape == (24, 16) and impl.meta.shape == (24, 8)
    assert impl.scale.shape == (256 // group_size, 24)
    assert (impl.group_size, impl.num_bits, impl.original_shape) == (group_size, 4, (24, 256))
    codes, scale, zero_point = impl.get_plain()
    assert codes.dtype == torch.int32 and int(codes.min()) >= 0 and int(codes.max()) <= 15
    assert int((codes != 8).reshape(-1, 4).sum(1).max()) == 2 and bool((zero_point == 8).all())
    # the compressed tensors are the op's on those codes, and the round trip is exact
    values, meta, err = T.int4_sp24_compress(codes)
    assert int(err) == 0 and torch.equal(values, impl.int_data) and torch.equal(meta, impl.meta)
    w = ((codes - 8).float() * scale.float().repeat_interleave(group_size, 1)).to(dtype)
    assert torch.equal(m.weight.dequantize(), w)
    x = torch.randn(2, 3, 256).to(dtype)
    assert torch.equal(m(x), F.linear(x, w, m.bias))
    assert torch.equal(
        T.int4_sp24_weight_only_linear(x, values, meta, impl.scale, group_size, m.bias), m(x))


def test_group_size_other_than_128_or_in_features_is_the_references_assertion():
    with pytest.raises(AssertionError, match="only supports 128 group size or per channel"):
        quantize_(torch.nn.Linear(256, 8).to(torch.bfloat16), _config(64))


@pytest.mark.parametrize("make, kw, match", [
    (lambda: torch.nn.Linear(128, 16), {"use_hqq": True}, "use_hqq"),
    (lambda: torch.nn.Linear(192, 16), {"group_size": 64}, "multiple of 128"),
    (lambda: torch.nn.Conv1d(8, 16, 128), {}, "2-D"),
])
def test_refusals_come_before_any_module_is_changed(make, kw, match):
    m = torch.nn.Sequential(torch.nn.Linear(128, 128), make()).to(torch.bfloat16)
    served = m[0].weight
    with pytest.raises(NotImplementedError, match=match):
        quantize_(m, _config(**kw), filter_fn=lambda mod, fqn: hasattr(mod, "weight"))
    assert m[0].weight is served and type(m[0].weight) is torch.nn.Parameter


def test_three_kept_codes_in_a_group_raise():
    codes = torch.full((2, 128), 8, dtype=torch.int32)
    codes[1, 124:] = torch.tensor([1, 8, 2, 3], dtype=torch.int32)
    assert int(T.int4_sp24_compress(codes)[2]) == 1
    with pytest.raises(ValueError, match="2:4"):
        MarlinSparseAQTTensorImpl.from_plain(
            codes, torch.ones(2, 1), torch.full((2, 1), 8.0), MarlinSparseLayout())


def test_c_entries_reject_bad_arguments_before_device_work():
    lib, p = _lib.lib(), 4096

    def call(name, *args):
        return getattr(lib, name)(*args), lib.tao_last_error().decode()

    for rc, msg, want in [
        call("tao_int4_sp24_compress", p, p, p, p, 8, 192, None) + ("multiple of 128",),
        call("tao_int4_sp24_compress", p, p, p, None, 8, 128, None) + ("err are required",),
        call("tao_int4_sp24_decompress", p, p, 8, 8, 128, None) + ("codes must be 16-byte",),
        call("tao_int4_sp24_linear_bf16", p, p, p, p, None, p, 1, 8, 64, 64, None)
        + ("K (64)",),
        call("tao_int4_sp24_linear_bf16", p, p, p, p, None, p, 1, 8, 256, 64, None)
        + ("group_size (64)",),
        call("tao_int4_sp24_linear_bf16", p, p, p, p, None, p, -1, 8, 128, 128, None) + ("M (",),
        call("tao_int4_sp24_linear_bf16", p, p, p, None, None, p, 1, 8, 128, 128, None)
        + ("scale and y are required",),
        call("tao_int4_sp24_linear_bf16", p, p, 4, p, None, p, 1, 8, 128, 128, None)
        + ("meta must be 8-byte",),
        call("tao_tune_int4_sp24", 3, 0, 0, 0, 0, 0, 0, 0) + ("int4_sp24 route",),
        call("tao_tune_int4_sp24", 0, 0, 0, 0, 0, 48, 0, 0) + ("bm must be",),
    ]:
        assert rc == 1 and want in msg, (rc, msg, want)
    # empty problems succeed without touching a pointer; the route rule is a host function
    assert call("tao_int4_sp24_linear_bf16", p, p, p, p, None, p, 0, 8, 128, 128, None)[0] == 0
    bound = next(M for M in range(1, 64) if lib.tao_int4_sp24_route(M + 1, 16, 128) == 2)
    assert lib.tao_int4_sp24_route(bound, 16, 128) == 1
    # tokens that do not fit the GEMV's LDS go to the GEMM
    assert lib.tao_int4_sp24_route(1, 16, 32768) == 2
