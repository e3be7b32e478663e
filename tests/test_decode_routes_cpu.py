"""The routing table of the fused decode path (kernels.DECODE_FORMATS), the parts that need no
GPU: each format's K limits and where its RMSNorm runs, against the rules the kernels were
measured and built for (csrc: the entries' K checks; kernels.prologue_pays)."""

import pytest

from torchao._models.llama import kernels
from torchao._models.llama import model as M

WQKV, W13, HEAD = (6144, 4096), (28672, 4096), (128256, 4096)
W13_70B = (57344, 8192)


def test_rows_and_order():
    assert list(kernels.DECODE_FORMATS) == ["int4", "int8wo", "int8dq", "fp8wo", "fp8dq"]
    assert list(M._DECODE_PARTS) == list(kernels.DECODE_FORMATS)
    for name, f in kernels.DECODE_FORMATS.items():
        assert f.name == name
        assert f.entry == f"tao_{'int4wo' if name == 'int4' else name}_decode_bf16"
        assert callable(getattr(kernels, f"{name}_decode"))
        assert f.bf16_x_only == name.startswith("fp8")


@pytest.mark.parametrize("name,norm_max_k,max_k", [
    ("int4", 16384, None), ("int8wo", 16384, None), ("int8dq", 8192, 32768),
    ("fp8wo", 16384, None), ("fp8dq", 16384, 32768)])
def test_limits(name, norm_max_k, max_k):
    f = kernels.DECODE_FORMATS[name]
    assert (f.norm_max_k, f.max_k) == (norm_max_k, max_k)
    assert kernels.FP8_NORM_MAX_K == 16384 and kernels.FP8DQ_MAX_K == 32768


@pytest.mark.parametrize("name", ["int8wo", "fp8wo"])
def test_weight_only_byte_formats_take_the_norm_inside_at_every_shape(name):
    f = kernels.DECODE_FORMATS[name]
    for N, K in (WQKV, W13, HEAD, W13_70B, (37, 16384)):
        assert f.norm_placement(N, K) == "inside"
    # past the prologue's limit: rmsnorm as its own launch, then the fused kernel without it
    assert f.norm_placement(37, 16400) == f.norm_placement(37, 16416) == "outside"
    assert f.norm_placement(37, 1 << 20) == "outside"


@pytest.mark.parametrize("name", ["int4", "fp8dq"])
def test_prologue_pays_formats(name):
    f = kernels.DECODE_FORMATS[name]
    for N, K in (WQKV, W13, HEAD, W13_70B, (10240, 8192), (37, 16384), (16384, 4128)):
        want = "inside" if kernels.prologue_pays(N, K) else "outside"
        assert f.norm_placement(N, K) == want
    assert f.norm_placement(*WQKV) == f.norm_placement(*W13) == "inside"
    assert f.norm_placement(*HEAD) == f.norm_placement(*W13_70B) == "outside"
    assert f.norm_placement(37, 16416) == "outside"  # prologue_pays says inside; the limit rules
    assert f.norm_placement(37, 32768) == "outside"
    assert f.norm_placement(37, 32784) == ("outside" if name == "int4" else None)


def test_int8dq_is_fused_with_its_norm_up_to_8192_and_unfused_past_it():
    f = kernels.DECODE_FORMATS["int8dq"]
    for N, K in (WQKV, W13, HEAD, W13_70B, (37, 8192)):
        assert f.norm_placement(N, K) == "inside"
    assert f.norm_placement(37, 8208) is None
    assert f.norm_placement(128256, 16384) is None
    assert f.norm_placement(37, 32784) is None
