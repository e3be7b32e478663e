"""CPU tests of the 2:4 sparse int8 workflow (Int8DynamicActivationInt8WeightConfig with
SemiSparseLayout): the pruning rule, the plain-torch definitions of compress / decompress, the
quantize_ swap and its refusals, the state_dict round trip and the C entries' argument checks."""

import copy
import ctypes

import pytest
import torch

from torchao import _lib
from torchao.dtypes import SemiSparseAQTTensorImpl, SemiSparseLayout, TensorCoreTiledLayout
from torchao.quantization import Int8DynamicActivationInt8WeightConfig, quantize_

T = torch.ops.torchao
EDGE = [[0, 0, 0, 0], [5, 0, 0, 0], [0, -6, 0, 0], [0, 0, 7, 0], [0, 0, 0, -127],
        [1, 2, 0, 0], [1, 0, 2, 0], [1, 0, 0, 2], [0, 1, 2, 0], [0, 1, 0, 2], [0, 0, 1, 2]]


def _config(layout=None):
    return Int8DynamicActivationInt8WeightConfig(layout=layout or SemiSparseLayout())


def test_pre_process_zeroes_the_two_smallest_magnitudes_of_each_four():
    g = torch.Generator().manual_seed(0)
    mags = torch.stack([torch.randperm(4, generator=g) + 1 for _ in range(64)]).float()
    w = (mags * (torch.randint(0, 2, mags.shape, generator=g) * 2 - 1)).reshape(2, 128)
    out = SemiSparseLayout().pre_process(w.to(torch.bfloat16)).float()
    assert torch.equal(out, torch.where(w.abs() >= 3, w, torch.zeros_like(w)))


def test_compress_then_decompress_is_the_identity_on_2_4_data():
    g = torch.Generator().manual_seed(1)
    w = torch.randint(-127, 128, (5, 256), generator=g, dtype=torch.int8)
    w = SemiSparseLayout().pre_process(w.float()).to(torch.int8)
    w[4, :44] = torch.tensor(EDGE, dtype=torch.int8).reshape(-1)
    values, meta, err = T.int8_sp24_compress(w)
    assert values.shape == (5, 128) and meta.shape == (5, 8) and meta.dtype == torch.int32
    assert int(err) == 0
    # the eleven edge groups: kept positions, low field first (p0 | p1 << 2), and kept values
    codes = [(int(meta[4, g // 8]) >> (4 * (g % 8))) & 0xF for g in range(11)]
    assert codes == [0x4, 0x4, 0x4, 0x8, 0xC, 0x4, 0x8, 0xC, 0x9, 0xD, 0xE]
    assert values[4, :8].tolist() == [0, 0, 5, 0, 0, -6, 0, 7]
    assert torch.equal(T.int8_sp24_decompress(values, meta), w)


def test_three_nonzeros_in_a_group_raise():
    w = torch.zeros(2, 128, dtype=torch.int8)
    w[1, 124:] = torch.tensor([1, 0, 2, 3], dtype=torch.int8)
    assert int(T.int8_sp24_compress(w)[2]) == 1
    with pytest.raises(ValueError, match="2:4"):
        SemiSparseAQTTensorImpl.from_plain(w, torch.ones(2), None, SemiSparseLayout())


def test_quantize_swaps_the_weight_and_state_dict_round_trips():
    torch.manual_seed(2)
    m = torch.nn.Sequential(torch.nn.Linear(128, 24), torch.nn.Linear(24, 8)).to(torch.bfloat16)
    b0 = m[0].bias.data.clone()
    only_first = lambda mod, fqn: isinstance(mod, torch.nn.Linear) and mod.in_features == 128
    quantize_(m, _config(), filter_fn=only_first)
    impl = m[0].weight.original_weight_tensor.tensor_impl
    assert isinstance(impl, SemiSparseAQTTensorImpl)
    assert impl.values.shape == (24, 64) and impl.meta.shape == (24, 4) and impl.shape == (24, 128)
    # the stored weight is 2:4, and the module computes the op's definition
    assert int((impl.get_plain()[0] != 0).reshape(-1, 4).sum(1).max()) == 2
    x = torch.randn(3, 128).to(torch.bfloat16)
    y = m(x)
    assert torch.equal(y, m[1](T.int8_sp24_dyn_linear(x, impl.values, impl.meta, impl.scale, b0)))
    fresh = torch.nn.Sequential(torch.nn.Linear(128, 24), torch.nn.Linear(24, 8)).to(torch.bfloat16)
    quantize_(fresh, _config(), filter_fn=only_first)
    fresh.load_state_dict(copy.deepcopy(m.state_dict()))
    assert torch.equal(fresh(x), y)


@pytest.mark.parametrize("make, layout, match", [
    (lambda: torch.nn.Linear(192, 16), None, "multiple of 128"),
    (lambda: torch.nn.Conv1d(8, 16, 128), None, "2-D"),
    (lambda: torch.nn.Linear(128, 16), TensorCoreTiledLayout(), "only PlainLayout"),
])
def test_refusals_come_before_any_module_is_changed(make, layout, match):
    m = torch.nn.Sequential(torch.nn.Linear(128, 128), make()).to(torch.bfloat16)
    served = m[0].weight
    with pytest.raises(NotImplementedError, match=match):
        quantize_(m, _config(layout), filter_fn=lambda mod, fqn: hasattr(mod, "weight"))
    assert m[0].weight is served and type(m[0].weight) is torch.nn.Parameter


def test_small_in_features_are_left_alone_as_by_the_plain_layout():
    m = torch.nn.Sequential(torch.nn.Linear(128, 16), torch.nn.Linear(16, 8)).to(torch.bfloat16)
    quantize_(m, _config())
    assert type(m[1].weight) is torch.nn.Parameter and type(m[0].weight) is not torch.nn.Parameter


def test_c_entries_are_exported_and_reject_bad_arguments_before_device_work():
    names = ["tao_int8_sp24_compress", "tao_int8_sp24_decompress", "tao_int8_sp24_scaled_mm_bf16",
             "tao_int8_sp24_dyn_linear_bf16", "tao_int8_sp24_route", "tao_tune_sp24",
             "tao_tune_sp24_gemm"]
    raw = ctypes.CDLL(_lib.library_path())
    assert all(hasattr(raw, n) and n in _lib.exported_symbols() for n in names)
    lib, p = _lib.lib(), 4096

    def call(name, *args):
        return getattr(lib, name)(*args), lib.tao_last_error().decode()

    for rc, msg, want in [
        call("tao_int8_sp24_compress", p, p, p, p, 8, 192, None) + ("multiple of 128",),
        call("tao_int8_sp24_compress", p, p, p, None, 8, 128, None) + ("are required",),
        call("tao_int8_sp24_decompress", 8, p, p, 8, 128, None) + ("16-byte aligned",),
        call("tao_int8_sp24_scaled_mm_bf16", p, p, p, p, p, None, p, 1, 8, 64, None)
        + ("multiple of 128",),
        call("tao_int8_sp24_scaled_mm_bf16", p, p, p, p, p, None, p, -1, 8, 128, None) + ("M (",),
        call("tao_int8_sp24_scaled_mm_bf16", p, p, p, p, p, None, 4, 1, 8, 128, None)
        + ("8-byte aligned",),
        call("tao_int8_sp24_dyn_linear_bf16", p, p, p, p, None, p, 2, 8, 128, None)
        + ("one token",),
        call("tao_int8_sp24_dyn_linear_bf16", p, p, p, p, None, p, 1, 8, 32768 + 128, None)
        + ("32768",),
        call("tao_tune_sp24", 3, 0, 0, 0, 0) + ("sp24 route",),
        call("tao_tune_sp24_gemm", 48, 0, 0) + ("bm must be",),
    ]:
        assert rc == 1 and want in msg, (rc, msg, want)
    # empty problems succeed without touching a pointer; the route rule is a host function
    assert call("tao_int8_sp24_scaled_mm_bf16", p, p, p, p, p, None, p, 0, 8, 128, None)[0] == 0
    assert lib.tao_int8_sp24_route(2, 16, 128) == 1 and lib.tao_int8_sp24_route(3, 16, 128) == 2
    # two tokens of K = 32768 do not fit the GEMV's LDS (tests/test_gpu_sp24.py runs both sides)
    assert lib.tao_int8_sp24_route(2, 16, 32256) == 1 and lib.tao_int8_sp24_route(2, 16, 32768) == 2
