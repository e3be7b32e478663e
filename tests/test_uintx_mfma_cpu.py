"""The uintx linear's MFMA route in the route rule (csrc/uintx_host.h) through the C ABI: the hook
tao_tune_uintx_mfma / tuning(uintx_mfma=1) turns every "dequantize + matmul" answer on a shape the
kernel serves into "MFMA GEMM" (3) and nothing else."""

import pytest

from torchao import _lib
from torchao.kernel.tuning import tuning

MS = range(1, 33)
OFF = [1] * 8 + [2] * 24
ON = [1] * 8 + [3] * 24


def routes(bits=3, n=4096, k=4096, g=64):
    route = _lib.lib().tao_uintx_linear_route_g
    return [route(m, n, k, bits, g) for m in MS]


def test_hook_turns_dequant_mm_into_mfma():
    _lib.call("tao_tune_reset")
    assert routes() == OFF
    try:
        _lib.call("tao_tune_uintx_mfma", 1)
        for bits in range(1, 8):
            for n, k, g in ((4096, 4096, 64), (14336, 4096, 128), (1, 128, 32), (37, 384, 384)):
                assert routes(bits, n, k, g) == ON
        # unserved: groups that are no multiple of 32 keep dequantize + matmul
        for k, g in ((384, 48), (4096, 16), (3840, 80)):
            assert routes(3, 37, k, g) == OFF
        # the entry without a group size answers for a served one
        assert [_lib.lib().tao_uintx_linear_route(m, 37, 384, 3) for m in (8, 9)] == [1, 3]
        # max_gemv_m still moves the GEMV boundary; a forced route wins over the hook
        _lib.call("tao_tune_uintx", 0, 1, 0, 0, 0, 0, 0)
        assert routes() == [1] + [3] * 31
        for forced in (1, 2):
            _lib.call("tao_tune_uintx", forced, 0, 0, 0, 0, 0, 0)
            assert routes() == [forced] * 32
        _lib.call("tao_tune_uintx", 0, 0, 0, 0, 0, 0, 0)
        assert routes() == ON  # the 7-tuple knob leaves the hook alone
        _lib.call("tao_tune_uintx_mfma", 0)
        assert routes() == OFF
        for bad in (-1, 2):
            with pytest.raises(RuntimeError, match="tune: uintx mfma"):
                _lib.call("tao_tune_uintx_mfma", bad)
        _lib.call("tao_tune_uintx_mfma", 1)
    finally:
        _lib.call("tao_tune_reset")
    assert routes() == OFF


def test_tuning_knob_is_scoped():
    with tuning(uintx_mfma=1):
        assert routes() == ON
    assert routes() == OFF
