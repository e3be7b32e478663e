"""The FP6 linear's MFMA route in the route rule (csrc/fp6_host.h) through the C ABI: the hook
tao_tune_fp6_mfma / tuning(fp6_mfma=1) turns every "dequantize + matmul" answer into "MFMA GEMM"
(3) and nothing else."""

import pytest

from torchao import _lib
from torchao.kernel.tuning import tuning

MS = (1, 8, 9, 512)


def routes(n=4096, k=4096):
    route = _lib.lib().tao_fp6_linear_route
    return [route(m, n, k) for m in MS]


def test_hook_turns_dequant_mm_into_mfma():
    _lib.call("tao_tune_reset")
    assert routes() == [1, 1, 2, 2]
    try:
        _lib.call("tao_tune_fp6_mfma", 1)
        for n, k in ((4096, 4096), (14336, 4096), (1, 64)):
            assert routes(n, k) == [1, 1, 3, 3]
        # max_gemv_m still moves the GEMV boundary; a forced route wins over the hook
        _lib.call("tao_tune_fp6", 0, 1, 0, 0, 0, 0)
        assert routes() == [1, 3, 3, 3]
        for forced in (1, 2):
            _lib.call("tao_tune_fp6", forced, 0, 0, 0, 0, 0)
            assert routes() == [forced] * 4
        _lib.call("tao_tune_fp6", 0, 0, 0, 0, 0, 0)
        assert routes() == [1, 1, 3, 3]
        _lib.call("tao_tune_fp6_mfma", 0)
        assert routes() == [1, 1, 2, 2]
        for bad in (-1, 2):
            with pytest.raises(RuntimeError, match="tune: fp6 mfma"):
                _lib.call("tao_tune_fp6_mfma", bad)
        _lib.call("tao_tune_fp6_mfma", 1)
    finally:
        _lib.call("tao_tune_reset")
    assert routes() == [1, 1, 2, 2]


def test_tuning_knob_is_scoped():
    with tuning(fp6_mfma=1):
        assert routes() == [1, 1, 3, 3]
    assert routes() == [1, 1, 2, 2]
