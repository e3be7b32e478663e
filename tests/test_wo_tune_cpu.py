"""The tuning hooks and route rules of the NF4, FP6 and uintx weight-only linears through the C ABI:
every refusal of tao_tune_nf4 / tao_tune_fp6 / tao_tune_uintx with its full message, which of two
bad arguments is reported, that a refused call changes nothing, and that the three route rules
agree wherever they share inputs. No GPU: the hooks and the route queries are host code."""

import pytest

from torchao import _lib
from torchao.kernel.tuning import tuning

# hook -> (name in the messages, arguments after the five shared ones)
HOOKS = {"tao_tune_nf4": ("nf4", ()), "tao_tune_fp6": ("fp6", (0,)), "tao_tune_uintx": ("uintx", (0, 0))}

# (route, max_gemv_m, rows_per_wave, waves_k, row_groups) -> the message after "tune: <fmt> "
SHARED = [
    ((3, 0, 0, 0, 0), "route must be 0 (auto), 1 (gemv) or 2 (dequant + mm)"),
    ((-1, 0, 0, 0, 0), "route must be 0 (auto), 1 (gemv) or 2 (dequant + mm)"),
    ((0, -1, 0, 0, 0), "max_gemv_m must be >= 0"),
    ((0, 0, 3, 0, 0), "rows_per_wave must be 0, 2, 4 or 8"),
    ((0, 0, 0, 9, 0), "waves_k must be in [0, 8]"),
    ((0, 0, 0, 0, 9), "row_groups must be in [0, 8]"),
    ((0, 0, 0, 4, 4), "waves_k * row_groups must be <= 8"),
]
OWN = [
    ("tao_tune_fp6", (0, 0, 0, 0, 0, 3),
     "tune: fp6 chunk_groups must be 0 (built-in), 1 (24 B) or 2 (48 B)"),
    ("tao_tune_uintx", (0, 0, 0, 0, 0, 5, 0),
     "tune: uintx unit must be 0 (built-in), 4, 8 or 16 bytes"),
    ("tao_tune_uintx", (0, 0, 0, 0, 0, 0, 3),
     "tune: uintx x_lds must be 0 (built-in), 1 (through L1) or 2 (staged in LDS)"),
]
# two bad arguments in one call: the one that is reported
TWO = [
    ("tao_tune_nf4", (3, 0, 3, 0, 0),
     "tune: nf4 route must be 0 (auto), 1 (gemv) or 2 (dequant + mm)"),
    ("tao_tune_nf4", (0, -1, 0, 0, 9), "tune: nf4 max_gemv_m must be >= 0"),
    ("tao_tune_fp6", (0, 0, 0, 4, 4, 3), "tune: fp6 waves_k * row_groups must be <= 8"),
    ("tao_tune_fp6", (0, 0, 0, 9, 9, 0), "tune: fp6 waves_k must be in [0, 8]"),
    ("tao_tune_uintx", (0, 0, 3, 0, 0, 5, 0), "tune: uintx rows_per_wave must be 0, 2, 4 or 8"),
    ("tao_tune_uintx", (0, 0, 0, 0, 0, 5, 3),
     "tune: uintx unit must be 0 (built-in), 4, 8 or 16 bytes"),
]

N, K = 4096, 4096


def _refused(hook, args):
    """The status and tao_last_error() of a hook call that must be refused."""
    lib = _lib.lib()
    rc = getattr(lib, hook)(*args)
    assert rc != 0, f"{hook}{args} was accepted"
    return lib.tao_last_error().decode()


def _routes(m, bits=3, group=32):
    lib = _lib.lib()
    return (lib.tao_nf4_linear_route(m, N, K), lib.tao_fp6_linear_route(m, N, K),
            lib.tao_uintx_linear_route_g(m, N, K, bits, group))


@pytest.fixture(autouse=True)
def _built_in():
    _lib.call("tao_tune_reset")
    yield
    _lib.call("tao_tune_reset")


@pytest.mark.parametrize("hook", sorted(HOOKS))
@pytest.mark.parametrize("args,text", SHARED, ids=[str(a) for a, _ in SHARED])
def test_shared_refusals(hook, args, text):
    fmt, rest = HOOKS[hook]
    assert _refused(hook, args + rest) == f"tune: {fmt} {text}"


@pytest.mark.parametrize("hook,args,text", OWN, ids=[f"{h}{a}" for h, a, _ in OWN])
def test_own_refusals(hook, args, text):
    assert _refused(hook, args) == text


@pytest.mark.parametrize("hook,args,text", TWO, ids=[f"{h}{a}" for h, a, _ in TWO])
def test_first_of_two_bad_arguments_is_reported(hook, args, text):
    assert _refused(hook, args) == text


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_refused_call_leaves_the_tuning_in_force(hook):
    fmt, rest = HOOKS[hook]
    which = ("nf4", "fp6", "uintx").index(fmt)  # its place in _routes()
    _lib.call(hook, 2, 0, 0, 0, 0, *rest)  # every call to dequantize + matmul
    assert _routes(1)[which] == 2
    for args, _ in SHARED:
        _refused(hook, args + rest)
        assert _routes(1)[which] == 2
    for h, args, _ in OWN:
        if h == hook:
            _refused(h, args)
            assert _routes(1)[which] == 2
    _lib.call("tao_tune_reset")
    assert _routes(1)[which] == 1


def test_the_three_route_rules_agree():
    assert _routes(1) == (1, 1, 1) and _routes(512) == (2, 2, 2)  # built-in, hooks off
    for force in (1, 2):
        with tuning(nf4=(force, 0, 0, 0, 0), fp6=(force, 0, 0, 0, 0, 0),
                    uintx=(force, 0, 0, 0, 0, 0, 0)):
            assert _routes(1) == (force,) * 3 and _routes(512) == (force,) * 3
        # a forced route wins over the MFMA hooks too
        with tuning(fp6=(force, 0, 0, 0, 0, 0), uintx=(force, 0, 0, 0, 0, 0, 0), fp6_mfma=1,
                    uintx_mfma=1):
            assert _routes(512)[1:] == (force, force)
    with tuning(nf4=(0, 2, 0, 0, 0), fp6=(0, 2, 0, 0, 0, 0), uintx=(0, 2, 0, 0, 0, 0, 0)):
        assert _routes(2) == (1, 1, 1) and _routes(3) == (2, 2, 2)
    assert _routes(1) == (1, 1, 1)  # and the built-in rule is back


def test_mfma_hooks():
    # FP6 and uintx share the built-in boundary of 8 tokens: one past it goes to the MFMA GEMM
    assert _routes(8)[1:] == (1, 1) and _routes(9)[1:] == (2, 2)
    with tuning(fp6_mfma=1, uintx_mfma=1):
        assert _routes(8)[1:] == (1, 1) and _routes(9)[1:] == (3, 3)
        assert _routes(9)[0] == 2  # NF4 has no such hook
        # uintx only where the kernel serves the group size (a multiple of 32)
        assert _routes(9, group=16)[2] == 2 and _routes(9, group=32)[2] == 3
        assert _lib.lib().tao_uintx_linear_route(9, N, K, 3) == 3  # group size unknown: served
    with tuning(fp6=(0, 2, 0, 0, 0, 0), uintx=(0, 2, 0, 0, 0, 0, 0), fp6_mfma=1, uintx_mfma=1):
        assert _routes(2)[1:] == (1, 1) and _routes(3)[1:] == (3, 3)
    assert _routes(9)[1:] == (2, 2)
