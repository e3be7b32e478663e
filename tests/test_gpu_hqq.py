"""GPU tests of the fused HQQ int4 quantizer (csrc/hqq.hip, torchao::int4_hqq_quantize_pack,
tao_int4_hqq_quantize_bf16) against the reference's CPU results (tests/golden/hqq_*.npz,
experiments/gen_golden_hqq.py), through the op and through the C ABI.

The scale does not depend on the iteration: its bits equal the reference's exactly, and so does
the number of iterations run (the fixtures keep every comparison of the stop rule 3e-5 apart).
The iteration is discontinuous, so codes and zeros follow the *moved groups* rule: the share of
groups in which any code or the bf16 zero differs from the reference's is at most twice the
fixture's ``moved_model`` (the share that moves when every new zero of the reference's own loop
is moved by one fp32 ulp; the factor because the device pow may be 2 ulp off where the model
moves 1), and within a moved group codes differ by at most 1 and zeros by at most the group's
scale. Each test prints its measured share and the relative gap of the mean |W - W^| to the
fixture's before asserting.

Measured on the MI355X (share of moved groups, cap, relative gap of the mean |W - W^|):
see DESIGN.md §4.22 (all within the cap; every moved group differs in its bf16 zero alone)."""

import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import bf16, load_golden

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, TensorCoreTiledAQTTensorImpl
from torchao.quantization import Int4WeightOnlyConfig, quantize_
from torchao.quantization.quant_primitives import _choose_qparams_and_quantize_affine_hqq

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.ops.torchao
TOL_REF = 1e-2   # tests/test_gpu_int4.py: bf16 output against the bf16 dequantized product
FIXTURES = ["hqq_N64_K256_g32.npz", "hqq_N96_K1024_g64.npz", "hqq_N48_K512_g128.npz",
            "hqq_N40_K2048_g256.npz"]
TAIL = "hqq_N40_K352_g32.npz"  # 1760 eight-weight pieces: 6 workgroups and 224 tail threads


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _plain(packed, sz):
    """(codes uint8 [R, K], scale bf16 [R, K/g], zero bf16 [R, K/g]) on the CPU."""
    K8 = packed.shape[-1]
    q = T.int4_unpack(packed.reshape(-1, K8).contiguous()).cpu().to(torch.uint8)
    sz = sz.reshape(q.shape[0], -1, 2).cpu()
    return q, sz[..., 0].contiguous(), sz[..., 1].contiguous()


def _via_op(w, g):
    packed, sz, it = T.int4_hqq_quantize_pack(w.to(DEV), g)
    return packed, sz, int(it.item())


def _via_capi(w, g):
    w = w.to(DEV).contiguous()
    N, K = w.shape
    packed = torch.empty(N, K // 8, dtype=torch.int32, device=DEV)
    sz = torch.empty(N, K // g, 2, dtype=torch.bfloat16, device=DEV)
    it = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    nbytes = _lib.lib().tao_int4_hqq_scratch_bytes(N, K)
    assert nbytes == (N * K // 8 + 255) // 256 * 20 * 8
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.call("tao_int4_hqq_quantize_bf16", p(w), p(packed), p(sz), p(it), p(scratch), N, K, g,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return packed, sz, int(it.item())


ROUTES = {"op": _via_op, "capi": _via_capi}


@functools.lru_cache(maxsize=None)
def _result(name, route):
    rec = load_golden(name)
    packed, sz, it = ROUTES[route](bf16(rec["w"]), int(rec["g"]))
    return packed, sz, it


def _mean_err(w, q, s, z, g):
    N, K = w.shape
    deq = (q.double().reshape(N, K // g, g) - 8) * s.double()[..., None] + z.double()[..., None]
    return float((w.double() - deq.reshape(N, K)).abs().mean())


def _check_moved(q, s, z, q_ref, s_ref, z_ref, g, cap, what):
    """The moved-groups rule; returns the share. q uint8 [N, K], s / z bf16 [N, K/g]."""
    N, K = q.shape
    assert np.array_equal(_bits(s), _bits(s_ref)), f"{what}: scale bits differ"
    dq = (q.int() - q_ref.int()).reshape(N, K // g, g)
    dz = torch.from_numpy(_bits(z) != _bits(z_ref))
    moved = (dq != 0).any(-1) | dz
    share = float(moved.float().mean())
    print(f"{what}: moved groups {int(moved.sum())} of {moved.numel()} = {share:.5f} "
          f"(cap {cap:.5f}), codes changed {float((dq != 0).float().mean()):.2e}")
    assert int(dq.abs().max()) <= 1, f"{what}: a code moved by more than one step"
    assert bool(((z.float() - z_ref.float()).abs() <= s_ref.float()).all()), \
        f"{what}: a zero moved by more than the group's scale"
    assert share <= cap, f"{what}: {share} of the groups moved, cap {cap}"
    return share


@pytest.mark.parametrize("route", ["op", "capi"])
@pytest.mark.parametrize("name", FIXTURES + [TAIL])
def test_fixture_scales_iterations_and_moved_groups(name, route):
    """All four lanes-per-group instantiations (g = 32, 64, 128, 256) and the tail shape."""
    rec = load_golden(name)
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    packed, sz, it = _result(name, route)
    assert packed.shape == (N, K // 8) and packed.dtype == torch.int32
    assert sz.shape == (N, K // g, 2) and sz.dtype == torch.bfloat16
    q, s, z = _plain(packed, sz)
    w = bf16(rec["w"])
    err = _mean_err(w, q, s, z, g)
    gap = err / float(rec["mean_err_hqq"]) - 1
    print(f"{name} {route}: iters {it} (fixture {int(rec['iters'])}), mean |W - W^| {err:.6e}, "
          f"relative gap to the fixture's {gap:+.2e}, plain {float(rec['mean_err_plain']):.6e}")
    assert np.array_equal(_bits(s), rec["s"]), "scale bits differ"
    assert it == int(rec["iters"])
    assert err < float(rec["mean_err_plain"]), "HQQ's mean |W - W^| is not below plain's"
    _check_moved(q, s, z, torch.from_numpy(rec["q"]), bf16(rec["s"]), bf16(rec["z"]), g,
                 2 * float(rec["moved_model"]), f"{name} {route}")


def test_tail_shape_against_the_plain_torch_function():
    """N40 x K352 at g = 32 against this package's CPU function (which the CPU tests hold to the
    reference bit for bit), under the same rule."""
    rec = load_golden(TAIL)
    w, g = bf16(rec["w"]), 32
    q_ref, s_ref, z_ref, _ = _choose_qparams_and_quantize_affine_hqq(
        w, nbits=4, group_size=g, axis=1, compute_dtype=torch.bfloat16, device="cpu")
    q, s, z = _plain(*_result(TAIL, "op")[:2])
    _check_moved(q, s, z, q_ref, s_ref.reshape(s.shape), z_ref.reshape(z.shape), g,
                 2 * float(rec["moved_model"]), "tail vs the CPU function")


@pytest.mark.parametrize("route", ["op", "capi"])
def test_edge_rows_scales_are_exact(route):
    rec = load_golden("hqq_quant_edges.npz")
    packed, sz, it = ROUTES[route](bf16(rec["w"]), 32)
    q, s, z = _plain(packed, sz)
    assert np.array_equal(_bits(s), rec["s"]), "scale bits differ"
    assert it == int(rec["iters"])
    assert bool(torch.isfinite(z.float()).all()) and int(q.max()) <= 15
    dq = (q.int() - torch.from_numpy(rec["q"]).int()).abs()
    dz = _bits(z) != rec["z"]
    print(f"edges {route}: codes differing {int((dq != 0).sum())}, zeros differing {int(dz.sum())}")
    assert int(dq.max()) <= 1
    assert bool(((z.float() - bf16(rec["z"]).float()).abs() <= s.float()).all())


def test_two_calls_are_bit_equal_and_the_next_shape_is_correct():
    """Run-to-run equality, then a different shape right after (the allocator hands the scratch
    of the first call to the second) equals that shape's own first result."""
    a, b = FIXTURES[1], FIXTURES[0]
    ra, rb = load_golden(a), load_golden(b)
    wa, wb = bf16(ra["w"]).to(DEV), bf16(rb["w"]).to(DEV)
    p1, s1, i1 = T.int4_hqq_quantize_pack(wa, int(ra["g"]))
    p2, s2, i2 = T.int4_hqq_quantize_pack(wa, int(ra["g"]))
    p3, s3, i3 = T.int4_hqq_quantize_pack(wb, int(rb["g"]))
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int16), s2.view(torch.int16))
    assert torch.equal(i1, i2)
    want_p, want_s, want_i = _result(b, "op")
    assert torch.equal(p3, want_p) and torch.equal(s3.view(torch.int16), want_s.view(torch.int16))
    assert int(i3.item()) == want_i == int(rb["iters"])
    assert np.array_equal(_bits(_plain(p3, s3)[1]), rb["s"])


def test_3d_weight_equals_the_2d_call_on_the_stacked_rows():
    rec = load_golden(FIXTURES[0])
    w = bf16(rec["w"]).to(DEV)
    N, K = w.shape
    p3, s3, i3 = T.int4_hqq_quantize_pack(w.view(2, N // 2, K), 32)
    p2, s2, i2 = _result(FIXTURES[0], "op")
    assert p3.shape == (2, N // 2, K // 8) and s3.shape == (2, N // 2, K // 32, 2)
    assert torch.equal(p3.view(N, -1), p2)
    assert torch.equal(s3.view(N, -1, 2).view(torch.int16), s2.view(torch.int16))
    assert int(i3.item()) == i2


def test_capi_checks_arguments_before_any_device_work():
    w = torch.zeros(8, 96, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(8, 12, dtype=torch.int32, device=DEV)
    sz = torch.zeros(8, 3, 2, dtype=torch.bfloat16, device=DEV)
    it = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for g, msg in ((48, "group_size"), (64, "group_size")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("tao_int4_hqq_quantize_bf16", p(w), p(out), p(sz), p(it), p(scratch), 8, 96,
                      g, st)
    with pytest.raises(RuntimeError, match="aligned"):
        _lib.call("tao_int4_hqq_quantize_bf16", ctypes.c_void_p(w.data_ptr() + 2), p(out), p(sz),
                  p(it), p(scratch), 8, 96, 32, st)
    with pytest.raises(RuntimeError, match="scratch"):
        _lib.call("tao_int4_hqq_quantize_bf16", p(w), p(out), p(sz), p(it), ctypes.c_void_p(0), 8,
                  96, 32, st)
    torch.cuda.synchronize()
    assert int(it.item()) == -7 and int(out.abs().sum()) == 0
    with pytest.raises(RuntimeError, match="bf16"):
        T.int4_hqq_quantize_pack(w.float(), 32)
    with pytest.raises(RuntimeError, match="group_size"):
        T.int4_hqq_quantize_pack(w, 48)


def test_graph_replay_equals_eager():
    """Captured on a side stream and replayed on a second weight: nothing in the op synchronises
    or reads on the host, and the stop decision is remade on the device at every replay."""
    ra, rb = load_golden(FIXTURES[0]), load_golden(TAIL)
    first = bf16(ra["w"])[:40, :].repeat(1, 2)[:, :352].contiguous()  # another weight, same shape
    second = bf16(rb["w"])
    buf = first.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.int4_hqq_quantize_pack(buf, 32)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = T.int4_hqq_quantize_pack(buf, 32)
    torch.cuda.current_stream().wait_stream(s)
    for w in (second, first):
        want = T.int4_hqq_quantize_pack(w.to(DEV), 32)
        buf.copy_(w)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0])
        assert torch.equal(out[1].view(torch.int16), want[1].view(torch.int16))
        assert torch.equal(out[2], want[2])


def test_opcheck():
    w = bf16(load_golden(FIXTURES[0])["w"]).to(DEV)
    torch.library.opcheck(T.int4_hqq_quantize_pack.default, (w, 32))
    torch.library.opcheck(T.int4_hqq_quantize_pack.default, (w.view(2, 32, 256), 64))


def _rel_l2(y, ref):
    y, ref = y.detach().cpu().double(), ref.detach().cpu().double()
    return float((y - ref).norm() / ref.norm())


@pytest.mark.parametrize("name", [FIXTURES[0], FIXTURES[2]])
def test_quantize_on_a_gpu_linear(name):
    rec = load_golden(name)
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
    quantize_(lin, Int4WeightOnlyConfig(group_size=g, use_hqq=True))
    wt = lin.weight
    assert isinstance(wt, AffineQuantizedTensor)
    impl = wt.tensor_impl
    assert isinstance(impl, TensorCoreTiledAQTTensorImpl)
    want_p, want_s, _ = _result(name, "op")
    assert torch.equal(impl.packed_weight, want_p)
    assert torch.equal(impl.scale_and_zero.view(torch.int16), want_s.view(torch.int16))
    deq = wt.dequantize()
    for M in (1, 5):
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(DEV)
        with torch.no_grad():
            y = lin(x)
        direct = T.int4_weight_only_linear(x, impl.packed_weight, impl.scale_and_zero, g, None)
        assert torch.equal(y, direct), M
        e_bf16 = _rel_l2(y, F.linear(x, deq))
        e_f64 = _rel_l2(y, x.double().cpu() @ deq.double().cpu().t())
        print(f"{name} M={M}: rel-L2 vs the bf16 product {e_bf16:.3e}, vs float64 {e_f64:.3e}")
        assert e_bf16 < TOL_REF


def test_non_bf16_gpu_weight_takes_the_plain_torch_function():
    """fp16 weights are not the kernel's: the fp32 torch-op function runs on the GPU and the
    layout's own pack follows; the result obeys the same rule against the CPU's."""
    rec = load_golden(FIXTURES[0])
    w = bf16(rec["w"]).to(torch.float16)
    got = _choose_qparams_and_quantize_affine_hqq(w.to(DEV), group_size=32, device=DEV,
                                                  compute_dtype=torch.float16)
    want = _choose_qparams_and_quantize_affine_hqq(w, group_size=32, device="cpu",
                                                   compute_dtype=torch.float16)
    assert got[0].is_cuda and got[1].dtype == torch.float16
    assert torch.equal(got[1].cpu(), want[1])
    assert int((got[0].cpu().int() - want[0].int()).abs().max()) <= 1


def test_awq_composition_runs():
    from torchao.prototype.awq import AWQConfig

    rec = load_golden("awq_N64_K256_g32.npz")
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    model = torch.nn.Sequential(lin)
    base = Int4WeightOnlyConfig(group_size=32, use_hqq=True)
    quantize_(model, AWQConfig(base, step="prepare", scale_search_space_size=3))
    with torch.no_grad():
        model(bf16(rec["calib"]).to(DEV))
    quantize_(model, AWQConfig(base, step="convert", scale_search_space_size=3))
    x = bf16(rec["x"]).to(DEV)
    with torch.no_grad():
        y = model(x)
    assert y.shape == (x.shape[0], N) and bool(torch.isfinite(y.float()).all())
    assert float(y.float().abs().max()) > 0


def test_moe_composition_and_fused_gate_up_run():
    from torchao.prototype.moe_quant import (MOEFeedForwardAOQuantizable, MoEQuantConfig,
                                             cond_ffn_filter)
    from torchao.quantization import fuse_gate_up_

    E_, A_, D_, I_ = 4, 2, 256, 512  # tests/test_gpu_moe.py
    gen = torch.Generator().manual_seed(31)
    m = MOEFeedForwardAOQuantizable(D_, I_, E_, A_).to(torch.bfloat16)
    with torch.no_grad():
        m.router.weight.copy_(torch.randn(E_, D_, generator=gen) * 0.5)
        m.experts.w1.copy_(torch.randn(E_, I_, D_, generator=gen) / D_ ** 0.5)
        m.experts.w2.copy_(torch.randn(E_, D_, I_, generator=gen) / I_ ** 0.5)
        m.experts.w3.copy_(torch.randn(E_, I_, D_, generator=gen) / D_ ** 0.5)
    m = m.to(DEV)
    quantize_(m, MoEQuantConfig(Int4WeightOnlyConfig(group_size=32, use_hqq=True)),
              cond_ffn_filter)
    for n in ("w1", "w2", "w3"):
        assert isinstance(getattr(m.experts, n), AffineQuantizedTensor)
    for Tn in (5, 1):
        x = torch.randn(Tn, 1, D_, generator=gen).to(torch.bfloat16).to(DEV)
        with torch.no_grad():
            y = m(x)
        assert y.shape == x.shape and bool(torch.isfinite(y.float()).all())

    class FeedForward(torch.nn.Module):
        def __init__(self, d, h):
            super().__init__()
            self.w1 = torch.nn.Linear(d, h, bias=False)
            self.w3 = torch.nn.Linear(d, h, bias=False)
            self.w2 = torch.nn.Linear(h, d, bias=False)

        def forward(self, x):
            return self.w2(F.silu(self.w1(x)) * self.w3(x))

    torch.manual_seed(1)
    ff = FeedForward(256, 512).to(device=DEV, dtype=torch.bfloat16)
    x = torch.randn(5, 256, device=DEV, dtype=torch.bfloat16)
    assert fuse_gate_up_(ff) == 1
    quantize_(ff, Int4WeightOnlyConfig(group_size=32, use_hqq=True))
    with torch.no_grad():
        y = ff(x)
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0


def test_decode_status_stays_clean():
    from torchao._models.llama import kernels

    T.int4_hqq_quantize_pack(bf16(load_golden(FIXTURES[0])["w"]).to(DEV), 32)
    kernels.check_decode_status()
