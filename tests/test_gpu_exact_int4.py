"""Bit-exact GPU tests of every route of torch.ops.torchao.int4_weight_only_linear.

A hard gate with no tolerance to tune: the inputs (tests/exact_inputs.py) make every product and
every partial sum an exact fp32 number, so the kernels' accumulation orders cannot matter and the
output must equal the float64 reference rounded once to bf16, bit for bit (the two conditions, bf16
representability and T < 2^24, and the CPU proof of order independence: exact_inputs.py,
test_exact_inputs_cpu.py). An aggregate norm cannot see a fault confined to one row, one
quantisation group or one tail lane; torch.equal does. A mismatch here is a kernel (or op
wrapper) bug by construction; the "probe" family's failing (m, n) and its probed k locate it.

Routes: the M = 1 GEMV under every branch of its built-in launch-shape choice and under forced
launch shapes, the GEMV at M > 1, the 16x16x32 and 32x32x16 MFMA kernels (built-in and forced
tiles, split-K), the weight-shared tile kernel, the single-fetch kernels (both seams, loader
waves, asymmetric slices, the fenced hand-off), and the chained entry points (the decode entry,
the grouped MoE GEMV, a replayed graph). Both families, bias on and off.
"""

import functools

import pytest
import torch

import exact_inputs as E

from torchao import _lib
from torchao.kernel import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROBE_SEEDS_M1 = 4  # at M = 1 the probe family runs 4 seeds (4 sets of probed k)


def _sf_status_clean():
    st = torch.zeros(1, dtype=torch.int32)
    _lib.call("tao_gemm_sf_status", st.data_ptr())
    assert int(st.item()) == 0, "gemm_sf reducer poll timed out"


def _last_kernel():
    return _lib.lib().tao_last_kernel().decode()


@functools.lru_cache(maxsize=8)
def _inputs(M, N, K, g, families=E.FAMILIES):
    """[(label, x, packed, sz, bias, want, want_with_bias)] on the device / CPU, made once per
    shape and shared by the cases that use it (never modified)."""
    seed = (M * 31 + N * 7 + K + g) % 1000
    q = E.make_q(N, K, seed)
    packed = torch.ops.torchao.int4_pack(q.to(DEV))
    bias = E.make_bias(N, seed)
    out = []
    for family in families:
        n_seeds = PROBE_SEEDS_M1 if (family == "probe" and M == 1) else 1
        for i in range(n_seeds):
            _, s, z, x = E.make_int4_exact(M, N, K, g, seed + 1000 * i, family, q=q)
            want = E.ref_int4(x, q, s, z, g)
            sz = torch.stack([s, z], dim=-1).contiguous().to(DEV)
            out.append((f"{family}[{i}]", x.to(DEV), packed, sz, bias.to(DEV), want,
                        E.add_bias(want, bias)))
    return tuple(out)


def _linear(x, packed, sz, g, bias):
    return torch.ops.torchao.int4_weight_only_linear(x, packed, sz, g, bias)


def check(route, M, N, K, g, run=_linear, with_bias=True, families=E.FAMILIES):
    """Every input set of the shape through `run`, bias off and on, torch.equal to the reference."""
    for label, x, packed, sz, bias, want, want_b in _inputs(M, N, K, g, families):
        for b, ref in ((None, want), (bias, want_b)) if with_bias else ((None, want),):
            got = run(x, packed, sz, g, b).cpu()
            where = f"{route} M={M} N={N} K={K} g={g} {label} bias={'on' if b is not None else 'off'}"
            assert got.shape == ref.shape, where
            assert torch.equal(got, ref), E.describe_mismatch(
                f"{where} kernel={_last_kernel()}", got, ref)


# ---- M = 1: the GEMV on its built-in launch shapes -------------------------------------------------

@pytest.mark.parametrize("N,K,g", E.M1_ROUTED)
def test_m1_built_in_routing(N, K, g):
    check("gemv m1", 1, N, K, g)


@pytest.mark.parametrize("N,K,g", E.M1_GROUPS)
def test_m1_group_sizes(N, K, g):
    check("gemv m1", 1, N, K, g)


# ---- M = 1: forced launch shapes ---------------------------------------------------------------------

@pytest.mark.parametrize("rpw,wk,rg,occ", E.GEMV_FORCED_SHAPES)
def test_m1_forced_launch_shapes(rpw, wk, rg, occ):
    with tuning(int4_gemv=(rpw, wk, rg, occ)):
        for N, K in E.GEMV_FORCED_NK:
            check(f"gemv m1 forced rpw={rpw} wk={wk} g={rg} occ={occ}", 1, N, K, 32)


@pytest.mark.parametrize("N,K", E.XLDS_NK)
def test_m1_x_staged_in_lds(N, K):
    # (with a bias the knob does not apply and the plain kernel runs: checked all the same)
    with tuning(int4_xlds=1):
        check("gemv m1 xlds", 1, N, K, 32)


# ---- the GEMV at M > 1 --------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K,g", E.GEMV_MULTI_M)
def test_gemv_multi_m(M, N, K, g):
    with tuning(linear_crossover=8):
        check("gemv", M, N, K, g)
        assert "gemv" in _last_kernel()


# ---- MFMA 16x16x32 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", E.MFMA_NK)
@pytest.mark.parametrize("M", E.MFMA16_M)
def test_mfma16_built_in_routing(M, N, K):
    check("mfma built-in", M, N, K, 32)


@pytest.mark.parametrize("bm,kg,splits", E.FORCED_TILES)
@pytest.mark.parametrize("M,N,K", E.FORCED_MNK)
def test_mfma16_forced_tiles_and_split_k(bm, kg, splits, M, N, K):
    with tuning(gemm=(bm, kg, splits)):
        check(f"mfma16 bm={bm} kg={kg} splits={splits}", M, N, K, 32)
        assert "gemm_mfma" in _last_kernel()


@pytest.mark.parametrize("knob,value", [("gemm_nw", 2), ("gemm_order", 1), ("gemm_table", 1)])
def test_mfma16_variants(knob, value):
    with tuning(**{knob: value}):
        check(f"mfma16 {knob}={value}", 70, 200, 1056, 32)


@pytest.mark.parametrize("g", E.GROUPS)
def test_mfma16_group_sizes(g):
    with tuning(gemm=(16, 2, 3)):
        check("mfma16 bm=16 kg=2 splits=3", 70, 200, 2048, g)
    check("mfma built-in", 70, 200, 2048, g)


def test_mfma16_split_k_fenced():
    with tuning(gemm=(16, 1, 8), splitk_fenced=1):
        check("mfma16 split-K fenced", 70, 200, 2048, 32)


# ---- MFMA 32x32x16 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("g", [32, 256])
@pytest.mark.parametrize("N,K", E.MFMA_NK)
@pytest.mark.parametrize("M", E.MFMA32_M)
def test_mfma32(M, N, K, g, splits):
    K = E.round_up(K, g)
    with tuning(linear_crossover=1, int4_mfma32=1, gemm=(0, 0, splits)):
        check(f"mfma32 splits={splits}", M, N, K, g)
        assert "gemm32" in _last_kernel()


# ---- the weight-shared tile kernel ------------------------------------------------------------------------

@pytest.mark.parametrize("splits", E.TILE_SPLITS)
@pytest.mark.parametrize("g", [32, 64])
@pytest.mark.parametrize("M,N,K", E.TILE_MNK)
def test_tile_kernel(splits, M, N, K, g):
    with tuning(gemm_tile=(2, splits)):
        check(f"tile splits={splits}", M, N, K, g)
        assert "tile" in _last_kernel()


# ---- the single-fetch kernels --------------------------------------------------------------------------------

def _seams(cfg):
    """The spread seam exists on the 16x16 kernel (wm > 1) at 2 / 4 / 8 slices only."""
    bn, wm, splits = cfg[:3]
    return (0, 1) if wm != 1 and splits in (2, 4, 8) else (0,)


@pytest.mark.parametrize("cfg", E.SF_CFGS)
@pytest.mark.parametrize("M,N,K", E.SF_MNK)
def test_single_fetch(cfg, M, N, K):
    for seam in _seams(cfg):
        with tuning(gemm_sf=(2, *cfg, 0), gemm_sf_seam=seam):
            check(f"sf cfg={cfg} seam={seam}", M, N, K, 32)
            # (above one 128-row tile the forced mode leaves the shape to the MFMA kernels)
            assert M > 128 or "gemm_sf" in _last_kernel()
        _sf_status_clean()


# loader waves: once per kernel family (16x16: 64-column tiles; 32x32x16: 64 / 128 columns at 3
# stages); (bn, wm, splits, stages, a_steps)
@pytest.mark.parametrize("loaders", [1, 2, 3])
@pytest.mark.parametrize("cfg", [(64, 2, 4, 3, 0), (128, 1, 4, 3, 0)])
def test_single_fetch_loader_waves(cfg, loaders):
    with tuning(gemm_sf=(2, *cfg, 0), gemm_sf_seam=0, gemm_sf_loaders=loaders):
        check(f"sf cfg={cfg} loaders={loaders}", 100, 200, 3072, 32)
        assert "gemm_sf" in _last_kernel()
    _sf_status_clean()


def test_single_fetch_loader_waves_rejected_off_three_stages():
    """The one knob combination of this file the library refuses: loader waves on the 32x32x16
    kernel at a stage count it has no kernel for. It must say so, not run something else."""
    _, x, packed, sz, _, _, _ = _inputs(100, 200, 3072, 32)[0]
    with tuning(gemm_sf=(2, 128, 1, 4, 2, 0, 0), gemm_sf_loaders=2):
        with pytest.raises(RuntimeError, match="loader waves need 3 stages"):
            _linear(x, packed, sz, 32, None)


@pytest.mark.parametrize("g", E.GROUPS)
@pytest.mark.parametrize("cfg", [(64, 2, 4, 3, 0), (128, 1, 4, 3, 0)])
def test_single_fetch_group_sizes(cfg, g):
    with tuning(gemm_sf=(2, *cfg, 0)):
        check(f"sf cfg={cfg}", *E.SF_GROUPS_MNK, g)
    _sf_status_clean()


@pytest.mark.parametrize("a_steps", [1, 3])
def test_single_fetch_asymmetric_slices(a_steps):
    for wm in (2, 1):
        with tuning(gemm_sf=(2, 64, wm, 4, 3, a_steps, 0)):
            check(f"sf wm={wm} a_steps={a_steps}", 100, 200, 3072, 32)
    _sf_status_clean()


def test_single_fetch_split_k_fenced():
    with tuning(gemm_sf=(2, 64, 2, 4, 3, 0, 0), splitk_fenced=1):
        check("sf fenced", 100, 200, 3072, 32)
    _sf_status_clean()


# ---- chained entry points: each against the reference directly ----------------------------------------------

def test_decode_entry_plain():
    from torchao._models.llama import kernels

    N, K = E.CHAINED_NK
    check("int4_decode", 1, N, K, 32, with_bias=False, families=("dense",),
          run=lambda x, packed, sz, g, b: kernels.int4_decode(x, packed, sz, g))


def test_grouped_decode_three_experts():
    from torchao._models.llama import kernels

    (N, K), g, nE = E.CHAINED_NK, 32, 3
    qs, ss, zs = [], [], []
    for e in range(nE):
        q, s, z, x = E.make_int4_exact(nE, N, K, g, seed=40 + e, family="dense")
        qs.append(q), ss.append(s), zs.append(z)
    # x of the last maker, one row per activated expert; the conditions hold against every expert
    for e in range(nE):
        E.check_int4_exact(x, qs[e], ss[e], zs[e], g)
    packed = torch.stack([torch.ops.torchao.int4_pack(q.to(DEV)) for q in qs]).contiguous()
    sz = torch.stack([torch.stack([s, z], dim=-1) for s, z in zip(ss, zs)]).contiguous().to(DEV)
    idx = torch.tensor([2, 0, 1], dtype=torch.int64)
    y = kernels.int4_grouped_decode(x.to(DEV), packed, sz, g, idx.to(DEV)).cpu()
    for a, e in enumerate(idx.tolist()):
        want = E.ref_int4(x[a:a + 1], qs[e], ss[e], zs[e], g)
        assert torch.equal(y[a:a + 1], want), E.describe_mismatch(
            f"grouped decode row {a} expert {e}", y[a:a + 1], want)
    # the shared-x form: one row for every expert
    y1 = kernels.int4_grouped_decode(x[:1].contiguous().to(DEV), packed, sz, g, idx.to(DEV)).cpu()
    for a, e in enumerate(idx.tolist()):
        want = E.ref_int4(x[:1], qs[e], ss[e], zs[e], g)
        assert torch.equal(y1[a:a + 1], want), E.describe_mismatch(
            f"grouped decode shared x, expert {e}", y1[a:a + 1], want)


def test_graph_replay_of_m1_linear():
    N, K = E.CHAINED_NK
    label, x, packed, sz, bias, want, _ = _inputs(1, N, K, 32)[0]
    _linear(x, packed, sz, 32, None)  # eager warm-up outside the capture
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = _linear(x, packed, sz, 32, None)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, want), E.describe_mismatch(f"graph replay {label}", got, want)


# ---- the gate bites: single-edge faults fed through the real kernel ---------------------------------------

def test_single_edge_faults_change_exactly_their_output():
    """The kernel run on weights carrying one fault (the last row takes its neighbour's (scale,
    zero) for its last group; two nibbles of one dword swapped at a probed k) differs from the
    reference of the intact weights in exactly that row's output and nowhere else: the probed k
    reach the output bits, and the comparison above would flag a kernel that made such a slip."""
    M, N, K, g = 1, 37, 2080, 32
    q, s, z, x = E.make_int4_exact(M, N, K, g, seed=5, family="probe")
    want = E.ref_int4(x, q, s, z, g)
    xd = x.to(DEV)

    def run(q_, s_, z_):
        sz = torch.stack([s_, z_], dim=-1).contiguous().to(DEV)
        return _linear(xd, torch.ops.torchao.int4_pack(q_.to(DEV)), sz, g, None).cpu()

    assert torch.equal(run(q, s, z), want)
    s1, z1 = s.clone(), z.clone()
    s1[N - 1, -1], z1[N - 1, -1] = s[N - 2, -1], z[N - 2, -1]
    assert (run(q, s1, z1) != want).nonzero().tolist() == [[0, N - 1]]
    n, k1 = N // 2, K - 1  # k = K - 1 is probed in every row of x
    k0 = next(k for k in range(K - 8, K - 1)
              if float(x[0, k]) == 0 and int(q[n, k]) != int(q[n, k1]))
    q2 = q.clone()
    q2[n, k0], q2[n, k1] = q[n, k1], q[n, k0]
    assert (run(q2, s, z) != want).nonzero().tolist() == [[0, n]]
