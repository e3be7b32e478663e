"""bench.py --dump-outputs on a one-layer stand-in for the Llama shapes: one float32 .npy per
linear holding the step's output row, equal to the CPU oracle's dequant linear on the same
weights, and identical when the step is rebuilt from the same seeds (what lets two builds be
compared output for output)."""

import os

import numpy as np
import pytest
import torch

import bench
from oracle import oracle

pytestmark = pytest.mark.gpu

# N = 256 (wqkv, wo, w2), 1280 (w1||w3) and a 1000-row head; K = 256 and 640
TINY = dict(dim=256, n_layer=1, n_head=2, n_kv_head=1, head_dim=64, intermediate=640, vocab=1000)
G = 32


def _dumped(tmp_path, tag):
    dev = torch.device("cuda", 0)
    lins = bench.llama_linears(TINY)
    st = bench.LinearStep(lins, ["whole"] * len(lins), 1, 0, G, dev, False)
    graph = st.capture()
    graph.replay()
    out = tmp_path / tag
    bench.dump_outputs(st, str(out))
    return lins, st, out


def test_dump_outputs_files_match_the_oracle_and_repeat(tmp_path):
    lins, st, a = _dumped(tmp_path, "a")
    assert sorted(os.listdir(a)) == sorted(f"{name}.npy" for name, _, _ in lins)
    for (name, N, K), entry in zip(lins, st.plan):
        y = np.load(a / f"{name}.npy")
        assert y.dtype == np.float32 and y.shape == (N,)
        packed, sz = entry[3], entry[4]
        q = torch.ops.torchao.int4_unpack(packed).cpu()
        s, z = sz[..., 0].cpu().contiguous(), sz[..., 1].cpu().contiguous()
        ref = oracle.int4_linear(st.xs[K].cpu(), q, s, z, G).float().reshape(-1)
        # bf16 outputs of a K <= 640 dot product in fp32: the smoke test's bar
        assert oracle.rel_l2(torch.from_numpy(y), ref) < 1e-2, name
    _, _, b = _dumped(tmp_path, "b")
    for name, _, _ in lins:
        assert np.array_equal(np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")), name
