"""The leaf step's per-size tally (kernels/deep.hip leaf_step) on a clique, on the GPU.

12 items present in all T transactions (8 noise items in one transaction each never reach the
support), so every subset of every class survives: a leaf step then runs all its passes with every
lane tallying, classes of every size 2..8 occur, and ``per_level[k]`` must be C(12, k) exactly.
T = 64 is a block of one word, 1000 the widest tier a leaf step is built for (16 words) and 1100 a
wider one (24 words), where the classes take the row / batch steps whatever the hook says.
``leaf_m`` comes from the test hook ``deep_leaf_m``; ``max_len`` cuts inside the leaf classes.
"""
from math import comb

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLIQUE, NOISE = 12, 8
LEAF_T_MAX = 16 * 64  # transactions of the widest block a leaf step takes (kLeafTier words)

_cache = {}


def _data(gpu_mod, T):
    """(a loaded miner, CSR arrays) of the clique over T transactions: built once, shared."""
    if T not in _cache:
        rows = []
        for t in range(T):
            row = list(range(CLIQUE))
            if t < NOISE:
                row.append(CLIQUE + t)
            rows.append(row)
        ptr = np.zeros(T + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(r) for r in rows])
        items = np.array([i for r in rows for i in r], dtype=np.int32)
        g = gpu_mod.GpuMiner(0)
        g.load_csr(ptr, items, CLIQUE + NOISE)
        _cache[T] = (g, ptr, items)
    return _cache[T]


def _ref(gpu_mod, T, max_len):
    key = (T, max_len)
    if key not in _cache:
        _, ptr, items = _data(gpu_mod, T)
        _cache[key] = gpu_mod.mine_cpu_count(ptr, items, CLIQUE + NOISE, 0.5, max_len)
    return _cache[key]


@pytest.mark.parametrize("max_len", [0, 5, 9])
@pytest.mark.parametrize("leaf_m", [0, 2, 5, 6, 7, 8])
@pytest.mark.parametrize("T", [64, 1000, 1100])
def test_clique_tally(gpu_mod, monkeypatch, T, leaf_m, max_len):
    g, _, _ = _data(gpu_mod, T)
    ref = _ref(gpu_mod, T, max_len)
    monkeypatch.setenv("KMLS_TEST_HOOKS", f"deep_leaf_m={leaf_m}")
    d = g.mine_deep(0.5, max_len=max_len)
    cap = max_len if max_len else CLIQUE
    per = [int(x) for x in d["per_level"]]
    print(T, leaf_m, max_len, per[:CLIQUE + 2], {k: d[k] for k in (
        "candidates", "leaf_candidates", "leaf_steps", "batch_steps", "row_steps")})
    for k in range(1, cap + 1):
        assert per[k] == comb(CLIQUE, k), (k, per)
    assert all(x == 0 for x in per[cap + 1:]), per
    assert d["n_itemsets"] == ref["n_itemsets"] == sum(comb(CLIQUE, k) for k in range(1, cap + 1))
    assert d["digest"] == ref["digest"]
    fits = T <= LEAF_T_MAX  # (every row is full, so no projection narrows a block)
    assert (d["leaf_candidates"] == 0) == (leaf_m == 0 or not fits), d["leaf_candidates"]
    assert d["leaf_candidates"] <= d["candidates"]
    assert d["leaf_steps"] + d["batch_steps"] + d["row_steps"] > 0
    assert (d["leaf_steps"] == 0) == (d["leaf_candidates"] == 0)
    if leaf_m == 0:
        assert d["leaf_steps"] == 0
