"""Closed / maximal itemset flags on the GPU (csrc/kernels/closed.hip): the uploaded host trie
(``itemset_flags_gpu``) and the device-resident deep trie (``GpuMiner.deep_trie_flags``), against
the transaction-based oracle of tests/closed_oracle.py and the CPU twin.  Supports are integers,
so every comparison is exact equality."""
import threading

import numpy as np
import pytest

from kubernetes_machine_learning_server_amd.data.synthetic import generate
from kubernetes_machine_learning_server_amd.models import fpgrowth as fp
from tests import closed_oracle as co

pytestmark = pytest.mark.gpu


def _arrays(trie):
    return (np.ascontiguousarray(trie.parent, np.int64), np.ascontiguousarray(trie.item, np.int32),
            np.ascontiguousarray(trie.count, np.uint32), np.ascontiguousarray(trie.depth, np.uint8))


def _counts(f):
    return int(((f & co.CLOSED) != 0).sum()), int(((f & co.MAXIMAL) != 0).sum())


def test_uploaded_trie_matches_oracle_and_cpu(gpu_mod):
    _, _, trie, want = co.tiny_case(0.02, 2)
    got = gpu_mod.itemset_flags_gpu(*_arrays(trie))["flags"]
    assert got.dtype == np.uint8 and (got == want).all()
    assert (got == gpu_mod.itemset_flags(*_arrays(trie))).all()
    assert _counts(got) == (6405, 3271)
    t2 = fp.ItemsetTrie(trie.parent, trie.item, trie.count, trie.depth, trie.n_tx, 0.02)
    assert (t2.flags(backend="gpu") == want).all()


def test_clique_depth_16_all_ties(gpu_mod):
    ptr, items = co.clique_csr(16, 40)
    trie = fp.mine_csr(ptr, items, 16, 0.3, backend="cpu")
    assert len(trie) == 65535 and int(trie.depth.max()) == 16
    got = gpu_mod.itemset_flags_gpu(*_arrays(trie))["flags"]
    assert _counts(got) == (17, 1)
    closed, maximal = (got & co.CLOSED) != 0, (got & co.MAXIMAL) != 0
    assert (closed == ((trie.depth == 1) | (trie.depth == 16))).all()
    assert (maximal == (trie.depth == 16)).all()


def test_no_reliance_on_sibling_order(gpu_mod):
    _, _, trie, want = co.tiny_case(0.02, 2)
    parent, item, count, depth = _arrays(trie)
    # sizes in ascending order, a random order inside each size: parents stay first
    rng = np.random.default_rng(7)
    n = len(item)
    order = np.concatenate([rng.permutation(np.flatnonzero(depth == k))
                            for k in range(1, int(depth.max()) + 1)])  # new position -> old id
    new_of = np.empty(n, dtype=np.int64)
    new_of[order] = np.arange(n)
    p2 = parent[order]
    p2 = np.where(p2 >= 0, new_of[np.maximum(p2, 0)], -1)
    got = gpu_mod.itemset_flags_gpu(p2, item[order], count[order], depth[order])["flags"]
    assert (got == want[order]).all()


def test_device_resident_deep_trie(gpu_mod):
    tx = generate("ds1", seed=0)
    g = gpu_mod.GpuMiner(0)
    g.load_csr(tx.tx_ptr, tx.items, tx.n_items)
    d = g.mine_deep(0.05, emit=True)
    t = g.deep_arena_trie(1, 0)
    got = g.deep_trie_flags()["flags"]
    assert int(t["n"]) == int(d["n_itemsets"]) == 77905 == len(got)
    assert int(t["depth"].max()) == 10
    trie = fp.ItemsetTrie(t["parent"], t["item"], t["count"], t["depth"], tx.n_tx, 0.05)
    assert (got == gpu_mod.itemset_flags(*_arrays(trie))).all()
    assert _counts(got) == (47684, 11483)
    g.deep_arena_trie(3, 0)  # a rank's share: not closed under subsets
    with pytest.raises(RuntimeError, match="partial export"):
        g.deep_trie_flags()


def test_wide_item_ids(gpu_mod):
    tx = generate("tiny", seed=2)
    g = gpu_mod.GpuMiner(0)
    g.load_csr(tx.tx_ptr, (tx.items.astype(np.int64) * 700).astype(np.int32), 70_000)
    g.mine_deep(0.02, emit=True)
    t = g.deep_arena_trie(1, 0)
    assert t["item"].dtype == np.int32 and int(t["item"].max()) > 65535
    got = g.deep_trie_flags()["flags"]
    trie = fp.ItemsetTrie(t["parent"], t["item"], t["count"], t["depth"], tx.n_tx, 0.02)
    assert (got == gpu_mod.itemset_flags(*_arrays(trie))).all()
    assert len(got) == 6518 and _counts(got) == (6405, 3271)


def test_max_len_through_mine_csr(gpu_mod):
    tx, X, _, _ = co.tiny_case(0.02, 2)
    trie = fp.mine_csr(tx.tx_ptr, tx.items, tx.n_items, 0.02, max_len=3, backend="gpu", flags=True)
    assert trie.stats.get("miner") == "deep" and "flags_ms" in trie.stats
    assert trie._flags is not None and int(trie.depth.max()) == 3
    want = co.oracle_flags(X, co.trie_sets(trie), 0.02, max_len=3)
    assert (trie.flags() == want).all()


def test_missing_interior_node_raises(gpu_mod):
    _, _, trie, _ = co.tiny_case(0.02, 2)
    cut = co.drop_node(_arrays(trie), co.childless_pair_with_supersets(trie))
    box = {}

    def call():
        try:
            gpu_mod.itemset_flags_gpu(*cut)
            box["r"] = "returned"
        except Exception as e:  # noqa: BLE001
            box["r"] = e

    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(timeout=120)
    assert not th.is_alive(), "itemset_flags_gpu did not return"
    assert isinstance(box["r"], RuntimeError) and "missing from the trie" in str(box["r"])
