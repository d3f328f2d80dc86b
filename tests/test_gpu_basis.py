"""Generator flags, closure ids and the min-max rule basis on the GPU: ``itemset_condense_gpu`` and
``GpuMiner.deep_trie_flags(generators, closure)`` (csrc/kernels/closed.hip) and
``association_rules_gpu`` with and without ``basis`` (csrc/kernels/rules.hip), against the
transaction-based oracle of tests/basis_oracle.py and the CPU twins.  Ids, flag bytes and
confidence (one count ratio) compare with exact equality; lift (two correctly rounded operations)
with rtol 1e-12.  The rule tests threshold on confidence only."""
import threading

import numpy as np
import pytest

from kubernetes_machine_learning_server_amd.data.synthetic import generate
from kubernetes_machine_learning_server_amd.models import fpgrowth as fp
from kubernetes_machine_learning_server_amd.models.rules import rules_from_trie
from tests import basis_oracle as bo
from tests import closed_oracle as co

pytestmark = pytest.mark.gpu

CASES = {"tiny": bo.tiny, "tie_rich": bo.tie_rich}


def _same_rules(a, b):
    assert len(a) == len(b)
    for k in ("itemset", "antecedent", "consequent", "confidence"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    np.testing.assert_allclose(a.lift, b.lift, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_uploaded_trie_matches_oracle_and_cpu(gpu_mod, name):
    case = CASES[name]()
    got = gpu_mod.itemset_condense_gpu(*bo.arrays(case.trie))
    cpu = gpu_mod.itemset_condense(*bo.arrays(case.trie))
    assert got["flags"].dtype == np.uint8 and got["closure"].dtype == np.int32
    assert (got["flags"] == case.flags).all() and (got["closure"] == case.closure).all()
    assert got["flags"].tobytes() == cpu["flags"].tobytes()
    assert got["closure"].tobytes() == cpu["closure"].tobytes()
    assert got["kernel_ms"] > 0
    t = case.trie
    t2 = fp.ItemsetTrie(t.parent, t.item, t.count, t.depth, t.n_tx, 0.02)
    assert (t2.flags(backend="gpu", generators=True) == case.flags).all()
    assert (t2.closure(backend="gpu") == case.closure).all()
    assert (t2.flags(backend="gpu") == (case.flags & 3)).all()


def test_no_reliance_on_sibling_order(gpu_mod):
    case = bo.tie_rich()
    parent, item, count, depth = bo.arrays(case.trie)
    # sizes in ascending order, a random order inside each size: parents stay first
    rng = np.random.default_rng(7)
    n = len(item)
    order = np.concatenate([rng.permutation(np.flatnonzero(depth == k))
                            for k in range(1, int(depth.max()) + 1)])  # new position -> old id
    new_of = np.empty(n, dtype=np.int64)
    new_of[order] = np.arange(n)
    p2 = parent[order]
    p2 = np.where(p2 >= 0, new_of[np.maximum(p2, 0)], -1)
    got = gpu_mod.itemset_condense_gpu(p2, item[order], count[order], depth[order])
    assert (got["flags"] == case.flags[order]).all()
    # the closure is one itemset whatever the numbering: its new id
    assert (got["closure"] == new_of[case.closure[order]]).all()
    # and the rule kernel's sibling shortcut sees scattered siblings and skipped itemsets
    t2 = fp.ItemsetTrie(p2, item[order], count[order], depth[order], case.trie.n_tx, 0.02)
    _same_rules(rules_from_trie(t2, "confidence", 0.0, backend="gpu", basis="minmax"),
                rules_from_trie(t2, "confidence", 0.0, backend="cpu", basis="minmax"))


@pytest.fixture(scope="module")
def clique16():
    ptr, items = co.clique_csr(16, 40)
    trie = fp.mine_csr(ptr, items, 16, 0.3, backend="cpu")
    assert len(trie) == 65535 and int(trie.depth.max()) == 16
    return trie, rules_from_trie(trie, "confidence", 0.0, backend="cpu", basis="minmax")


@pytest.mark.parametrize("scratch_bits", [None, "12"])
def test_clique_16_basis_rules(gpu_mod, clique16, monkeypatch, scratch_bits):
    # k = 16: the per-wave global subset table; with 12 scratch bits, the walk
    trie, want = clique16
    if scratch_bits is not None:
        monkeypatch.setenv("KMLS_RULES_SCRATCH_BITS", scratch_bits)
    got = rules_from_trie(trie, "confidence", 0.0, backend="gpu", basis="minmax")
    assert len(got) == 136
    _same_rules(got, want)
    top = int(np.flatnonzero(trie.depth == 16)[0])
    assert (got.itemset == top).all()
    assert (np.sort(got.antecedent) == np.flatnonzero(trie.depth <= 2)).all()


def test_clique_16_flags_and_closure(gpu_mod, clique16):
    trie, _ = clique16
    got = gpu_mod.itemset_condense_gpu(*bo.arrays(trie))
    assert (((got["flags"] & bo.GENERATOR) != 0) == (trie.depth <= 2)).all()
    top = int(np.flatnonzero(trie.depth == 16)[0])
    assert (got["closure"][trie.depth >= 2] == top).all()
    assert (got["closure"][trie.depth == 1] == np.flatnonzero(trie.depth == 1)).all()


@pytest.mark.parametrize("thr", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(CASES))
def test_basis_rules_match_cpu_and_oracle(gpu_mod, name, thr):
    case = CASES[name]()
    got = rules_from_trie(case.trie, "confidence", thr, backend="gpu", basis="minmax")
    _same_rules(got, rules_from_trie(case.trie, "confidence", thr, backend="cpu", basis="minmax"))
    assert bo.rule_triples(got, case.sets) == case.basis_at(thr)


def test_all_rules_match_cpu(gpu_mod):
    trie = bo.tiny().trie
    got = rules_from_trie(trie, "confidence", 0.5, backend="gpu", basis="all")
    want = rules_from_trie(trie, "confidence", 0.5, backend="cpu")
    assert len(got) > len(bo.tiny().basis_at(0.5))
    _same_rules(got, want)
    _same_rules(rules_from_trie(trie, "confidence", 0.5, backend="gpu"), want)


def _wide(trie_dict, n_tx, ms):
    return fp.ItemsetTrie(trie_dict["parent"], trie_dict["item"], trie_dict["count"],
                          trie_dict["depth"], n_tx, ms)


def test_device_resident_deep_trie(gpu_mod):
    tx = generate("ds1", seed=0)
    g = gpu_mod.GpuMiner(0)
    g.load_csr(tx.tx_ptr, tx.items, tx.n_items)
    d = g.mine_deep(0.05, emit=True)
    t = g.deep_arena_trie(1, 0)
    plain = g.deep_trie_flags()
    got = g.deep_trie_flags(generators=True, closure=True)
    assert int(t["n"]) == int(d["n_itemsets"]) == 77905 == len(got["flags"])
    assert set(plain) == {"flags", "kernel_ms"} and plain["flags"].max() <= 3
    f = plain["flags"]
    assert (int(((f & co.CLOSED) != 0).sum()), int(((f & co.MAXIMAL) != 0).sum())) == (47684, 11483)
    want = gpu_mod.itemset_condense(*bo.arrays(_wide(t, tx.n_tx, 0.05)))
    assert got["flags"].tobytes() == want["flags"].tobytes()
    assert got["closure"].dtype == np.int32
    assert got["closure"].tobytes() == want["closure"].tobytes()
    assert ((got["flags"] & 3) == f).all()
    only_gen = g.deep_trie_flags(generators=True)
    assert "closure" not in only_gen and (only_gen["flags"] == got["flags"]).all()
    g.deep_arena_trie(3, 0)  # a rank's share: not closed under subsets
    with pytest.raises(RuntimeError, match="partial export"):
        g.deep_trie_flags(generators=True, closure=True)


def test_wide_item_ids(gpu_mod):
    tx = generate("tiny", seed=2)
    g = gpu_mod.GpuMiner(0)
    g.load_csr(tx.tx_ptr, (tx.items.astype(np.int64) * 700).astype(np.int32), 70_000)
    g.mine_deep(0.02, emit=True)
    t = g.deep_arena_trie(1, 0)
    assert t["item"].dtype == np.int32 and int(t["item"].max()) > 65535
    got = g.deep_trie_flags(generators=True, closure=True)
    want = gpu_mod.itemset_condense(*bo.arrays(_wide(t, tx.n_tx, 0.02)))
    assert got["flags"].tobytes() == want["flags"].tobytes()
    assert got["closure"].tobytes() == want["closure"].tobytes()
    assert len(got["flags"]) == 6518
    assert int(((got["flags"] & bo.GENERATOR) != 0).sum()) == 6405


def test_missing_interior_node_raises(gpu_mod):
    trie = bo.tiny().trie
    cut = co.drop_node(bo.arrays(trie), co.childless_pair_with_supersets(trie))
    box = {}

    def call():
        for name, fn in (("condense", lambda: gpu_mod.itemset_condense_gpu(*cut)),
                         ("rules", lambda: gpu_mod.association_rules_gpu(
                             *cut, trie.n_tx, 0, 0.0, 0, 0, 1))):
            try:
                fn()
                box[name] = "returned"
            except Exception as e:  # noqa: BLE001
                box[name] = e

    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(timeout=120)
    assert not th.is_alive(), "the GPU call did not return"
    for name in ("condense", "rules"):
        assert isinstance(box[name], RuntimeError) and "missing from the trie" in str(box[name])
