"""Closed / maximal itemsets on the CPU: the C++ twin (csrc/host/closed_cpu.cpp) behind
``ItemsetTrie.flags``, ``fpmax`` / ``fpclose`` and the job's ITEMSET_FLAGS option, against the
transaction-based oracle of tests/closed_oracle.py (exact equality: supports are integers)."""
import numpy as np
import pytest

from kubernetes_machine_learning_server_amd.job import main as job
from kubernetes_machine_learning_server_amd.config import JobSettings
from kubernetes_machine_learning_server_amd.models import fpgrowth as fp
from kubernetes_machine_learning_server_amd.ops import native
from tests import closed_oracle as co
from tests.helpers import job_settings, make_datasets


def _arrays(trie):
    return (np.ascontiguousarray(trie.parent, np.int64), np.ascontiguousarray(trie.item, np.int32),
            np.ascontiguousarray(trie.count, np.uint32), np.ascontiguousarray(trie.depth, np.uint8))


def test_cpu_flags_match_oracle_tiny():
    _, _, trie, want = co.tiny_case(0.02, 2)
    got = native.load().itemset_flags(*_arrays(trie))
    assert got.dtype == np.uint8 and (got == want).all()
    assert len(trie) == 6518 and int(trie.depth.max()) == 5
    assert int((got & co.CLOSED).astype(bool).sum()) == 6405
    assert int((got & co.MAXIMAL).astype(bool).sum()) == 3271
    t2 = fp.ItemsetTrie(trie.parent, trie.item, trie.count, trie.depth, trie.n_tx, 0.02)
    assert (t2.flags(backend="cpu") == want).all() and t2.flags() is t2.flags()
    assert (t2.closed_mask() == ((want & co.CLOSED) != 0)).all()
    assert (t2.maximal_mask() == ((want & co.MAXIMAL) != 0)).all()


def test_fpmax_fpclose_dataframes():
    tx, X, trie, want = co.tiny_case(0.03, 2)
    sets = co.trie_sets(trie)
    sup = {frozenset(s): c / tx.n_tx for c, s in trie.itemsets()}
    assert len(sets) == 1788
    mx = fp.fpmax(X, 0.03, backend="cpu")
    cl = fp.fpclose(X, 0.03, backend="cpu")
    assert list(mx.columns) == ["support", "itemsets"] == list(cl.columns)
    want_max = {frozenset(s) for s, f in zip(sets, want) if f & co.MAXIMAL}
    want_cl = {frozenset(s) for s, f in zip(sets, want) if f & co.CLOSED}
    assert len(want_cl) == 1785 and len(want_max) == 1048
    assert len(mx) == len(want_max) and set(mx["itemsets"]) == want_max
    assert len(cl) == len(want_cl) and set(cl["itemsets"]) == want_cl
    for df in (mx, cl):
        assert all(sup[s] == v for v, s in zip(df["support"], df["itemsets"]))
    assert set(mx["itemsets"]) <= set(cl["itemsets"])
    # without a mask, to_dataframe / to_records are what they were
    full = trie.to_dataframe(use_colnames=False)
    recs = trie.to_records(use_colnames=False)
    assert len(full) == len(trie) == len(recs)
    assert [(v, s) for v, s in zip(full["support"], full["itemsets"])] == recs
    assert recs == [(c / trie.n_tx, frozenset(s)) for c, s in trie.itemsets()]
    assert trie.to_records(False, mask=np.ones(len(trie), bool)) == recs
    with pytest.raises(ValueError):
        trie.to_records(False, mask=np.ones(3, bool))


def test_clique_all_ties():
    ptr, items = co.clique_csr(16, 40)
    trie = fp.mine_csr(ptr, items, 16, 0.3, backend="cpu")
    assert len(trie) == 65535
    f = trie.flags(backend="cpu")
    closed, maximal = (f & co.CLOSED) != 0, (f & co.MAXIMAL) != 0
    assert int(closed.sum()) == 17 and int(maximal.sum()) == 1
    assert (closed == ((trie.depth == 1) | (trie.depth == 16))).all()
    assert (maximal == (trie.depth == 16)).all()
    assert (trie.count[trie.depth == 1] == 41).all() and (trie.count[trie.depth > 1] == 40).all()


def test_max_len_flags_are_relative_to_the_trie():
    tx, X, _, _ = co.tiny_case(0.02, 2)
    trie = fp.mine_csr(tx.tx_ptr, tx.items, tx.n_items, 0.02, max_len=3, backend="cpu", flags=True)
    assert int(trie.depth.max()) == 3 and trie._flags is not None
    want = co.oracle_flags(X, co.trie_sets(trie), 0.02, max_len=3)
    assert (trie.flags() == want).all()
    assert (trie.flags()[trie.depth == 3] == (co.CLOSED | co.MAXIMAL)).all()


def test_missing_subset_raises():
    _, _, trie, _ = co.tiny_case(0.02, 2)
    gone = co.childless_pair_with_supersets(trie)
    cut = co.drop_node(_arrays(trie), gone)
    with pytest.raises(RuntimeError, match="missing from the trie"):
        native.load().itemset_flags(*cut)
    # a child that precedes its parent is refused before any walk
    p = cut[0].copy()
    p[0] = 5
    with pytest.raises(RuntimeError, match="malformed trie"):
        native.load().itemset_flags(p, *cut[1:])


def test_job_itemset_flags_option(tmp_path, monkeypatch):
    keys = {"parent", "item", "count", "depth", "n_tx", "min_support"}
    make_datasets(tmp_path)
    assert JobSettings.from_env(dotenv=False).itemset_flags is False
    cfg = job_settings(tmp_path)
    job.run(cfg)
    with np.load(cfg.pickles_folder / job.ITEMSETS_FILE) as z:
        assert set(z.files) == keys
        plain = {k: z[k] for k in z.files}
    monkeypatch.setenv("ITEMSET_FLAGS", "1")
    on = JobSettings.from_env(dotenv=False).itemset_flags
    assert on is True
    root2 = tmp_path / "second"
    make_datasets(root2)
    cfg2 = job_settings(root2, itemset_flags=on)
    job.run(cfg2)
    with np.load(cfg2.pickles_folder / job.ITEMSETS_FILE) as z:
        assert set(z.files) == keys | {"flags"}
        got = {k: z[k] for k in z.files}
    for k in keys:
        assert (got[k] == plain[k]).all()
    trie = fp.ItemsetTrie(got["parent"], got["item"], got["count"], got["depth"],
                          int(got["n_tx"]), float(got["min_support"]))
    assert got["flags"].dtype == np.uint8 and (got["flags"] == trie.flags(backend="cpu")).all()
    assert 0 < int((got["flags"] & co.MAXIMAL).astype(bool).sum()) < len(trie)
