"""Generator flags, closure ids and the min-max rule basis on the CPU: ``itemset_condense`` and
``association_rules(basis=1)`` (csrc/host/closed_cpu.cpp, rules_cpu.cpp) behind
``ItemsetTrie.flags(generators=True)`` / ``generator_mask`` / ``closure`` and
``rules_from_trie(basis="minmax")``, against the transaction-based oracle of tests/basis_oracle.py.
Supports are integers and confidence is one count ratio: every comparison is exact equality."""
import numpy as np
import pytest

from kubernetes_machine_learning_server_amd.models import fpgrowth as fp
from kubernetes_machine_learning_server_amd.models.rules import association_rules, rules_from_trie
from kubernetes_machine_learning_server_amd.ops import native
from tests import basis_oracle as bo
from tests import closed_oracle as co


def _check_against_oracle(case, n_sets, n_gen, n_basis, n_exact):
    trie = case.trie
    got = native.load().itemset_condense(*bo.arrays(trie))
    assert got["flags"].dtype == np.uint8 and (got["flags"] == case.flags).all()
    assert (got["closure"] == case.closure).all()
    assert ((got["closure"] == np.arange(len(trie))) == ((case.flags & co.CLOSED) != 0)).all()
    assert len(trie) == n_sets
    assert int(((got["flags"] & bo.GENERATOR) != 0).sum()) == n_gen
    t2 = fp.ItemsetTrie(trie.parent, trie.item, trie.count, trie.depth, trie.n_tx, 0.02)
    assert (t2.flags(backend="cpu", generators=True) == case.flags).all()
    assert (t2.generator_mask("cpu") == ((case.flags & bo.GENERATOR) != 0)).all()
    assert (t2.closure("cpu") == case.closure).all()
    r = rules_from_trie(trie, "confidence", 0.0, backend="cpu", basis="minmax")
    assert bo.rule_triples(r, case.sets) == case.basis
    assert len(r) == n_basis and int((r.confidence == 1.0).sum()) == n_exact
    # consequent = itemset minus antecedent, lift = conf * T / count(consequent)
    for s, a, c in list(zip(r.itemset, r.antecedent, r.consequent))[::97]:
        assert set(case.sets[c]) == set(case.sets[s]) - set(case.sets[a])
    assert np.array_equal(r.lift, r.confidence * trie.n_tx / trie.count[r.consequent])
    half = rules_from_trie(trie, "confidence", 0.5, backend="cpu", basis="minmax")
    assert bo.rule_triples(half, case.sets) == case.basis_at(0.5)
    return r


def test_tiny_flags_closure_basis_match_oracle():
    case = bo.tiny()
    _check_against_oracle(case, 6518, 6405, 47051, 113)
    assert int(((case.flags & co.CLOSED) != 0).sum()) == 6405


def test_tie_rich_flags_closure_basis_match_oracle():
    _check_against_oracle(bo.tie_rich(), 11692, 8369, 60285, 3843)


def test_clique_generators_closure_and_basis():
    ptr, items = co.clique_csr(16, 40)
    trie = fp.mine_csr(ptr, items, 16, 0.3, backend="cpu")
    assert len(trie) == 65535
    gen = trie.generator_mask("cpu")
    assert (gen == (trie.depth <= 2)).all() and int(gen.sum()) == 16 + 120
    top = int(np.flatnonzero(trie.depth == 16)[0])
    clo = trie.closure("cpu")
    assert (clo[trie.depth >= 2] == top).all()
    assert (clo[trie.depth == 1] == np.flatnonzero(trie.depth == 1)).all()
    r = rules_from_trie(trie, "confidence", 0.0, backend="cpu", basis="minmax")
    assert len(r) == 136 and (r.itemset == top).all()
    assert (np.sort(r.antecedent) == np.flatnonzero(trie.depth <= 2)).all()
    exact = rules_from_trie(trie, "confidence", 1.0, backend="cpu", basis="minmax")
    assert len(exact) == 120 and (trie.depth[exact.antecedent] == 2).all()
    assert (exact.confidence == 1.0).all()


def test_basis_is_lossless_on_the_tie_rich_case():
    case = bo.tie_rich()
    trie = case.trie
    clo = case.closure
    full = rules_from_trie(trie, "confidence", 0.0, backend="cpu", basis="all")
    basis = rules_from_trie(trie, "confidence", 0.0, backend="cpu", basis="minmax")
    assert len(full) == 150856
    have = {}
    for s, a, c in zip(basis.itemset, basis.antecedent, basis.confidence):
        have.setdefault((int(clo[a]), int(s)), set()).add(float(c))
    ca, cs = clo[full.antecedent], clo[full.itemset]
    same = ca == cs
    assert (full.confidence[same] == 1.0).all()
    for a, s, c in zip(ca[~same], cs[~same], full.confidence[~same]):
        assert float(c) in have.get((int(a), int(s)), ()), (a, s, c)


def test_max_len_generators_and_relative_closure():
    tx, X, _, _ = co.tiny_case(0.02, 2)
    trie = fp.mine_csr(tx.tx_ptr, tx.items, tx.n_items, 0.02, max_len=3, backend="cpu")
    sets = co.trie_sets(trie)
    assert int(trie.depth.max()) == 3
    assert (trie.generator_mask("cpu") == bo.oracle_generators(X, sets)).all()
    clo = trie.closure("cpu")
    closed = trie.closed_mask("cpu")
    assert closed[clo].all() and (trie.count[clo] == trie.count).all()
    assert all(set(sets[v]) <= set(sets[c]) for v, c in enumerate(clo))
    assert ((clo == np.arange(len(trie))) == closed).all()


def test_missing_interior_node_raises():
    trie = bo.tiny().trie
    cut = co.drop_node(bo.arrays(trie), co.childless_pair_with_supersets(trie))
    with pytest.raises(RuntimeError, match="missing from the trie"):
        native.load().itemset_condense(*cut)
    with pytest.raises(RuntimeError, match="missing from the trie"):
        native.load().association_rules(*cut, trie.n_tx, 0, 0.0, 0, 0, 1)


def test_unknown_basis_raises():
    trie = bo.tiny().trie
    with pytest.raises(ValueError, match="basis"):
        rules_from_trie(trie, basis="nonsense")
    with pytest.raises(ValueError, match="basis"):
        association_rules(trie, basis="nonsense")


def test_default_flags_are_the_two_bit_bytes():
    case = bo.tiny()
    trie = case.trie
    t2 = fp.ItemsetTrie(trie.parent, trie.item, trie.count, trie.depth, trie.n_tx, 0.02)
    two = native.load().itemset_flags(*bo.arrays(trie))
    assert (two == (case.flags & 3)).all()
    assert t2.flags(generators=True, backend="cpu").max() >= bo.GENERATOR
    assert (t2.flags() == two).all() and t2.flags() is t2.flags()
    assert t2.flags(generators=True) is t2.flags(generators=True)
    # basis="all" is the engine as it was, and the DataFrame surface takes the argument
    a = rules_from_trie(trie, "confidence", 0.5, backend="cpu")
    b = rules_from_trie(trie, "confidence", 0.5, backend="cpu", basis="all")
    assert np.array_equal(a.itemset, b.itemset) and np.array_equal(a.antecedent, b.antecedent)
    df = association_rules(trie, min_threshold=0.5, basis="minmax")
    assert len(df) == len(case.basis_at(0.5))
