"""Transaction-based reference for the generator flag, the closure ids and the min-max rule basis
(tests/test_rule_basis.py, tests/test_gpu_basis.py).  Like tests/closed_oracle.py it knows nothing
about tries: with the one-hot matrix X,

* S is a generator iff dropping any one item strictly raises the support (a singleton always is:
  the empty set is no itemset);
* closure(S) is the set of columns that are all-ones over the rows containing S;
* the basis is enumerated by brute force: every closed itemset c, every non-empty proper subset g
  of c that is a generator, rule g -> c \\ g with confidence supp(c) / supp(g).

Supports are integers and confidence is one count ratio, so every comparison is exact."""
import functools

import numpy as np

from kubernetes_machine_learning_server_amd.models.fpgrowth import mine_csr
from tests import closed_oracle as co

GENERATOR = 4


class Supports:
    """Support counts straight from X, memoised by itemset."""

    def __init__(self, X):
        self.X = X
        self.memo = {}

    def __call__(self, s):
        s = frozenset(s)
        c = self.memo.get(s)
        if c is None:
            c = int(self.X[:, sorted(s)].all(axis=1).sum())
            self.memo[s] = c
        return c


def is_generator(sup, s):
    s = frozenset(s)
    if len(s) == 1:
        return True
    c = sup(s)
    return all(sup(s - {i}) > c for i in s)


def closure_of(X, s):
    rows = X[:, sorted(s)].all(axis=1)
    return frozenset(int(i) for i in np.flatnonzero(X[rows].all(axis=0)))


def oracle_generators(X, itemsets):
    sup = Supports(X)
    return np.array([is_generator(sup, s) for s in itemsets], dtype=bool)


def oracle_closures(X, itemsets):
    return [closure_of(X, s) for s in itemsets]


def oracle_basis(X, itemsets, min_conf=0.0):
    """[(antecedent, itemset, confidence)] of the min-max basis among ``itemsets`` with confidence
    >= min_conf, ordered as the engines order them: itemset position, then subset mask over the
    itemset's items in the order given."""
    sup = Supports(X)
    out = []
    for s in itemsets:
        s = list(s)
        if len(s) < 2 or closure_of(X, s) != frozenset(s):
            continue
        cs = sup(s)
        for m in range(1, (1 << len(s)) - 1):
            g = frozenset(s[i] for i in range(len(s)) if (m >> i) & 1)
            if not is_generator(sup, g):
                continue
            conf = cs / sup(g)
            if conf >= min_conf:
                out.append((g, frozenset(s), conf))
    return out


def rule_triples(rules, sets):
    """A Rules object as [(antecedent, itemset, confidence)] in its own order."""
    fs = [frozenset(s) for s in sets]
    return [(fs[a], fs[s], float(c))
            for s, a, c in zip(rules.itemset, rules.antecedent, rules.confidence)]


def tie_rich_csr(tx):
    """The transactions of ``tx`` plus item 100 wherever the most frequent item occurs and item 101
    wherever the 2nd and 3rd most frequent both occur (frequency order: stable sort of descending
    counts): many equal-support supersets."""
    assert tx.n_items == 100
    X = np.zeros((tx.n_tx, 102), dtype=bool)
    X[:, :100] = co.one_hot(tx.tx_ptr, tx.items, tx.n_items)
    order = np.argsort(-X[:, :100].sum(axis=0), kind="stable")
    X[:, 100] = X[:, order[0]]
    X[:, 101] = X[:, order[1]] & X[:, order[2]]
    rows, cols = np.nonzero(X)
    ptr = np.zeros(tx.n_tx + 1, dtype=np.int64)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr), cols.astype(np.int32), X


class Case:
    """A mined trie with everything the oracle says about it; computed once, read-only."""

    def __init__(self, X, trie, min_support):
        self.X, self.trie, self.min_support = X, trie, min_support
        self.sets = co.trie_sets(trie)
        ids = {frozenset(s): n for n, s in enumerate(self.sets)}
        gen = oracle_generators(X, self.sets)
        self.flags = co.oracle_flags(X, self.sets, min_support) | (gen * GENERATOR).astype(np.uint8)
        self.closure = np.array([ids[c] for c in oracle_closures(X, self.sets)], dtype=np.int64)
        self.basis = oracle_basis(X, self.sets)
        for a in (self.flags, self.closure):
            a.setflags(write=False)

    def basis_at(self, min_conf):
        return [r for r in self.basis if r[2] >= min_conf]


def arrays(trie):
    return (np.ascontiguousarray(trie.parent, np.int64), np.ascontiguousarray(trie.item, np.int32),
            np.ascontiguousarray(trie.count, np.uint32), np.ascontiguousarray(trie.depth, np.uint8))


@functools.lru_cache(maxsize=None)
def tiny():
    tx, X, trie, _ = co.tiny_case(0.02, 2)
    return Case(X, trie, 0.02)


@functools.lru_cache(maxsize=None)
def tie_rich():
    tx = co.tiny_case(0.02, 2)[0]
    ptr, items, X = tie_rich_csr(tx)
    trie = mine_csr(ptr, items, 102, 0.02, backend="cpu")
    return Case(X, trie, 0.02)
