"""Transaction-based reference for the closed / maximal itemset flags (tests/test_closed.py,
tests/test_gpu_closed.py).  It knows nothing about tries: with the one-hot matrix X, an itemset S
is closed iff the AND of the rows containing S has no set column outside S, and maximal iff no
item outside S keeps the support at or above the miner's count threshold for itemsets of two or
more items, ceil(min_support * n_tx).  Supports are integers: every comparison is exact."""
import functools
import math

import numpy as np

from kubernetes_machine_learning_server_amd.data.synthetic import generate
from kubernetes_machine_learning_server_amd.models.fpgrowth import mine_csr

CLOSED, MAXIMAL = 1, 2


def one_hot(tx_ptr, items, n_items):
    X = np.zeros((len(tx_ptr) - 1, n_items), dtype=bool)
    for t in range(len(tx_ptr) - 1):
        X[t, items[tx_ptr[t]:tx_ptr[t + 1]]] = True
    return X


def oracle_flags(X, itemsets, min_support, max_len=None):
    """Flag byte per itemset (iterables of column ids).  ``max_len``: flags relative to the
    itemsets of at most that many items (one of the cap size has no superset to lose to)."""
    minc = math.ceil(min_support * X.shape[0])
    out = np.zeros(len(itemsets), dtype=np.uint8)
    for n, s in enumerate(itemsets):
        s = list(s)
        if max_len and len(s) >= max_len:
            out[n] = CLOSED | MAXIMAL
            continue
        rows = X[:, s].all(axis=1)
        cnt = X[rows].sum(axis=0)
        cnt[s] = 0
        closed = not (cnt == rows.sum()).any()
        maximal = not (cnt >= minc).any()
        out[n] = (CLOSED if closed else 0) | (MAXIMAL if maximal else 0)
    return out


def trie_sets(trie):
    return [s for _, s in trie.itemsets()]


@functools.lru_cache(maxsize=None)
def tiny_case(min_support=0.02, seed=2):
    """(tx, X, CPU-mined trie, oracle flags) of the `tiny` shape; computed once, read-only."""
    tx = generate("tiny", seed=seed)
    X = one_hot(tx.tx_ptr, tx.items, tx.n_items)
    trie = mine_csr(tx.tx_ptr, tx.items, tx.n_items, min_support, backend="cpu")
    want = oracle_flags(X, trie_sets(trie), min_support)
    want.setflags(write=False)
    return tx, X, trie, want


def clique_csr(n_items=16, n_full=40):
    """n_full transactions holding every item, then one transaction per item alone."""
    rows = [list(range(n_items))] * n_full + [[i] for i in range(n_items)]
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, np.int32) for r in rows])
    return ptr, items


def drop_node(trie_arrays, gone):
    """The trie without node `gone` (which must have no children): ids above it shift down."""
    parent, item, count, depth = trie_arrays
    assert not (parent == gone).any()
    keep = np.arange(len(item)) != gone
    p = parent[keep].astype(np.int64)
    p[p > gone] -= 1
    return p, item[keep], count[keep], depth[keep]


def childless_pair_with_supersets(trie):
    """A 2-itemset with no children in the trie whose supersets are in it."""
    sets = trie_sets(trie)
    has_child = np.zeros(len(sets), dtype=bool)
    has_child[trie.parent[trie.parent >= 0]] = True
    bigger = [frozenset(s) for s in sets if len(s) == 3]
    for n, s in enumerate(sets):
        if len(s) == 2 and not has_child[n] and any(frozenset(s) < b for b in bigger):
            return n
    raise AssertionError("no childless pair with supersets in this trie")
