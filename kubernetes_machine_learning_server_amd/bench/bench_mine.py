"""Mining sections of ``bench.py`` (the headline itself lives in bench.py).

* ``run_deep``       — count-only full mining of one dataset, split over the ranks (the headline
                       and the config-2 family); verified by the itemset digest.
* ``run_levelwise``  — the round-2 headline form: ds1 @0.05 through the level-wise graph path
                       with the trie download and the device rule map in the step, verified
                       against the native CPU miner; at N > 1 one relabelled dataset per rank
                       (weak scaling, a secondary field of the bench line).
* ``run_config2``    — BASELINE config 2 (ds1 @0.01): the deployed rule map, mining truncated at
                       4 items, and full mining at 0.01 with the size cap raised until a time
                       budget is spent (per-level counts up to the cap).
* ``run_config3``    — BASELINE config 3 (10M x 1M @2e-4) transaction-DP over all ranks.

Reference timed region: ``machine-learning/main.py:264-308`` (encode + fpgrowth + rule map);
all sizes mined (``main.py:272``), support sweep downwards (``main.py:450-473``).
"""
from __future__ import annotations

import json
import os
import time
from typing import Callable, Dict, List, Optional

import numpy as np

# Whole-problem references computed on the build host by the native CPU miner
# (``mine_cpu_count``, 8 threads, 143 s) on ``generate("ds1", seed=0)``: (digest, n_itemsets,
# per-level counts from size 1).  The digest uses the round-3 digest_terms (kmls/digest.hpp).
CPU_REF = {
    0.02: ("1d15b1d026fe928d14a65f5b88be8656", 1414082373,
           [2032, 81637, 897824, 5004384, 18407680, 51371444, 114076602, 200624405, 274917544,
            289754387, 232392862, 139994181, 62090008, 19642215, 4215542, 566649, 41695, 1275,
            7]),
}
# config 3 support: 2e-4 leaves 14,773 frequent items of the 1M vocabulary (46,061 itemsets up
# to 6 items); at the round-2 setting (1e-3) only 756 items were frequent
C3_MIN_SUPPORT = 0.0002


def digest_of(N, r, min_depth=0):
    return N.trie_digest(r["parent"], r["item"], r["count"], r["depth"], min_depth)


def index_equal(ix, ref) -> bool:
    """Device rule map == CPU-built index (row_ptr, consequents, counts)."""
    rp = np.asarray(ix["row_ptr"], np.int64)
    if len(rp) != len(ref.row_ptr) or not np.array_equal(rp, ref.row_ptr):
        return False
    return (np.array_equal(np.asarray(ix["cons"], np.int32), ref.cons) and
            np.array_equal(np.asarray(ix["count"], np.int64),
                           np.rint(ref.score * ref._n_tx).astype(np.int64)))


def cpu_index(N, tx, ms, names, max_len=2):
    from ..serve.index import build_index_from_trie
    r = N.mine_cpu(tx.tx_ptr, tx.items, tx.n_items, ms, max_len)
    ref = build_index_from_trie(r["parent"], r["item"], r["count"], r["depth"], tx.n_tx,
                                tx.n_items, names)
    ref._n_tx = tx.n_tx
    return ref


# ---------------------------------------------------------------------------------------------
# count-only full mining (headline)
# ---------------------------------------------------------------------------------------------
class CpuCountMiner:
    """The CPU tier of the headline (``bench.py --cpu``, tests): the native CPU count miner on
    this rank's share of the level-3 tasks, combined like the GPU partials (gloo)."""

    comm_backend = "torch"

    def __init__(self, tx, rank: int, world: int, threads: int = 0):
        from ..ops import native
        self.N, self.tx, self.rank, self.world, self.threads = native.load(), tx, rank, world, \
            threads

    def mine(self, ms: float, max_len: int = 0) -> Dict:
        from ..parallel.deep import allreduce_partial
        t = self.tx
        d = dict(self.N.mine_cpu_count(t.tx_ptr, t.items, t.n_items, ms, max_len, 1 << 62,
                                       self.threads, self.rank, self.world))
        d.update(candidates=0, chunks=0, level2_tasks=0, round_tasks=[],
                 phases_ms={"total": d["seconds"] * 1e3})
        return allreduce_partial(d, self.world) if self.world > 1 else d

    def synchronize(self) -> None:
        pass


def run_deep(tx, ms: float, world: int, rank: int, device: int, warmup: int, steps: int,
             barrier_sync: Callable[[], None], max_over_ranks: Callable[[float], float],
             comm: Optional[str] = None, max_len: int = 0, cpu: bool = False, **opts) -> Dict:
    """Time `steps` whole-problem calls (every itemset of every size of `tx` at `ms`, split
    over the ranks, per-size counts + digest combined over RCCL) after `warmup` untimed ones."""
    if cpu:
        dm = CpuCountMiner(tx, rank, world)
    else:
        from ..parallel.deep import DeepMiner
        dm = DeepMiner(tx.tx_ptr, tx.items, tx.n_items, device=device, rank=rank, world=world,
                       comm_backend=comm, **opts)
    r = None
    for _ in range(warmup):
        r = dm.mine(ms, max_len)
    dm.synchronize()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = dm.mine(ms, max_len)
    dm.synchronize()
    barrier_sync()
    ms_step = max_over_ranks((time.perf_counter() - t0) * 1000.0 / max(1, steps))
    out = {"ms_per_step": round(ms_step, 3), "n_itemsets": int(r["n_itemsets"]),
           "per_level": [int(x) for x in r["per_level"][1:]], "digest": r["digest"],
           "max_depth": int(r["max_depth"]), "n_frequent_items": int(r["n_frequent_items"]),
           "candidates": int(r["candidates"]), "chunks": int(r["chunks"]),
           "level2_tasks": int(r["level2_tasks"]), "comm": dm.comm_backend,
           "rank0_phases_ms": {k: round(v, 3) for k, v in r["phases_ms"].items()},
           "rank0_rounds": len(r["round_tasks"])}
    ref = CPU_REF.get(ms) if not max_len else None
    out["verified_digest"] = (r["digest"] == ref[0] and int(r["n_itemsets"]) == ref[1]) \
        if ref else None
    out["_miner"] = dm
    out["_last"] = r
    return out


def run_deep_emit(dm, ms: float, world: int, rank: int, warmup: int, steps: int,
                  barrier_sync, max_over_ranks, gather) -> Dict:
    """The headline problem with every itemset MATERIALISED (``mine_deep(emit=True)``): each
    frequent itemset becomes a node (parent node, item, support, size) of a trie arena in HBM,
    written inside the timed step.  Verified after the timing: the arena's own content digest
    (set hashes rebuilt on the device from parent links), combined over the ranks, must equal
    the CPU miner's digest of the whole problem."""
    dm.opts["emit"] = True
    try:
        r = None
        for _ in range(max(1, warmup)):  # (the first call sizes the arena)
            r = dm.mine(ms)
        dm.synchronize()
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            r = dm.mine(ms)
        dm.synchronize()
        barrier_sync()
        ms_step = max_over_ranks((time.perf_counter() - t0) * 1000.0 / max(1, steps))
        t1 = time.perf_counter()
        dg = dm.g.deep_arena_digest(1 if rank == 0 else 3)
        verify_s = time.perf_counter() - t1
    finally:
        dm.opts["emit"] = False
    parts = gather((int(dg["sum"]), int(dg["xor"]), int(dg["n"]), int(r["arena_nodes"])))
    s = x = n = nodes = 0
    for ps, px, pn, pa in parts:
        s, x, n, nodes = (s + ps) % (1 << 64), x ^ px, n + pn, nodes + pa
    digest = f"{s:016x}{x:016x}"
    ref = CPU_REF.get(ms)
    return {"ms_per_step": round(ms_step, 3), "n_itemsets_in_arenas": n,
            "arena_node_ids_used": nodes,
            "arena_bytes": int(nodes) * 13,
            "node_format": "SoA: parent u32, item rank u32, support u32, size u8 (13 B)",
            "arena_digest": digest,
            "verified_digest": (digest == ref[0] and n == ref[1]) if ref else None,
            "digest_equals_count_only": digest == r["digest"],
            "verify_s_rank0": round(verify_s, 3),
            "rank0_phases_ms": {k: round(v, 3) for k, v in r["phases_ms"].items()}}


OFFLINE_SOURCE = ("scripts/full_count.py --world 256 on one MI355X (every virtual rank mined "
                  "exactly, partials combined; profiles/config2_full/)")


def offline_full_count() -> Optional[Dict]:
    """The complete config-2 count (ds1 @ 0.01, every size) measured by scripts/full_count.py."""
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "config2_full_count.json")
    if not os.path.exists(p):
        return None
    with open(p) as fh:
        return json.load(fh)


# BASELINE config 2 complete, on a pre-declared subset of the offline run's 256 virtual ranks:
# the ranks at the 0 / 25 / 50 / 75 / 90 % quantiles of the offline per-rank time (1.3-23 s
# each, ~57 s in all), fixed before any bench run, so light and heavy shares are both timed.
CONFIG2_SUBSET_RANKS = (38, 250, 156, 92, 192)
CONFIG2_WORLD = 256


def config2_partials() -> Optional[Dict[int, Dict]]:
    """Per-virtual-rank partials of the complete config-2 count (scripts/full_count.py --world
    256: per-size counts, digest, seconds), as committed under profiles/config2_full/."""
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data",
                     "config2_world256_partials.jsonl")
    if not os.path.exists(p):
        return None
    out = {}
    with open(p) as fh:
        for line in fh:
            if line.strip():
                d = json.loads(line)
                out[int(d["rank"])] = d
    return out if len(out) == CONFIG2_WORLD else None


def _trim(per) -> List[int]:
    per = [int(x) for x in per]
    while per and per[-1] == 0:
        per.pop()
    return per


def config2_complete_subset(g, ms: float = 0.01, ranks=CONFIG2_SUBSET_RANKS) -> Dict:
    """Complete full mining of BASELINE config 2 (ds1 @ 0.01, every size: 1.64e14 itemsets)
    timed by the bench on `ranks` of the 256 snake-dealt virtual ranks: each rank's share (its
    level-3 tasks' whole subtrees) is mined exactly (``mine_deep`` with that rank / world, no
    communicator) and its per-size counts and digest must equal the offline run's partial of
    the same rank.  Reports the itemsets/s of config 2 proper and the whole-problem time
    projected from the offline per-rank times scaled by this run's measured/offline ratio."""
    parts = config2_partials()
    if parts is None:
        return {"error": "config2_world256_partials.jsonl missing"}
    recs, n_tot, s_tot, off_tot = [], 0, 0.0, 0.0
    for r in ranks:
        t = time.perf_counter()
        # the deal the offline partials were counted under: level-3 tasks by class size
        d = g.mine_deep(ms, 0, int(r), CONFIG2_WORLD, None, deal_key=0)
        s = time.perf_counter() - t
        ref = parts[int(r)]
        ok = (d["digest"] == ref["digest"] and int(d["n_itemsets"]) == int(ref["n_itemsets"])
              and _trim(d["per_level"]) == _trim(ref["per_level"]))
        recs.append({"rank": int(r), "s": round(s, 3), "offline_s": ref["s"],
                     "n_itemsets": int(d["n_itemsets"]), "max_depth": int(d["max_depth"]),
                     "verified": bool(ok)})
        n_tot += int(d["n_itemsets"])
        s_tot += s
        off_tot += float(ref["s"])
    all_off = sum(float(p["s"]) for p in parts.values())
    off = offline_full_count() or {}
    proj = all_off * s_tot / off_tot if off_tot else None
    return {"what": "BASELINE config 2 complete (ds1 @0.01, every itemset of every size), "
                    "mined exactly on pre-declared virtual ranks of the 256-way snake deal",
            "world_virtual": CONFIG2_WORLD, "ranks": recs,
            "verified": all(x["verified"] for x in recs),
            "n_itemsets": n_tot, "s": round(s_tot, 3),
            "itemsets_per_s": round(n_tot / s_tot, 1) if s_tot else None,
            "share_of_problem": round(n_tot / int(off["n_itemsets"]), 5) if off else None,
            "measured_over_offline": round(s_tot / off_tot, 4) if off_tot else None,
            "projected_whole_problem_s_1gpu": round(proj, 1) if proj else None,
            "projected_itemsets_per_s_1gpu": (round(int(off["n_itemsets"]) / proj, 1)
                                              if proj and off else None),
            "whole_problem_n_itemsets": off.get("n_itemsets")}


def deep_capped(dm, ms: float, budget_s: float, start_len: int = 4, max_cap: int = 64) -> Dict:
    """Full mining at `ms` with the itemset size cap raised one at a time while a call stays
    under `budget_s` (the last completed cap's counts, timed)."""
    last, trail = None, []
    L = start_len
    while L <= max_cap:
        t = time.perf_counter()
        r = dm.mine(ms, L)
        dt = time.perf_counter() - t
        trail.append({"max_len": L, "s": round(dt, 3), "n_itemsets": int(r["n_itemsets"])})
        last = (L, dt, r)
        if int(r["max_depth"]) < L:  # the cap no longer binds: this is the complete result
            break
        if dt * 4 > budget_s:  # the next size is usually several times larger
            break
        L += 1
    L, dt, r = last
    return {"max_len": L, "complete": int(r["max_depth"]) < L, "s": round(dt, 3),
            "n_itemsets": int(r["n_itemsets"]), "itemsets_per_s": round(r["n_itemsets"] / dt, 1),
            "per_level": [int(x) for x in r["per_level"][1:]], "digest": r["digest"],
            "trail": trail}


# ---------------------------------------------------------------------------------------------
# level-wise path (round-2 headline form)
# ---------------------------------------------------------------------------------------------
def run_levelwise(N, tx, ms: float, world: int, rank: int, device: int, warmup: int,
                  steps: int, barrier_sync, max_over_ranks, gather, weak: bool,
                  verify: bool = True, prefetch: bool = True) -> Dict:
    """ds1 @`ms` through the level-wise path: supports → encode → gram → every level → trie
    download + device rule map, launch-ahead steady state.  weak: one dataset per rank (rank r
    mines a relabelled copy), job total = sum of itemsets ÷ slowest rank."""
    from ..data.synthetic import relabel
    from ..parallel.dist_miner import DistMiner
    from ..serve.index import name_tie_rank
    data = relabel(tx, rank) if weak else tx
    tie = name_tie_rank(data.names) if data.names else np.arange(data.n_items, dtype=np.int32)
    m = DistMiner(data.tx_ptr, data.items, data.n_items, ms, device=device,
                  mode="local" if weak else "auto")
    m.set_tie_rank(tie)

    def step(pf=False):
        return m.step(download=True, reduce_count=False, prefetch=pf and prefetch,
                      rule_index=True)["trie"]

    r = None
    for i in range(warmup):
        r = step(i < warmup - 1)
    barrier_sync()
    m.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        r = step(i < steps - 1)
    m.synchronize()
    barrier_sync()
    ms_step = max_over_ranks((time.perf_counter() - t0) * 1000.0 / max(steps, 1))
    st = r["stats"]
    d = digest_of(N, r)
    ok = ok_ix = None
    if verify:
        ref = N.mine_cpu(data.tx_ptr, data.items, data.n_items, ms, 0)
        ok = digest_of(N, ref)["digest"] == d["digest"]
        ok_ix = index_equal(r["index"], cpu_index(N, data, ms, data.names))
    parts = gather((int(d["n"]), ok, ok_ix))
    n_total = sum(p[0] for p in parts)
    out = {"min_support": ms, "parallelism": f"dp{world}-one-dataset-per-gpu" if weak else
           "single", "ms_per_step": round(ms_step, 4), "n_itemsets": n_total,
           "n_itemsets_per_dataset": int(d["n"]),
           "itemsets_per_s": round(n_total / (ms_step / 1000.0), 1),
           "n_rules": int(r["index"]["nnz"]), "digest": d["digest"],
           "verified_digest": None if not verify else all(bool(p[1]) for p in parts),
           "verified_rule_map_vs_cpu": None if not verify else all(bool(p[2]) for p in parts),
           "levels_path": st.get("levels_path"),
           "step_overlap": "launch-ahead: step k+1's call is launched before step k's is waited"
                           " for" if prefetch else "none"}
    if "phases_ms" in st:
        out["phases_ms"] = st["phases_ms"]
    del m
    return out


# ---------------------------------------------------------------------------------------------
# BASELINE config 2
# ---------------------------------------------------------------------------------------------
def run_config2(N, tx, names, tie, steps: int, verify: bool, deep_miner=None,
                full_budget_s: float = 20.0) -> Dict:
    """BASELINE config 2: ds1 @ min_support 0.01 on 1 GPU."""
    ms = 0.01
    # a 64 GB arena for the 1e8-node 4-item trie: the fused level loop (1G-candidate look-back
    # window) runs it from the second call on, once the first has sized the trie arrays
    g = N.GpuMiner(0, 64 << 30)
    g.load_csr(tx.tx_ptr, tx.items, tx.n_items)
    g.set_tie_rank(tie)
    out = {"min_support": ms, "model": "fpgrowth-ds1-shape", "global_batch": int(tx.n_tx),
           "seq_len": int(tx.n_items)}
    # (a) the deployed artifact: rule map = 1- and 2-itemsets, built and downloaded as a CSR
    for _ in range(2):
        r = g.mine(ms, 2, download=True, rule_index=True)
    g.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = g.mine(ms, 2, download=True, rule_index=True)
    g.synchronize()
    dt = (time.perf_counter() - t0) / steps
    st = r["stats"]
    a = {"ms_per_step": round(dt * 1e3, 4), "steps": steps,
         "n_keys": int(st["n_frequent_items"]), "n_rules": int(r["index"]["nnz"]),
         "n_itemsets": int(st["n_itemsets"])}
    if verify:
        ref = cpu_index(N, tx, ms, names)
        a["verified_vs_cpu_index"] = index_equal(r["index"], ref)
        cpu = N.mine_cpu(tx.tx_ptr, tx.items, tx.n_items, ms, 2)
        a["verified_digest"] = digest_of(N, r)["digest"] == digest_of(N, cpu)["digest"]
    out["rule_map"] = a
    # (b) every frequent itemset of size <= 4 + supports, materialised as a trie and downloaded
    r = g.mine(ms, 4, download=True, rule_index=True)
    g.synchronize()
    k = max(1, steps // 4)
    t0 = time.perf_counter()
    for _ in range(k):
        r = g.mine(ms, 4, download=True, rule_index=True)
    g.synchronize()
    dt = (time.perf_counter() - t0) / k
    st = r["stats"]
    d4 = digest_of(N, r)
    b = {"max_len": 4, "ms_per_step": round(dt * 1e3, 3), "steps": k,
         "n_itemsets": int(st["n_itemsets"]), "itemsets_per_s": round(st["n_itemsets"] / dt, 1),
         "per_level": d4["per_depth"][1:], "levels_path": st.get("levels_path")}
    del r
    if verify:
        cpu = N.mine_cpu(tx.tx_ptr, tx.items, tx.n_items, ms, 4)
        b["verified_digest"] = d4["digest"] == digest_of(N, cpu)["digest"]
        del cpu
    out["mine_max_len4"] = b
    del g
    # (c) full mining at 0.01, count-only: the size cap is raised while a call stays in budget
    if deep_miner is not None:
        f = deep_capped(deep_miner, ms, full_budget_s)
        f["verified_max_len4_vs_trie"] = None
        if f["trail"] and f["trail"][0]["max_len"] == 4:
            r4 = deep_miner.mine(ms, 4)
            f["verified_max_len4_vs_trie"] = r4["digest"] == d4["digest"]
        off = offline_full_count()
        if off is not None:
            # the complete result, counted once in 256 virtual-rank calls (55 GPU-minutes: too
            # long for a bench step); this step's size-capped per-size counts must equal its prefix
            L = f["max_len"]
            f["complete_count_offline"] = {
                k: off[k] for k in ("n_itemsets", "max_depth", "digest", "one_gpu_s",
                                    "itemsets_per_s", "world_virtual")}
            f["complete_count_offline"]["source"] = OFFLINE_SOURCE
            f["capped_counts_match_offline_prefix"] = (
                f["per_level"] == [int(x) for x in off["per_level"][1:L + 1]])
        out["full_mining"] = f
        out["complete_subset"] = config2_complete_subset(deep_miner.g, ms)
    return out


# ---------------------------------------------------------------------------------------------
# BASELINE config 3
# ---------------------------------------------------------------------------------------------
def sampled_supports_ok(trie, ptr, items, world: int, rank: int, k: int = 64,
                        seed: int = 0) -> Optional[bool]:
    """Independent check of a tx-DP result: `k` itemsets sampled from rank 0's trie (every size
    >= 2 represented) get their supports recounted on the host from each rank's CSR shard
    (tid-list intersection) and summed over the ranks; all must equal the trie's counts."""
    import torch.distributed as dist
    box = [None]
    if rank == 0:
        par, it, cnt = (np.asarray(trie[x]) for x in ("parent", "item", "count"))
        dep = np.asarray(trie["depth"])
        rng = np.random.default_rng(seed)
        picks = []
        for d in range(2, int(dep.max()) + 1):
            idx = np.flatnonzero(dep == d)
            picks += rng.choice(idx, size=min(len(idx), max(1, k // int(dep.max()))),
                                replace=False).tolist()
        sample = []
        for n in picks:
            s, m = [], int(n)
            while m >= 0:
                s.append(int(it[m]))
                m = int(par[m])
            sample.append((tuple(sorted(s)), int(cnt[int(n)])))
        box = [sample]
    if world > 1:
        dist.broadcast_object_list(box, src=0)
    sample = box[0]
    want = np.unique(np.array([x for s, _ in sample for x in s], np.int64))
    pos = np.flatnonzero(np.isin(items, want))
    tx_of = np.searchsorted(ptr, pos, side="right") - 1
    it_at = np.asarray(items)[pos]
    tids = {int(x): np.unique(tx_of[it_at == x]) for x in want}
    local = np.zeros(len(sample), np.int64)
    for q, (s, _) in enumerate(sample):
        t = tids[s[0]]
        for x in s[1:]:
            t = np.intersect1d(t, tids[x], assume_unique=True)
        local[q] = len(t)
    if world > 1:
        import torch
        tl = torch.from_numpy(local)
        if dist.get_backend() == "nccl":
            tl = tl.cuda()
        dist.all_reduce(tl)
        local = tl.cpu().numpy()
    return bool(all(int(local[q]) == c for q, (_, c) in enumerate(sample))) if rank == 0 else None


def run_config3(N, world: int, rank: int, device: int, steps: int = 5, warmup: int = 1,
                comm: str = "host", min_support: float = C3_MIN_SUPPORT,
                mode: str = "tx", shape_name: str = "10Mx1M",
                rules_min_confidence: float = 0.0) -> Dict:
    """BASELINE config 3 (10M transactions x 1M items; min_support 2e-4: 14.8k frequent items)
    on all ranks of the job: transaction-DP mining (each rank generates and encodes only its
    shard; supports, the MFMA gram and per-level candidate counts all-reduced), so support /
    encode / gram work shrinks with N.  Verified by recounting sampled itemsets' supports on the
    host from the CSR shards (sampled_supports_ok); the digest is reported (it must not depend
    on N)."""
    import torch
    import torch.distributed as dist
    from ..data.synthetic import SHAPES
    from ..parallel.dist_miner import DistMiner, shard_bounds
    prev = os.environ.get("KMLS_COMM")
    os.environ["KMLS_COMM"] = comm
    try:
        shape = SHAPES[shape_name]
        T = shape.n_tx
        lo, hi, _ = shard_bounds(T, world, rank)
        ptr, items = N.synth_transactions(T, shape.n_items, shape.mean_len, shape.n_genres,
                                          shape.genre_affinity, 0.85, 0, 0, lo, hi)
        dm = DistMiner(ptr, items, shape.n_items, min_support, device=device, mode=mode,
                       support_tiles=4, global_n_tx=T, arena_bytes=48 << 30)

        def bar():
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
                torch.cuda.synchronize()
        r = None
        for _ in range(warmup):
            r = dm.step(download=True)
        bar()
        t0 = time.perf_counter()
        for _ in range(steps):
            r = dm.step(download=True)
        dm.synchronize()
        bar()
        ms = (time.perf_counter() - t0) * 1000.0 / max(1, steps)
        if world > 1:
            t = torch.tensor([ms], dtype=torch.float64,
                             device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ms = float(t.item())
        st = r["stats"]
        out = {"model": f"fpgrowth-{shape_name}-synthetic", "global_batch": T, "seq_len": shape.n_items,
               "min_support": min_support, "n_gpus": world,
               "parallelism": f"tx-dp{world}" if mode == "tx" else f"item-shard{world}",
               "comm": comm, "steps": steps, "ms_per_step": round(ms, 3),
               "tx_per_s": round(T / (ms / 1000.0), 1),
               "n_frequent_items": int(st.get("n_frequent_items", 0)),
               "phases_ms": {k: round(v, 3) for k, v in (st.get("phases_ms") or {}).items()},
               "levels_path": st.get("levels_path"), "level2_method": st.get("level2_method")}
        if "horizontal" in st:
            out["horizontal"] = st["horizontal"]
        trie = r["trie"]
        if mode == "shard":  # per-rank sub-tries -> the whole trie on rank 0
            from ..parallel.dist_miner import gather_trie
            trie = gather_trie(trie, rank, world, int(st["n_frequent_items"]))
            out["bitmap_bytes_per_rank"] = int(st["own_bitmap_bytes"])
            out["replicated_bitmap_bytes"] = int(st["replicated_bitmap_bytes"])
            out["peak_batch_bitmap_bytes"] = int(st["peak_batch_bitmap_bytes"])
            out["rounds"] = int(st["rounds"])
            out["max_batch_rows"] = int(st["max_batch_rows"])
            out["shard_phases_ms"] = {k: round(v * 1e3, 1) for k, v in st["host_phases_s"].items()}
        ok = sampled_supports_ok(trie if rank == 0 else None, ptr, items, world, rank)
        if rank == 0:
            d = digest_of(N, trie)
            n = int(d["n"])
            out["n_itemsets"] = n
            out["per_level"] = d["per_depth"][1:]
            out["itemsets_per_s"] = round(n / (ms / 1000.0), 1)
            out["digest"] = d["digest"]
            out["verified_sampled_supports"] = ok
            if rules_min_confidence > 0:
                # rule generation on the mined trie (machine-learning/main.py:224-260's
                # association_rules(metric="confidence")), the HIP rule_score kernels
                from ..models.fpgrowth import ItemsetTrie
                from ..models.rules import rules_from_trie
                tr = ItemsetTrie(np.asarray(trie["parent"]), np.asarray(trie["item"]),
                                 np.asarray(trie["count"]), np.asarray(trie["depth"]), T,
                                 min_support)
                best = None
                for _ in range(3):
                    t1 = time.perf_counter()
                    rules = rules_from_trie(tr, "confidence", rules_min_confidence,
                                            backend="gpu", device=device)
                    dt = (time.perf_counter() - t1) * 1000.0
                    best = dt if best is None else min(best, dt)
                cpu = rules_from_trie(tr, "confidence", rules_min_confidence, backend="cpu")
                out["rules"] = {"metric": "confidence", "min_confidence": rules_min_confidence,
                                "n_rules": len(rules), "ms": round(best, 3),
                                "backend": "gpu (rule_score)",
                                "equal_cpu": len(rules) == len(cpu) and all(
                                    np.array_equal(getattr(rules, f), getattr(cpu, f))
                                    for f in ("itemset", "antecedent", "consequent"))}
        del dm
        return out
    finally:
        if prev is None:
            os.environ.pop("KMLS_COMM", None)
        else:
            os.environ["KMLS_COMM"] = prev


def run_job_full(tx, ms: float, want_digest: Optional[str] = None,
                 want_per_level=None) -> Dict:
    """The PRODUCT path at the headline support: the job (``job.main.run``, MINER=gpu,
    RULES_MODE=full) on a reference-schema CSV of this dataset — CSV ingest, pre-processing
    artifacts, every frequent itemset through the deep engine (emit -> device trie compaction
    -> host), the device rule map, ``recommendations.pickle`` / ``rules.idx`` and the
    1.4e9-itemset ``frequent_itemsets.npz``, marker last (machine-learning/main.py:421-484).
    Track names are made unique (``name #id``) so the job's name codes map back to this
    dataset's item ids: the written trie, relabelled, must carry the headline's digest."""
    import dataclasses
    import shutil
    import tempfile
    from ..config import JobSettings
    from ..data.synthetic import to_reference_csv
    from ..job import main as job
    from ..ops import native
    N = native.load()
    root = tempfile.mkdtemp(prefix="kmls_job_full_")
    try:
        names = [f"{n} #{i:05d}" for i, n in enumerate(tx.names or [f"t{i}" for i in range(tx.n_items)])]
        ds = os.path.join(root, "datasets")
        os.makedirs(ds)
        to_reference_csv(dataclasses.replace(tx, names=names), os.path.join(ds, "2023_spotify_ds1.csv"))
        import pathlib
        base = pathlib.Path(root) / "api-data"
        cfg = JobSettings(min_support=ms, base_dir=base, datasets_dir=pathlib.Path(ds),
                          pickles_folder=base / "pickles",
                          recommendations_file="recommendations.pickle",
                          best_tracks_file="best_tracks.pickle",
                          data_invalidation_file="last_execution.txt",
                          regex_filename="2023_spotify_ds*.csv", top_tracks_save_percentile=0.03,
                          miner="gpu", rules_mode="full")
        t0 = time.perf_counter()
        st = job.run(cfg)
        wall = time.perf_counter() - t0
        npz = base / "pickles" / "frequent_itemsets.npz"
        out = {"min_support": ms, "wall_s": round(wall, 2), "rule_seconds": round(st["rule_seconds"], 3),
               "n_itemsets": int(st["n_itemsets"]), "backend": st.get("backend"),
               "rule_map": st.get("rule_map"), "n_keys": int(st["n_keys"]),
               "npz_bytes": npz.stat().st_size,
               "what": "job.main.run end to end: CSV -> artifacts -> deep-engine trie -> npz, "
                       "marker last"}
        t1 = time.perf_counter()
        z = np.load(npz)
        par, item, cnt, dep = z["parent"], z["item"], z["count"], z["depth"]
        # job name code -> dataset item id (the "#id" suffix), then the content digest
        code_names = job_names(cfg)
        back = np.array([int(n.rsplit("#", 1)[1]) for n in code_names], dtype=np.int32)
        d = N.trie_digest(par, back[item.astype(np.int64)], cnt, dep)
        out["verify_s"] = round(time.perf_counter() - t1, 2)
        out["digest"] = d["digest"]
        out["per_level"] = [int(v) for v in d["per_depth"][1:]]
        if want_digest is not None:
            out["verified_digest"] = d["digest"] == want_digest
        if want_per_level is not None:
            out["per_level_equal_headline"] = out["per_level"] == [int(v) for v in want_per_level]
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def job_names(cfg) -> list:
    """The job's item-code -> track-name table for its (single) dataset: the same CSV read,
    cleaning and group-by as the job."""
    from ..job import preprocess as pp
    path = sorted(cfg.datasets_dir.glob(cfg.regex_filename))[0]
    t = pp.clean_df(pp.read_tracks(str(path), 1.0, verbose=False))
    return list(pp.group_tracks_by_playlist(t).names)
