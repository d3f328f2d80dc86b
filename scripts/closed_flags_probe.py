"""Probe of the closed / maximal flag paths on the ds1 shape: for each support, the median wall
time (after one warm-up call) of

* ``deep_trie_flags``    — the kernel on the device-resident deep trie, flag bytes downloaded;
* ``itemset_flags_gpu``  — the host trie uploaded, kernel, flag bytes downloaded;
* ``itemset_flags``      — the threaded CPU twin;

plus the kernel-only times and the closed / maximal counts.  GPU box only.

    python scripts/closed_flags_probe.py --supports 0.05,0.03 [--reps 5] [--shape ds1]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")


def timed(fn, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supports", default="0.05,0.03")
    ap.add_argument("--shape", default="ds1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true",
                    help="device-resident path only (tries too large to widen on the host)")
    a = ap.parse_args()
    from kubernetes_machine_learning_server_amd.data.synthetic import generate
    from kubernetes_machine_learning_server_amd.ops import native
    N = native.require_gpu()
    tx = generate(a.shape, seed=0)
    g = N.GpuMiner(0)
    g.load_csr(tx.tx_ptr, tx.items, tx.n_items)
    for ms in (float(s) for s in a.supports.split(",")):
        g.mine_deep(ms, emit=True)
        t = g.deep_arena_trie(1, 0)
        dev = timed(g.deep_trie_flags, a.reps)
        f = dev[3]["flags"]
        out = {"shape": a.shape, "support": ms, "n_itemsets": int(t["n"]),
               "max_depth": int(t["depth"].max()), "closed": int(((f & 1) != 0).sum()),
               "maximal": int(((f & 2) != 0).sum()), "reps": a.reps,
               "deep_trie_flags_ms": [round(x, 3) for x in dev[:3]],
               "deep_trie_flags_kernel_ms": round(dev[3]["kernel_ms"], 3)}
        if not a.no_host:
            args = (np.ascontiguousarray(t["parent"], np.int64),
                    np.ascontiguousarray(t["item"], np.int32),
                    np.ascontiguousarray(t["count"], np.uint32),
                    np.ascontiguousarray(t["depth"], np.uint8))
            up = timed(lambda: N.itemset_flags_gpu(*args), a.reps)
            cpu = timed(lambda: N.itemset_flags(*args), a.reps)
            out["itemset_flags_gpu_ms"] = [round(x, 3) for x in up[:3]]
            out["itemset_flags_gpu_kernel_ms"] = round(up[3]["kernel_ms"], 3)
            out["itemset_flags_cpu_ms"] = [round(x, 3) for x in cpu[:3]]
            out["all_equal"] = bool((up[3]["flags"] == f).all() and (cpu[3] == f).all())
        print(json.dumps(out), flush=True)
        del t


if __name__ == "__main__":
    main()
