"""Probe of the generator / closure flags and the min-max rule basis on the ds1 shape.  GPU box only.

``--mode flags``: for each support, the device time (``kernel_ms``, HIP events: hash build + marks
+ fold [+ resolve]) of the two-bit call and, where the build has it, of the three-bit + closure
call, on the device-resident deep trie and on the uploaded host trie: median (min - max) of
``--reps`` calls after one warm-up, plus closed / generator counts.  On a build without the new
calls (the parent commit) only the two-bit figures are printed, so the same command measures both
sides of the comparison: ``--root`` names the checkout whose package is imported.

``--mode rules``: for each support, rule counts and times of ``basis="all"`` against ``"minmax"``
at ``--metric confidence --min-threshold 0.5``: ``kernel_ms`` of the GPU engine and wall time of
the CPU twin.  ``"all"`` is skipped (and said so) when its candidate count, the sum of 2^k - 2 over
the itemsets, times 40 bytes per rule exceeds ``--max-gb``.

    python scripts/rule_basis_probe.py --mode flags --supports 0.05,0.03 [--reps 5] [--root DIR]
    python scripts/rule_basis_probe.py --mode rules --supports 0.05 [--no-cpu]
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np


def kernel_ms(fn, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        out = fn()
        ts.append(float(out["kernel_ms"]))
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)], out


def wall_ms(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)], out


def widen(t):
    return (np.ascontiguousarray(t["parent"], np.int64), np.ascontiguousarray(t["item"], np.int32),
            np.ascontiguousarray(t["count"], np.uint32), np.ascontiguousarray(t["depth"], np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("flags", "rules"), required=True)
    ap.add_argument("--supports", default="0.05,0.03")
    ap.add_argument("--shape", default="ds1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=".", help="checkout whose package is imported")
    ap.add_argument("--min-threshold", type=float, default=0.5)
    ap.add_argument("--max-gb", type=float, default=16.0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    from kubernetes_machine_learning_server_amd.data.synthetic import generate
    from kubernetes_machine_learning_server_amd.ops import native
    N = native.require_gpu()
    new = hasattr(N, "itemset_condense_gpu")
    tx = generate(a.shape, seed=0)
    g = N.GpuMiner(0)
    g.load_csr(tx.tx_ptr, tx.items, tx.n_items)
    for ms in (float(s) for s in a.supports.split(",")):
        g.mine_deep(ms, emit=True)
        t = g.deep_arena_trie(1, 0)
        n = int(t["n"])
        out = {"mode": a.mode, "shape": a.shape, "support": ms, "n_itemsets": n,
               "max_depth": int(t["depth"].max()), "reps": a.reps, "three_bit_build": new}
        args = widen(t)
        if a.mode == "flags":
            out["deep_two_bit_kernel_ms"], r = kernel_ms(g.deep_trie_flags, a.reps)
            out["closed"] = int(((r["flags"] & 1) != 0).sum())
            out["upload_two_bit_kernel_ms"], _ = kernel_ms(lambda: N.itemset_flags_gpu(*args), a.reps)
            if new:
                out["deep_three_bit_closure_kernel_ms"], r3 = kernel_ms(
                    lambda: g.deep_trie_flags(generators=True, closure=True), a.reps)
                out["deep_three_bit_kernel_ms"], _ = kernel_ms(
                    lambda: g.deep_trie_flags(generators=True), a.reps)
                out["upload_three_bit_closure_kernel_ms"], u3 = kernel_ms(
                    lambda: N.itemset_condense_gpu(*args), a.reps)
                out["generators"] = int(((r3["flags"] & 4) != 0).sum())
                out["equal"] = bool((r3["flags"] == u3["flags"]).all() and
                                    (r3["closure"] == u3["closure"]).all() and
                                    ((r3["flags"] & 3) == r["flags"]).all())
        else:
            cand = int(((1 << t["depth"].astype(np.int64)) - 2).sum())
            out["candidate_rules_all"] = cand
            rargs = args + (int(tx.n_tx), 0, a.min_threshold, 0)
            for name, basis in (("minmax", 1), ("all", 0)):
                if basis == 0 and cand * 40 > a.max_gb * 2 ** 30:
                    out["all_skipped"] = (f"{cand} candidate rules x 40 B exceed "
                                          f"{a.max_gb} GB")
                    continue
                try:
                    out[f"gpu_{name}_kernel_ms"], r = kernel_ms(
                        lambda: N.association_rules_gpu(*rargs, 0, basis), a.reps)
                except RuntimeError as e:  # the output did not fit
                    out[f"gpu_{name}_error"] = str(e)[:200]
                    continue
                out[f"{name}_rules"] = int(len(r["itemset"]))
                out[f"{name}_exact_rules"] = int((r["confidence"] == 1.0).sum())
                if not a.no_cpu:
                    out[f"cpu_{name}_wall_ms"], c = wall_ms(
                        lambda: N.association_rules(*rargs, 0, basis), min(a.reps, 3))
                    out[f"{name}_equal"] = bool(
                        all(np.array_equal(r[k], c[k]) for k in
                            ("itemset", "antecedent", "consequent", "confidence")))
                del r
        print(json.dumps(out), flush=True)
        del t, args


if __name__ == "__main__":
    main()
