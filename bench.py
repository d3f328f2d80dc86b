#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json metric): FP-Growth itemsets/sec mined on MI355X, plus the
serving half (p50 /api/recommend/ at fixed QPS).

Headline step = FULL mining of one ds1-shape dataset at min_support 0.02: every frequent itemset
of every size (1,414,082,373 itemsets, up to 19 items) and its support is computed on the
device — per-item supports → frequent-item selection → tid-bitmap encode (the reference's
one-hot) → level-2 classes → a persistent depth-first wave-per-task miner
(``csrc/kernels/deep.hip``) that counts per size and folds every (itemset, support) into an
order-independent digest instead of materialising 1.4e9 trie nodes (count-only; the digest equals
the digest of the full trie, ``kmls/digest.hpp``).  Verified: per-size counts and digest equal to
the native CPU miner's whole-problem count (``bench/bench_mine.CPU_REF``).

Multi-GPU (``torchrun --nproc-per-node N``, one rank per GPU): **strong scaling** — the SAME
problem is split over the ranks (every rank builds the deterministic level-2 classes itself,
measures every level-3 task's cost on the device, and takes its share of the cost-ordered snake
deal), and the per-size counts + digest sums are all-reduced,
digest xors all-gathered, over RCCL (torch.distributed on the nccl group); every rank ends with
the whole-problem result and verifies it.  ``value`` = itemsets of the problem ÷ the slowest
rank's step.

A plain run (``bench.py --gpus 1 --steps N --warmup W``) sets up, warms up, times the N headline
steps and prints the result line; ``--dump-outputs DIR`` also writes what the last timed step
returned (per-size counts, totals, digest) as ``DIR/<name>.npy``.  Everything below is measured
only with ``--full``.

Secondary fields (``--full``):
* ``serve.hip_loop`` — the same harness with the persistent HIP serving kernel forced
                    (``SERVE_BACKEND=loop``): every request answered by the polling kernel.
* ``serve``       — config 4, run FIRST in a fresh child process (this process has not touched
                    the GPU yet): native HTTP front + open-loop native load generator, latency
                    from the scheduled send time, fixed QPS points and the capacity (max QPS with
                    p99 < 5 ms).
* ``job_full``    — the product path at the headline support (N = 1): ``job.main.run`` end to
                    end on a reference-schema CSV of the same data (artifacts, the deep engine's
                    trie of all 1.4e9 itemsets written to ``frequent_itemsets.npz``, rule map,
                    marker last); wall time, and the written trie's digest (relabelled to the
                    dataset's ids) equal to the headline digest.
* ``levelwise_0.05`` — the round-2 headline form (ds1 @0.05 through the level-wise graph path,
                    trie download + device rule map in the step, verified against the CPU miner);
                    at N > 1 one relabelled dataset per rank (weak scaling).
* ``config2``     — ds1 @0.01: deployed rule map, truncated-at-4 trie, full count-only mining
                    with the size cap raised within a time budget (N = 1).
* ``config3``     — 10M x 1M @2e-4 (14.8k frequent items) transaction-DP over all ranks
* ``config5``     — 100M transactions x 1M items @2e-4 (BASELINE config 5) on all ranks: each
                    rank generates its transaction shard; the deployed rule map (pair supports
                    counted from the CSR, row blocks reduce-scattered, per-rank CSR, gather),
                    then rules.idx + hot reload + batched queries; gram rows and sampled
                    rule-map rows re-counted on the host.
* ``config3_shard`` — the same problem item-sharded (every N): the ranks all-gather their
                    frequent-rank CSRs, then each counts the pair rows and the horizontal
                    levels of its own items (``GpuMiner.mine_shard``, no bitmap, no count
                    reduction); sub-tries gathered on rank 0, digest compared with tx mode,
                    sampled supports recounted on the host from the CSR shards.
* ``config5_mine`` — config 5's data (100M x 1M @2e-4) mined completely at every N (tx-DP, every
                    frequent itemset of every size), sampled supports recounted on the host,
                    plus confidence rules (HIP rule_score) on rank 0, compared with the C++ rules.
* ``config3_wide`` — config 3's data at 7e-5 (59,664 frequent items; N = 1): the sparse path
                    past 32,768 ranks, sampled supports recounted on the host.
* ``native_rccl`` — at N > 1 the headline combine once more through the native RCCL
                    communicator (``csrc/host/comm_rccl.cpp``), digest compared.

Data: synthetic playlists of the reference's ds1/ds2 shape (2,246 playlists × 2,171 tracks),
calibrated by ``bench/calibrate.py``; random-init item vocabulary.
``vs_baseline`` = the SAME-config ratio: the reference's published 20.31 s (ds2 shape @0.05,
relatorio.pdf p.6) ÷ the ``levelwise_0.05`` step (this data @0.05, trie + rule map);
``vs_reference_replay`` uses the 7.24 s replay of the reference timed region on this data
(profiles/r2_calibration.md).  ``rate_ratio_0.02_vs_published_0.05`` keeps the old, not
like-for-like rate ratio for continuity.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

REF_SECONDS_DS2_005 = 20.313968  # relatorio.pdf p.6, mlxtend fpgrowth + rule map, ds2 @0.05
REPLAY_SECONDS_DS1_005 = 7.24    # replay of the reference timed region on this data
ITEMSETS_DS1_005 = 77905         # itemsets of the synthetic ds1 @0.05 (the published point)
REF_RATE = ITEMSETS_DS1_005 / REF_SECONDS_DS2_005
REPLAY_RATE = ITEMSETS_DS1_005 / REPLAY_SECONDS_DS1_005


class Watchdog:
    """Bounded sections: if a section overruns, rank 0 prints the line built so far (with the
    section named) and every rank exits, instead of the whole job hanging."""

    def __init__(self, out: dict, rank: int):
        self.out, self.rank = out, rank
        self.name, self.deadline = None, None
        self.lock = threading.Lock()
        threading.Thread(target=self._run, daemon=True).start()

    def _run(self):
        while True:
            time.sleep(1.0)
            with self.lock:
                if self.deadline is None or time.time() < self.deadline:
                    continue
                name = self.name
            if self.rank == 0:
                self.out.setdefault("errors", {})[name] = "timed out"
                print(json.dumps(self.out), flush=True)
            print(f"[bench] section {name} timed out; exiting", file=sys.stderr, flush=True)
            os._exit(0 if "value" in self.out else 1)

    def arm(self, name: str, seconds: float):
        with self.lock:
            self.name, self.deadline = name, time.time() + seconds

    def disarm(self):
        with self.lock:
            self.name, self.deadline = None, None


def run_serve_child(qps: str, duration: float, backend: str, timeout: float = 420.0,
                    extra=(), capacity: bool = True) -> dict:
    """Config 4 in a fresh child process (PVC populated by the real job on the CPU miner, the
    native-front server as its own child, the native open-loop load generator)."""
    fd, path = tempfile.mkstemp(prefix="kmls_serve_", suffix=".json")
    os.close(fd)
    cmd = [sys.executable, "-m", "kubernetes_machine_learning_server_amd.bench.bench_serve",
           "--backend", backend, "--qps", qps, "--duration", str(duration),
           "--json-out", path] + (["--capacity"] if capacity else []) + list(extra)
    try:
        p = subprocess.run(cmd, stdout=sys.stderr, stderr=sys.stderr, timeout=timeout)
        if p.returncode != 0:
            return {"error": f"bench_serve exited {p.returncode}"}
        with open(path) as f:
            s = json.load(f)
    except subprocess.TimeoutExpired:
        return {"error": f"bench_serve timed out after {timeout:.0f} s"}
    finally:
        os.unlink(path)
    keep = ("offered_qps", "achieved_qps", "p50_ms", "p90_ms", "p99_ms", "p999_ms", "max_ms",
            "errors", "unanswered", "send_lag_p99_ms")
    out = {k: s.get(k) for k in ("backend", "front", "threads", "client", "duration_s",
                                 "gpu_index", "gpu_min_batch", "server_ready_s", "cpu")}
    out["latency_from"] = "scheduled send time (open loop)"
    out["points"] = [{k: p_.get(k) for k in keep} for p_ in s.get("points", [])]
    cap = s.get("capacity") or {}
    out["capacity"] = {k: cap.get(k) for k in ("capacity_qps", "max_qps_p99_under_ms",
                                               "at_capacity", "limit_hit")}
    out["front_stats"] = s.get("front_stats")
    if s.get("reload_under_load"):
        out["reload_under_load"] = s["reload_under_load"]
    return out


def dump_outputs(path: str, r: dict) -> None:
    """What the last timed headline step returned to its caller (the whole-problem result of
    ``DeepMiner.mine``), one float64 ``.npy`` per field; every value is an integer below 2^53,
    so float64 holds it exactly.  The 128-bit digest is written as four 32-bit words (sum high,
    sum low, xor high, xor low)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    dg = r["digest"]
    arrays = {
        "per_level": [int(x) for x in r["per_level"]],
        "n_itemsets": [int(r["n_itemsets"])],
        "max_depth": [int(r["max_depth"])],
        "n_frequent_items": [int(r["n_frequent_items"])],
        "digest_words": [int(dg[i:i + 8], 16) for i in range(0, 32, 8)],
    }
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(v, dtype=np.float64))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-support", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-verify", action="store_true", help="skip the CPU-miner checks")
    ap.add_argument("--serve-qps", default="2000,5000,10000",
                    help="offered QPS points for the serving half ('' = skip)")
    ap.add_argument("--serve-duration", type=float, default=4.0)
    ap.add_argument("--serve-backend", default="auto")
    ap.add_argument("--no-serve-reference", action="store_true",
                    help="skip the reference-stack serving baseline (uvicorn + Python matcher)")
    ap.add_argument("--serve-loop-qps", default="2000,5000,10000",
                    help="QPS points with the persistent HIP serving kernel forced ('' = skip)")
    ap.add_argument("--no-config5-serve", action="store_true",
                    help="skip serving the config-5 index across a hot reload (10k QPS)")
    ap.add_argument("--no-levelwise", action="store_true")
    ap.add_argument("--no-emit", action="store_true", help="skip the materialising headline run")
    ap.add_argument("--no-config2", action="store_true")
    ap.add_argument("--no-job", action="store_true", help="skip the job at the headline support")
    ap.add_argument("--no-config5", action="store_true", help="skip the 100M-transaction rule map")
    ap.add_argument("--config5-steps", type=int, default=3)
    ap.add_argument("--no-config3", action="store_true")
    ap.add_argument("--cpu", action="store_true",
                    help="CPU tier of the headline (native CPU count miner, gloo): no GPU")
    ap.add_argument("--comm", default=os.environ.get("KMLS_BENCH_COMM", "torch"),
                    help="N>1 headline combine: torch (torch.distributed/RCCL) | rccl | host")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary section (serve, emit, job_full, levelwise, "
                         "config 2/3/5, native_rccl); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed headline step returned as DIR/<name>.npy")
    args = ap.parse_args()
    if not args.full:  # a plain run: set up, warm up, time the headline steps, print the line
        args.serve_qps = ""
        args.no_emit = args.no_job = args.no_levelwise = True
        args.no_config2 = args.no_config3 = args.no_config5 = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"[bench] warning: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)

    # ---- config 4 first, in a fresh child: this process has not touched the GPU yet ----
    serve = None
    if world == 1 and args.serve_qps and not args.cpu:
        t = time.time()
        serve = run_serve_child(args.serve_qps, args.serve_duration, args.serve_backend)
        serve["wall_s"] = round(time.time() - t, 1)
        # the same harness (open-loop native load generator, same PVC build, same queries)
        # against the reference's serving stack: one uvicorn worker (rest_api/Dockerfile:28)
        # running the reference-semantics Python matcher (rest_api/app/main.py:224-254)
        if not args.no_serve_reference:
            t = time.time()
            ref = run_serve_child(args.serve_qps, args.serve_duration, "python", timeout=300,
                                  extra=("--front", "uvicorn", "--workers", "1"),
                                  capacity=False)
            ref["wall_s"] = round(time.time() - t, 1)
            serve["reference_stack"] = ref
            try:
                serve["p50_ratio_reference_over_this"] = [
                    round(r["p50_ms"] / m["p50_ms"], 1)
                    for r, m in zip(ref["points"], serve["points"]) if m.get("p50_ms")]
            except Exception:  # noqa: BLE001 — a failed reference run leaves the field out
                pass
        # the persistent HIP serving kernel forced on (SERVE_BACKEND=loop): every request the
        # native front receives is answered by the polling kernel (front_stats.gpu_loop_batches)
        if args.serve_loop_qps:
            t = time.time()
            loop = run_serve_child(args.serve_loop_qps, 3.0, "loop", timeout=360, capacity=True)
            loop["wall_s"] = round(time.time() - t, 1)
            serve["hip_loop"] = loop

    import numpy as np
    import torch
    from kubernetes_machine_learning_server_amd.bench import bench_mine as bm
    from kubernetes_machine_learning_server_amd.data.synthetic import generate
    from kubernetes_machine_learning_server_amd.ops import native

    # KMLS_BENCH_DIST=gloo rehearses the N-rank path with ranks sharing GPUs (round robin)
    dist_backend = os.environ.get("KMLS_BENCH_DIST", "gloo" if args.cpu else "nccl")
    device = local_rank
    if world > 1 and args.cpu:
        import datetime
        import torch.distributed as dist
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=300))
    elif world > 1:
        import datetime
        import torch.distributed as dist
        if dist_backend != "nccl":
            device = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(device)
        if dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device),
                                    timeout=datetime.timedelta(seconds=300))
        else:
            dist.init_process_group(dist_backend, timeout=datetime.timedelta(seconds=300))

    def barrier_sync():
        if not args.cpu:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            if not args.cpu:
                torch.cuda.synchronize()

    def max_over_ranks(v: float) -> float:
        if world == 1:
            return v
        t = torch.tensor([v], dtype=torch.float64,
                         device="cuda" if dist_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def gather(obj):
        if world == 1:
            return [obj]
        parts = [None] * world
        dist.all_gather_object(parts, obj)
        return parts

    N = native.load() if args.cpu else native.require_gpu()
    tx = generate("ds1", seed=args.seed)
    out: dict = {}
    wd = Watchdog(out, rank)

    # ---- headline: full mining of ONE dataset, split over the ranks ----
    wd.arm("headline", 900)
    h = bm.run_deep(tx, args.min_support, world, rank, device, args.warmup, args.steps,
                    barrier_sync, max_over_ranks, comm=args.comm if world > 1 else None,
                    cpu=args.cpu)
    wd.disarm()
    deep_miner = h.pop("_miner")
    last = h.pop("_last")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    if args.seed != 0:
        h["verified_digest"] = None
    ms_step = h["ms_per_step"]
    value = h["n_itemsets"] / (ms_step / 1000.0)
    out.update({
        "metric": "itemsets/sec mined (FP-Growth, every frequent itemset of every size + its "
                  "support, one dataset split over the GPUs)",
        "value": round(value, 1),
        "unit": "itemsets/s",
        "n_gpus": 0 if args.cpu else world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_step,
        "higher_is_better": True,
        "scaling": "strong",
        # same-config ratio, filled in by the levelwise_0.05 section below (the reference's
        # published point is ds2 @0.05; itemsets/s at 0.02 is not comparable with a 0.05 rate)
        "vs_baseline": None,
        "rate_ratio_0.02_vs_published_0.05": round(value / REF_RATE, 1),
        "baseline_basis": "vs_baseline = the reference's published 20.31 s (ds2 shape @0.05, "
                          "relatorio.pdf p.6) / this framework's step on the SAME config "
                          "(levelwise_0.05: ds1 shape @0.05, trie + rule map); the headline "
                          "value (0.02, every size) has no published counterpart",
        "dtype": "uint64 tid-bitmaps / exact integer supports" + (" (CPU)" if args.cpu else ""),
        "data": "synthetic (ds1 shape: 2,246 playlists x 2,171 tracks, calibrated to "
                "relatorio.pdf p.5-6; random-init item vocab; bench/calibrate.py)",
        "config": {
            "model": "fpgrowth-ds1-shape",
            "global_batch": int(tx.n_tx),
            "seq_len": int(tx.n_items),
            "parallelism": (f"dp{world}-level3-task-split+count-allreduce({h['comm']})"
                            if world > 1 else "single"),
            "min_support": args.min_support,
            "max_len": 0,
            "output": "count-only: per-size counts + content digest of every (itemset, support)",
            "n_itemsets": h["n_itemsets"],
            "n_frequent_items": h["n_frequent_items"],
            "max_depth": h["max_depth"],
            "miner": ("cpu count miner (mine_cpu_count)" if args.cpu else
                      "deep: persistent wave-per-task DFS over tid-projected classes (deep.hip)"),
        },
        "verified_digest": h["verified_digest"],
        "digest": h["digest"],
        "per_level": h["per_level"],
        "deep": {k: h[k] for k in ("candidates", "chunks", "level2_tasks", "rank0_phases_ms",
                                   "rank0_rounds")},
    })
    if serve is not None:
        out["serve"] = serve

    # ---- the same problem MATERIALISED: every itemset written to an HBM trie arena ----
    if not args.cpu and not args.no_emit:
        wd.arm("emit", 600)
        try:
            e = bm.run_deep_emit(deep_miner, args.min_support, world, rank, args.warmup,
                                 args.steps, barrier_sync, max_over_ranks, gather)
            e["itemsets_per_s"] = round(h["n_itemsets"] / (e["ms_per_step"] / 1000.0), 1)
            out["emit"] = e
            out["value_emitted"] = e["itemsets_per_s"]
        except Exception as ex:
            out.setdefault("errors", {})["emit"] = repr(ex)[:300]
        wd.disarm()

    # ---- the product path at the headline support: the job end to end (1 GPU) ----
    if world == 1 and not args.cpu and not args.no_job:
        wd.arm("job_full", 420)
        try:
            out["job_full"] = bm.run_job_full(tx, args.min_support, h["digest"], h["per_level"])
        except Exception as ex:
            out.setdefault("errors", {})["job_full"] = repr(ex)[:300]
        wd.disarm()

    # ---- the round-2 headline form (level-wise, trie + rule map in the step) ----
    if args.cpu:  # the GPU sections below have no CPU tier
        args.no_levelwise = args.no_config2 = args.no_config3 = True
    if not args.no_levelwise:
        wd.arm("levelwise_0.05", 300)
        try:
            lw = bm.run_levelwise(N, tx, 0.05, world, rank, device, 5, 20, barrier_sync,
                                  max_over_ranks, gather, weak=world > 1,
                                  verify=not args.no_verify)
            lw["vs_baseline_same_config"] = round(
                world * REF_SECONDS_DS2_005 * 1e3 / lw["ms_per_step"], 1)
            lw["vs_reference_replay_same_config"] = round(
                world * REPLAY_SECONDS_DS1_005 * 1e3 / lw["ms_per_step"], 1)
            out["levelwise_0.05"] = lw
            out["vs_baseline"] = lw["vs_baseline_same_config"]
            out["vs_reference_replay"] = lw["vs_reference_replay_same_config"]
        except Exception as e:
            out.setdefault("errors", {})["levelwise_0.05"] = repr(e)[:300]
        wd.disarm()

    # ---- BASELINE config 2 (1 GPU) ----
    if world == 1 and not args.no_config2:
        from kubernetes_machine_learning_server_amd.serve.index import name_tie_rank
        wd.arm("config2", 520)
        try:
            tie = name_tie_rank(tx.names) if tx.names else np.arange(tx.n_items, dtype=np.int32)
            out["config2"] = bm.run_config2(N, tx, tx.names, tie, steps=10,
                                            verify=not args.no_verify, deep_miner=deep_miner)
        except Exception as e:
            out.setdefault("errors", {})["config2"] = repr(e)[:300]
        wd.disarm()

    # ---- the headline combine through the native RCCL communicator ----
    if args.full and world > 1 and dist_backend == "nccl" and args.comm != "rccl" \
            and not args.cpu:
        os.environ.setdefault("KMLS_COMM_TIMEOUT_S", "60")
        wd.arm("native_rccl", 240)
        try:
            r2 = bm.run_deep(tx, args.min_support, world, rank, device, 1, 3, barrier_sync,
                             max_over_ranks, comm="rccl")
            r2.pop("_miner")
            out["native_rccl"] = {"ms_per_step": r2["ms_per_step"],
                                  "digest_equal": r2["digest"] == h["digest"]}
        except Exception as e:
            out.setdefault("errors", {})["native_rccl"] = repr(e)[:300]
        wd.disarm()

    # ---- BASELINE config 3 (all ranks) ----
    if not args.no_config3:
        wd.arm("config3", 300)
        try:
            # over the native RCCL communicator when it came up for the headline combine above
            c3_comm = "rccl" if (world > 1 and out.get("native_rccl", {}).get("digest_equal")) \
                else "host"
            c3 = bm.run_config3(N, world, rank, device, comm=c3_comm)
            if rank == 0:
                out["config3"] = c3
        except Exception as e:
            out.setdefault("errors", {})["config3"] = repr(e)[:300]
        wd.disarm()

    # ---- BASELINE config 5 (all ranks): 100M transactions x 1M items, the deployed rule map ----
    if not args.no_config5 and not args.cpu:
        wd.arm("config5", 600)
        try:
            from kubernetes_machine_learning_server_amd.bench.bench_large import run_rule_map
            t_c5 = time.time()
            serve_c5 = world == 1 and not args.no_config5_serve and bool(args.serve_qps)
            pvc_c5 = tempfile.mkdtemp(prefix="kmls_pvc_c5_") if serve_c5 and rank == 0 else ""
            c5 = run_rule_map("100Mx1M", min_support=2e-4, steps=args.config5_steps, warmup=1,
                              pvc_dir=pvc_c5)
            c5["section_wall_s"] = round(time.time() - t_c5, 1)
            if rank == 0:
                c5["model"] = "rule-map-100Mx1M-synthetic"
                c5["what"] = ("BASELINE config 5: 100M transactions x 1M items @2e-4 -> the "
                              "deployed artifact (rule map = pair supports, main.py:282-304), "
                              "timed step = supports + selection + pair counts + CSR per rank, "
                              "then rules.idx write + hot reload into the C++ and HBM indexes")
                out["config5"] = c5
        except Exception as e:
            out.setdefault("errors", {})["config5"] = repr(e)[:300]
        wd.disarm()
        # the config-5 index served at 10k QPS while the next job's index is hot-reloaded
        # under load (the marker-last publish, rest_api/app/main.py:106-122): the default
        # router and the persistent HIP serving kernel forced, each in a fresh server process
        if serve_c5 and rank == 0 and (out.get("config5") or {}).get("pvc"):
            wd.arm("config5_serve", 420)
            try:
                alt = os.path.join(pvc_c5, "rules_alt.idx")
                c5s = {}
                for be in ("auto", "loop"):
                    t = time.time()
                    c5s[be] = run_serve_child("10000", 3.0, be, timeout=200, capacity=False,
                                              extra=("--pvc", pvc_c5, "--reload-index", alt,
                                                     "--reload-at", "3", "--reload-duration",
                                                     "8"))
                    c5s[be]["wall_s"] = round(time.time() - t, 1)
                    # (the PVC's marker and index are now the alt ones: restore for the next)
                    if be == "auto":
                        from kubernetes_machine_learning_server_amd.utils.atomic_io import \
                            atomic_write_bytes
                        pk = os.path.join(pvc_c5, "api-data", "pickles")
                        with open(os.path.join(pvc_c5, "rules_main.idx"), "rb") as fh:
                            atomic_write_bytes(os.path.join(pk, "rules.idx"), fh.read())
                        atomic_write_bytes(os.path.join(pvc_c5, "api-data", "last_execution.txt"),
                                           b"initial")
                out["config5"]["serve_reload"] = c5s
            except Exception as e:
                out.setdefault("errors", {})["config5_serve"] = repr(e)[:300]
            wd.disarm()
        if pvc_c5:
            import shutil
            shutil.rmtree(pvc_c5, ignore_errors=True)

    # ---- config 3 item-sharded (every N: each rank counts the pair rows and horizontal
    #      levels of its own items over the all-gathered frequent-rank CSRs) ----
    if not args.no_config3 and not args.cpu:
        wd.arm("config3_shard", 300)
        try:
            c3s = bm.run_config3(N, world, rank, device, steps=3, warmup=1, mode="shard")
            if rank == 0:
                c3s["digest_equal_tx"] = c3s.get("digest") == out.get("config3", {}).get("digest")
                out["config3_shard"] = c3s
        except Exception as e:
            out.setdefault("errors", {})["config3_shard"] = repr(e)[:300]
        wd.disarm()

    # ---- config 5's data mined completely (all ranks: every frequent itemset of every size
    #      of 100M x 1M @2e-4, tx-DP like config 3) + confidence rules on rank 0 ----
    if not args.no_config5 and not args.cpu:
        wd.arm("config5_mine", 420)
        try:
            c5m = bm.run_config3(N, world, rank, device, steps=2, warmup=1,
                                 comm=("rccl" if (world > 1 and out.get("native_rccl", {})
                                                  .get("digest_equal")) else "host"),
                                 shape_name="100Mx1M", rules_min_confidence=0.1)
            if rank == 0:
                out["config5_mine"] = c5m
        except Exception as e:
            out.setdefault("errors", {})["config5_mine"] = repr(e)[:300]
        wd.disarm()

    # ---- config 3's data at 7e-5 (59,664 frequent items, N = 1): the sparse path past 32,768
    #      ranks (16-bit rank windows), reference min_support sweep downwards ----
    if not args.no_config3 and not args.cpu and world == 1:
        wd.arm("config3_wide", 300)
        try:
            out["config3_wide"] = bm.run_config3(N, world, rank, device, steps=2, warmup=1,
                                                 min_support=7e-5)
        except Exception as e:
            out.setdefault("errors", {})["config3_wide"] = repr(e)[:300]
        wd.disarm()

    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
