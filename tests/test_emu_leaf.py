"""The deep miner's leaf step (csrc/kernels/deep.hip leaf_step) on the CPU wave emulator.

The same sanitised stand-alone binary as tests/test_emu.py (g++, AddressSanitizer + UBSan, the
kernel's own source against the emulator's HIP shim), with the test hook ``deep_leaf_m`` at 0
(row / batch steps only), 2, 3, the default and the compiled maximum.  Every run must report
``"ok": true``: per-size counts and content digest equal the CPU count miner's.

An emulator run spends its time in the lane threads' barriers, a few cores at most, so the runs
of this module are started together (a small pool) the first time one is asked for and each test
looks at its own; under pytest-xdist every worker runs only the cases it is given.
"""
import concurrent.futures as cf
import importlib.util
import json
import os
import pathlib
import re
import shutil
import subprocess
import threading

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _emu_suite():
    """tests/test_emu.py (its binary path and builder), loaded by path."""
    spec = importlib.util.spec_from_file_location("_kmls_test_emu", ROOT / "tests" / "test_emu.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _constant(path, name):
    m = re.search(rf"constexpr int {name} = (\d+);", (ROOT / path).read_text())
    assert m, (path, name)
    return int(m.group(1))


LEAF_DEFAULT = _constant("csrc/include/kmls/gpu.hpp", "kDeepLeafDefault")
LEAF_MAX = _constant("csrc/kernels/deep.hip", "kLeafMax")
LEAF_MS = sorted({0, 2, 3, LEAF_DEFAULT, LEAF_MAX})

# (arguments as in tests/test_emu.py)
CASES = [
    "64 -13 1 1 1 0.5 1 2 8 4 1 0 1 2",              # clique: every subset frequent, partner
                                                     # hand-offs while leaf frames sit on the stack
    "400 60 20 3 0.9 0.05",                          # subsets that fail inside a leaf class
    "300 50 25 2 0.95 0.08 4 4 64 1 1 4",            # max_len 4 cuts inside a leaf
    "1500 60 16 3 0.9 0.06 2 2 4 4 1 0 1 0",         # several width tiers
    "300 50 25 2 0.95 0.08 1 1 4 1 3 0 1 0",         # 3 ranks, eager spills
]
EMIT = "400 60 20 3 0.9 0.05 1 1 2 4 1 0 1 1 16 1"   # emit: the node arena's own digest
EMIT_PLAIN = "400 60 20 3 0.9 0.05"                  # the same data, count-only


class _Runs:
    """The module's emulator runs: (args, leaf_m) -> CompletedProcess, each run once."""

    def __init__(self, binary):
        self.binary = binary
        self.lock = threading.Lock()
        self.futures = {}
        workers = max(1, min(4, (os.cpu_count() or 2) // 2))
        self.pool = cf.ThreadPoolExecutor(max_workers=workers)

    def _run(self, args, leaf_m):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0",
                   KMLS_TEST_HOOKS=f"deep_leaf_m={leaf_m}")
        return subprocess.run([str(self.binary)] + args.split(), capture_output=True, text=True,
                              timeout=900, env=env)

    def _submit(self, key):
        with self.lock:
            if key not in self.futures:
                self.futures[key] = self.pool.submit(self._run, *key)
            return self.futures[key]

    def get(self, args, leaf_m):
        if "PYTEST_XDIST_WORKER" not in os.environ:
            # the one process runs every case: start them all, the longest (3 ranks) first
            for a in reversed(CASES):
                for m in LEAF_MS:
                    self._submit((a, m))
            self._submit((EMIT, LEAF_MAX))
        r = self._submit((args, leaf_m)).result()
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert '"ok": true' in r.stdout
        return json.loads(r.stdout)


@pytest.fixture(scope="module")
def runs():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    suite = _emu_suite()
    suite._build()
    r = _Runs(suite.BIN)
    yield r
    r.pool.shutdown(wait=True, cancel_futures=True)


def test_leaf_constants():
    assert 4 <= LEAF_DEFAULT <= LEAF_MAX == 8


@pytest.mark.parametrize("leaf_m", LEAF_MS)
@pytest.mark.parametrize("args", CASES)
def test_leaf_step_on_emulator(runs, args, leaf_m):
    runs.get(args, leaf_m)


def test_leaf_hook_leaves_emit_alone(runs):
    """Emit mode ignores the hook: with it at its maximum the arena's own digest and counts
    match the CPU miner's (the binary's ``ok``), and the result is the one the same data gives
    with the hook at 0."""
    got, want = runs.get(EMIT, LEAF_MAX), runs.get(EMIT_PLAIN, 0)
    for key in ("F", "n_cpu", "per_level", "cpu"):
        assert got[key] == want[key], key
