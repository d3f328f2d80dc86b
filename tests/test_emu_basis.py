"""The generator variant of the flag kernel, k_closure_resolve and the rule kernel with its basis
filter (csrc/kernels/closed.hip, rules.hip) run on the CPU wave emulator (csrc/emu) under
AddressSanitizer and UBSan: a stand-alone program (csrc/tests/basis_emu_main.cpp) mines small
datasets with a host tid-list loop and checks the three-bit flags and closure ids in all three
width sets, and the rule arrays of both passes of k_rules (the min-max basis; on the clique also
every rule, and both at a second threshold) in the host trie's widths, against definitions
computed in the same program."""
import fcntl
import json
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
BIN = ROOT / "build" / "emu" / "basis_emu"


def _build():
    srcs = [ROOT / "csrc/kernels/closed.hip", ROOT / "csrc/kernels/rules.hip"]
    main = ROOT / "csrc/tests/basis_emu_main.cpp"
    deps = srcs + [main] + list((ROOT / "csrc/emu").rglob("*")) + \
        list((ROOT / "csrc/include").rglob("*.hpp")) + \
        [ROOT / "csrc/kernels/kernels.hpp", ROOT / "csrc/kernels/trie_hash.hpp"]
    newest = max(p.stat().st_mtime for p in deps if p.is_file())
    if BIN.exists() and BIN.stat().st_mtime >= newest:
        return
    BIN.parent.mkdir(parents=True, exist_ok=True)
    with open(BIN.parent / ".build_basis.lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if BIN.exists() and BIN.stat().st_mtime >= newest:
            return
        tmp = BIN.with_name(f"{BIN.name}.{os.getpid()}.tmp")
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
               "-fno-omit-frame-pointer", f"-I{ROOT / 'csrc/emu'}", f"-I{ROOT / 'csrc/include'}",
               "-x", "c++"] + [str(s) for s in srcs] + ["-x", "none", str(main), "-lpthread",
                                                        "-o", str(tmp)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        os.replace(tmp, BIN)


@pytest.fixture(scope="module")
def basis_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    _build()
    return BIN


def _run(basis_bin, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([str(basis_bin)] + args.split(), capture_output=True, text=True,
                       timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_basis_clique_on_emulator(basis_bin):
    # 10 items, every count comparison a tie: generators are the 10 singletons and 45 pairs, the
    # only closed itemset of two or more items is the 10-set
    out = _run(basis_bin, "clique 10")
    assert out == {"itemsets": 1023, "closed": 11, "generators": 55, "max_depth": 10,
                   "basis_rules": 55, "exact_rules": 45, "all_rules": 57002, "bad": 0}, out


def test_basis_random_on_emulator(basis_bin):
    # n_tx n_items seed min_count, plus one duplicated and one AND-ed column
    out = _run(basis_bin, "random 300 30 1 6")
    assert out["bad"] == 0 and out["itemsets"] > 1000 and out["max_depth"] >= 5, out
    assert 0 < out["closed"] < out["itemsets"] and 0 < out["generators"] < out["itemsets"], out
    assert 0 < out["exact_rules"] < out["basis_rules"], out


def test_basis_missing_subset_on_emulator(basis_bin):
    assert _run(basis_bin, "missing")["bad"] == 0
