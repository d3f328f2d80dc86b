"""The closed / maximal flag kernel's own source (csrc/kernels/closed.hip, with rules.hip's hash
build for the host trie's widths) runs on the CPU wave emulator (csrc/emu) under AddressSanitizer
and UBSan: a stand-alone program (csrc/tests/closed_emu_main.cpp) mines small datasets with a host
tid-list loop and checks every flag, in all three width sets, against the transaction-based
definition computed in the same program."""
import fcntl
import json
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
BIN = ROOT / "build" / "emu" / "closed_emu"


def _build():
    srcs = [ROOT / "csrc/kernels/closed.hip", ROOT / "csrc/kernels/rules.hip"]
    main = ROOT / "csrc/tests/closed_emu_main.cpp"
    deps = srcs + [main] + list((ROOT / "csrc/emu").rglob("*")) + \
        list((ROOT / "csrc/include").rglob("*.hpp")) + \
        [ROOT / "csrc/kernels/kernels.hpp", ROOT / "csrc/kernels/trie_hash.hpp"]
    newest = max(p.stat().st_mtime for p in deps if p.is_file())
    if BIN.exists() and BIN.stat().st_mtime >= newest:
        return
    BIN.parent.mkdir(parents=True, exist_ok=True)
    with open(BIN.parent / ".build_closed.lock", "w") as lk:
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
def closed_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    _build()
    return BIN


def _run(closed_bin, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([str(closed_bin)] + args.split(), capture_output=True, text=True,
                       timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_closed_clique_on_emulator(closed_bin):
    # 10 items, every count comparison a tie: singletons closed, the 10-set closed and maximal
    out = _run(closed_bin, "clique 10")
    assert out == {"itemsets": 1023, "closed": 11, "maximal": 1, "max_depth": 10, "bad": 0}, out


def test_closed_random_on_emulator(closed_bin):
    # n_tx n_items seed min_count
    out = _run(closed_bin, "random 300 30 1 6")
    assert out["bad"] == 0 and out["itemsets"] > 1000 and out["max_depth"] >= 5, out
    assert 0 < out["maximal"] < out["closed"] < out["itemsets"], out


def test_closed_missing_subset_on_emulator(closed_bin):
    assert _run(closed_bin, "missing")["bad"] == 0
