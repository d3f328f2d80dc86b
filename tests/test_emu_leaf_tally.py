"""The leaf step's per-size tally (csrc/kernels/deep.hip leaf_step) on the CPU wave emulator.

The same sanitised stand-alone binary as tests/test_emu.py, in its clique mode (a negative item
count): every subset of every class survives, so each lane of a leaf pass adds to its packed
tally and the once-per-step sum over the lanes carries every size.  A clique of 12 at 64
transactions (blocks of one word) and at 130 (three words at the root, two below the half-support
item), with the hook ``deep_leaf_m`` at 6, 7 and the compiled maximum, and one run whose
``max_len`` cuts inside the leaf classes.  Every run must report ``"ok": true``: per-size counts
and content digest equal the CPU count miner's.
"""
import importlib.util
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _emu_suite():
    """tests/test_emu.py (its binary path and builder), loaded by path."""
    spec = importlib.util.spec_from_file_location("_kmls_test_emu", ROOT / "tests" / "test_emu.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# (arguments as in tests/test_emu.py)
TIER1 = "64 -12 1 1 1 0.5"
WIDER = "130 -12 1 1 1 0.5"
CAPPED = "130 -12 1 1 1 0.5 4 4 64 4 1 5"   # max_len 5

CASES = [(a, m) for a in (TIER1, WIDER) for m in (6, 7, 8)] + [(CAPPED, 8)]


@pytest.fixture(scope="module")
def emu_bin():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    suite = _emu_suite()
    suite._build()
    return suite.BIN


@pytest.mark.parametrize("args,leaf_m", CASES)
def test_leaf_tally_on_emulator(emu_bin, args, leaf_m):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", KMLS_TEST_HOOKS=f"deep_leaf_m={leaf_m}")
    r = subprocess.run([str(emu_bin)] + args.split(), capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert '"ok": true' in r.stdout, r.stdout[-2000:]
