"""The bits of the four MLP kernel families (payne_lnmlp_eval, payne_lnmlp_train_*, payne_specmlp_train_*, payne_specjac_eval) on
the MI355X, pinned: tests/golden/g21_mlp_bits.npz holds the sha256 of every result of tools/freeze_mlp_bits_golden.py's case
table, frozen from the library of the commit the fixture names (before the matrix product, the training tail and the entry
points of these families were each written once: csrc/mlp_tile.hpp, mlp_train_tail.hpp, mlp_api.hip).  The same table runs here
on the tree's library through the public ABI and must give equal digests; the fixture's fp64 sums only make a failure readable.

These kernels have no atomics and no order that depends on timing, so the bits are a property of the source and the compiler.
A mismatch after a change of toolchain (the fixture records the ROCm version it was frozen with; the test prints both) means:
re-freeze from a known-good commit with the new toolchain.  A mismatch after an edit means: the edit changed the arithmetic."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from freeze_mlp_bits_golden import CASES, case_id, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21(golden):
    z = golden("g21_mlp_bits")
    return {k: (s, v) for k, s, v in zip(z["keys"].tolist(), z["sha256"].tolist(), z["sums"].tolist())}, str(z["parent_commit"]), \
        str(z["rocm_version"])


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def test_the_fixture_covers_the_table(g21):
    frozen, commit, rocm = g21
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES) and {k.split("::")[0] for k in frozen} == ids


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_the_frozen_commit(lib, g21, case):
    import torch
    frozen, commit, rocm = g21
    res = run_case(lib, case)
    want = {k.split("::")[1]: v for k, v in frozen.items() if k.split("::")[0] == case_id(case)}
    assert sorted(res) == sorted(want)
    bad = []
    for name, a in res.items():
        sha = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        if sha != want[name][0]:
            bad.append("%s: sum %.17g, frozen %.17g" % (name, float(np.sum(a, dtype=np.float64)), want[name][1]))
    assert not bad, "bits differ from commit %s (frozen under ROCm %s, running %s): %s" % (commit, rocm, torch.version.hip, "; ".join(bad))
