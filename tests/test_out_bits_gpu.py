"""The bits of the output layer's kernels (payne_dense_dma2h / dma2hh / dma3 / dma3f / big3 / dma_kernel: csrc/dense_kernels.hpp on
the shared pieces of csrc/out_tile.hpp) on the MI355X, pinned: tests/golden/g22_out_bits.npz holds the sha256 of every result of
tools/freeze_out_bits_golden.py's case table, frozen from the library of the commit the fixture names (before the kernels' prologue,
fragments, products, k-loop and epilogue were each written once).  The same table runs here on the tree's library through the public
ABI and must give equal digests -- and every case must have run the kernel it is meant for (kernels_used()["out"]): a fall-back
would otherwise hide a kernel.  The fixture's fp64 sums only make a failure readable.

These kernels have no atomics and no order that depends on timing, so the bits are a property of the source and the compiler.
A mismatch after a change of toolchain (the fixture records the ROCm version it was frozen with; the test prints both) means:
re-freeze from a known-good commit with the new toolchain.  A mismatch after an edit means: the edit changed the arithmetic."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from freeze_out_bits_golden import CASES, case_id, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g22(golden):
    z = golden("g22_out_bits")
    return {k: (s, v) for k, s, v in zip(z["keys"].tolist(), z["sha256"].tolist(), z["sums"].tolist())}, str(z["parent_commit"]), \
        str(z["rocm_version"])


def test_the_fixture_covers_the_table(g22):
    frozen, commit, rocm = g22
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES) and {k.split("::")[0] for k in frozen} == ids


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_the_frozen_commit(g22, case):
    import torch
    frozen, commit, rocm = g22
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ran = run_case(case, n_cu=n_cu)
    if ran is None:
        pytest.skip("%d tiles of 64 x 128 do not exceed this device's %d compute units: every tile gets one to itself" % (case[1]["tiles"], n_cu))
    res, kernels = ran
    for label, (got, want) in kernels.items():
        assert got == want, (label, got, want)
    want = {k.split("::")[1]: v for k, v in frozen.items() if k.split("::")[0] == case_id(case)}
    assert sorted(res) == sorted(want)
    bad = []
    for name, a in res.items():
        sha = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        if sha != want[name][0]:
            bad.append("%s: sum %.17g, frozen %.17g" % (name, float(np.nansum(a, dtype=np.float64)), want[name][1]))
    assert not bad, "bits differ from commit %s (frozen under ROCm %s, running %s): %s" % (commit, rocm, torch.version.hip, "; ".join(bad))
