"""The bits of the forward pass as csrc/payne_hip.hip's host code wires it up (run_net: the first launch with its riders -- records,
photometric tiles --, the hidden layers on fp16 pairs, in fp32 or as one chain launch, the two-layer net, the continuum network), on
the MI355X, pinned: tests/golden/g23_forward_bits.npz holds the sha256 of every result of tools/freeze_forward_bits_golden.py's case
table, frozen from the library of the commit the fixture names (before the operands became values of the context and run_net a
sequence of named steps).  The same table runs here on the tree's library through the public ABI and must give equal digests -- and
every call must have launched the kernels its case names (kernels_used(): hidden, out, sed).  tests/test_out_bits_gpu.py does the same
for the output layer's kernels.  The fixture's fp64 sums only make a failure readable.

These launches have no atomics and no order that depends on timing within one process (the freeze was run twice: equal digests), so
the bits are a property of the source and the compiler.  A mismatch after a change of toolchain (the fixture records the ROCm version
it was frozen with; the test prints both) means: re-freeze from a known-good commit with the new toolchain.  A mismatch after an edit
means: the edit changed what a kernel is handed."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from freeze_forward_bits_golden import CASES, case_id, run_case  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g23(golden):
    z = golden("g23_forward_bits")
    return {k: (s, v) for k, s, v in zip(z["keys"].tolist(), z["sha256"].tolist(), z["sums"].tolist())}, str(z["parent_commit"]), \
        str(z["rocm_version"])


def test_the_fixture_covers_the_table(g23):
    frozen, commit, rocm = g23
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES) and {k.split("::")[0] for k in frozen} == ids


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_the_frozen_commit(g23, case):
    import torch
    frozen, commit, rocm = g23
    res, kernels = run_case(case)
    for key, (got, want) in kernels.items():
        assert got == want, (key, got, want)
    want = {k.split("::")[1]: v for k, v in frozen.items() if k.split("::")[0] == case_id(case)}
    assert sorted(res) == sorted(want)
    bad = []
    for name, a in res.items():
        sha = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        if sha != want[name][0]:
            bad.append("%s: sum %.17g, frozen %.17g" % (name, float(np.nansum(a, dtype=np.float64)), want[name][1]))
    assert not bad, "bits differ from commit %s (frozen under ROCm %s, running %s): %s" % (commit, rocm, torch.version.hip, "; ".join(bad))
