"""The bits of the fit kernels (payne_lmfit_update, payne_lmfit_update_poly, payne_contfit_batch) on the MI355X, pinned:
tests/golden/g24_fit_bits.npz holds the sha256 of every result of tools/freeze_fit_bits_golden.py's case table, frozen from the
library of the commit the fixture names (before the normal-equations tile, the scaled solve and the Chebyshev series were each
written once: csrc/normal_tile.hpp, cheb_series.hpp).  The same table runs here on the tree's library through the public ABI and
must give equal digests; the fixture's fp64 sums only make a failure readable.

The other GPU tests of these kernels hold the device to the host emulators within a bound, since the order in which the matrix
instruction adds its four products is the hardware's; this one holds the device to itself.  The kernels have no atomics and no
order that depends on timing, so the bits are a property of the source and the compiler.  A mismatch after a change of toolchain
(the fixture records the ROCm version it was frozen with; the test prints both) means: re-freeze from a known-good commit with the
new toolchain.  A mismatch after an edit means: the edit changed the arithmetic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from freeze_fit_bits_golden import CASES, case_id, run_case, sha_of, sum_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g24(golden):
    z = golden("g24_fit_bits")
    return {k: (s.tobytes(), v) for k, s, v in zip(z["keys"].tolist(), z["sha256"], z["sums"].tolist())}, str(z["parent_commit"]), \
        str(z["rocm_version"])


@pytest.fixture(scope="module")
def lib():
    from thepayne_amd import _lib
    return _lib.load()


def test_the_fixture_covers_the_table(g24):
    frozen, commit, rocm = g24
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES) and {k.split("::")[0] for k in frozen} == ids


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_the_frozen_commit(lib, g24, case):
    import torch
    frozen, commit, rocm = g24
    res = run_case(lib, case)
    want = {k.split("::")[1]: v for k, v in frozen.items() if k.split("::")[0] == case_id(case)}
    assert sorted(res) == sorted(want)
    bad = ["%s: sum %.17g, frozen %.17g" % (name, sum_of(a), want[name][1]) for name, a in res.items() if sha_of(a) != want[name][0]]
    assert not bad, "bits differ from commit %s (frozen under ROCm %s, running %s): %s" % (commit, rocm, torch.version.hip, "; ".join(bad))
