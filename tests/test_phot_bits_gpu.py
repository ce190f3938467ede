"""The bits of the photometric nets' kernels (sed_tile in the hidden-layer launch, payne_sed_kernel, payne_sedfit_jac,
payne_sedfit_run) on the MI355X, pinned: tests/golden/g25_phot_bits.npz holds the sha256 of every result of
tools/freeze_phot_bits_golden.py's case table, frozen from the library of the commit the fixture names (before the fp64 matrix tile of
the photometric nets and the rows' arithmetic were each written once: csrc/sed_tile.hpp, sed_core.hpp).  The same table runs here on
the tree's library through the public ABI and must give equal digests; the fixture's fp64 sums only make a failure readable.

The other GPU tests of these kernels hold the device to a long-double reference within a bound; this one holds the device to itself.
The kernels have no atomics and no order that depends on timing, so the bits are a property of the source and the compiler.  A
mismatch after a change of toolchain (the fixture records the ROCm version it was frozen with; the test prints both) means: re-freeze
from a known-good commit with the new toolchain.  A mismatch after an edit means: the edit changed the arithmetic."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from freeze_phot_bits_golden import CASES, case_id, run_case, sha_of, sum_of, tile_plan  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g25(golden):
    z = golden("g25_phot_bits")
    return {k: (s.tobytes(), v) for k, s, v in zip(z["keys"].tolist(), z["sha256"], z["sums"].tolist())}, str(z["parent_commit"]), \
        str(z["rocm_version"]), int(z["n_cu"])


def test_the_fixture_covers_the_table(g25):
    frozen, commit, rocm, n_cu = g25
    ids = {case_id(c) for c in CASES}
    assert len(ids) == len(CASES) and {k.split("::")[0] for k in frozen} == ids


def test_tile_cases_reach_every_row_tile_count(g25):
    """On this device the tile cases run sed_tile with 16, 32 and 48 candidates, each with a last tile whose live rows are no
    multiple of 16 -- and with the tile sizes the fixture was frozen at (a device with another CU count has other digests)."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    plan = tile_plan(n_cu)
    assert plan == tile_plan(g25[3]), (n_cu, g25[3])
    for want in (16, 32, 48):
        assert any(cb == want and ((B - 1) % cb + 1) % 16 != 0 for _, _, B, cb in plan), (want, n_cu, plan)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_the_frozen_commit(g25, case):
    import torch
    frozen, commit, rocm, _ = g25
    res = run_case(case)
    want = {k.split("::")[1]: v for k, v in frozen.items() if k.split("::")[0] == case_id(case)}
    assert sorted(res) == sorted(want)
    bad = ["%s: sum %.17g, frozen %.17g" % (name, sum_of(a), want[name][1]) for name, a in res.items() if sha_of(a) != want[name][0]]
    assert not bad, "bits differ from commit %s (frozen under ROCm %s, running %s): %s" % (commit, rocm, torch.version.hip, "; ".join(bad))
