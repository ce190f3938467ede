"""Payne.testing.testspec (network validation: medians of |testpred - prediction| along both axes) -- what runs without a GPU:
the import names, ANN(testing=True) reading the test set from an .npz, the label bins, and the selection arithmetic of the
median kernels (csrc/mad_core.hpp) executed on the host under ASan / UBSan, bit for bit against np.median.  The kernels
themselves and the class on the device: tests/test_testspec_gpu.py, which shares the cases built here."""
import os
import subprocess
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAD_N = (1, 2, 5, 64, 65, 257)
MAD_P = (1, 63, 64, 65, 300)
PAD = 7
GROUP_NAMES = ("all", "empty", "one row", "alternate", "even size", "odd size")


def mad_groups(N, seed=0):
    """uint8 [6][N]: all rows, none, one row, alternate rows, a scattered set of even size and one of odd size."""
    rng = np.random.default_rng(100 + seed)
    g = np.zeros((len(GROUP_NAMES), N), dtype=np.uint8)
    g[0] = 1
    g[2, N // 2] = 1
    g[3, ::2] = 1
    n_even, n_odd = 2 * ((N + 1) // 3), min(N, 2 * (N // 3) + 1)
    g[4, rng.permutation(N)[:n_even]] = 3                 # (any non-zero byte is membership)
    g[5, rng.permutation(N)[:n_odd]] = 255
    assert g[4].astype(bool).sum() % 2 == 0 and g[5].astype(bool).sum() % 2 == 1
    return g


def mad_case(N, P, nan_column=False, seed=0):
    """(pred, truth) fp32 [N][P + PAD] whose residuals reach every digit of the key.  Column j is of kind j % 6:
      0  |truth - pred| spanning 1e-30 .. 1e+30 (either sign on both sides);
      1  a handful of exactly representable values: many exact ties, exact zeros;
      2  truth == pred in most rows (residual +0, also from -0 and from x - x);
      3  truth = pred + k ulp of pred, k in 0..5;
      4  a network-like column: pred ~ 0.5 .. 1.1, truth = pred + 1e-3 noise;
      5  residuals that differ only in the last bits of the fp64 difference: truth = 2^20 + k / 8, pred = -c 2^-30.
    One NaN sits in truth at (row N // 3, column P // 2); with `nan_column`, pred's column P // 3 is NaN in every row.  The
    padding beyond P holds NaN (truth) and +-1e35 (pred): read as data it would change every row median."""
    rng = np.random.default_rng(1000 * N + P + seed)
    ld = P + PAD
    pred = rng.uniform(0.5, 1.1, (N, ld)).astype(np.float32)
    truth = pred.copy()
    for j in range(P):
        kind = j % 6
        if kind == 0:
            pred[:, j] = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-30, 30, N)
            truth[:, j] = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-30, 30, N)
        elif kind == 1:
            pred[:, j] = rng.choice([0.5, 0.75, 1.0], N)
            truth[:, j] = pred[:, j] + rng.choice([0.0, 0.25, 0.5, -0.25], N).astype(np.float32)
        elif kind == 2:
            pred[:, j] = rng.choice([0.0, -0.0, 1.0, 3.5], N)
            truth[:, j] = np.where(rng.random(N) < 0.8, np.abs(pred[:, j]), pred[:, j] + np.float32(1e-3))
        elif kind == 3:
            t = pred[:, j].copy()
            for _ in range(5):
                step = rng.random(N) < 0.5
                t[step] = np.nextafter(t[step], np.float32(2.0))
            truth[:, j] = t
        elif kind == 4:
            truth[:, j] = pred[:, j] + rng.normal(0, 1e-3, N).astype(np.float32)
        else:
            pred[:, j] = -rng.integers(0, 8, N).astype(np.float32) * np.float32(2.0 ** -30)
            truth[:, j] = np.float32(2.0 ** 20) + rng.integers(0, 4, N).astype(np.float32) / np.float32(8.0)
    truth[N // 3, P // 2] = np.nan
    if nan_column:
        pred[:, P // 3] = np.nan
    truth[:, P:] = np.nan
    pred[:, P:] = np.where(rng.random((N, PAD)) < 0.5, np.float32(1e35), np.float32(-1e35))
    return pred, truth


def mad_reference(pred, truth, P, groups):
    """The numpy expression payne_mad_stats replaces: (pix_med [G][P], row_med [N])."""
    r = np.abs(truth[:, :P].astype(np.float64) - pred[:, :P].astype(np.float64))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        pix = np.stack([np.median(r[g.astype(bool)], axis=0) for g in groups]) if len(groups) else np.empty((0, P))
        row = np.median(r, axis=1)
    return pix, row


def same_bits(a, b):
    """The same 64 bits in every element, and NaN exactly where the other is NaN.  (Which NaN is not compared: numpy's median of an
    empty set is its mean, 0 / 0, whose sign is the host's -- the quiet NaN of x86 is negative, that of |NaN| positive.)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)])


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/mad_emul.cpp built with the sanitizers; returns run(pred, truth, P, groups, rows) -> (pix_med, row_med)."""
    build = tmp_path_factory.mktemp("mad_emul")
    exe = str(build / "mad_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "mad_emul.cpp")],
                   check=True)
    count = [0]

    def run(pred, truth, P, groups, rows=True):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        for name, a in (("pred", pred), ("truth", truth), ("groups", groups)):
            np.ascontiguousarray(a).tofile(str(d / (name + ".bin")))
        N, G = pred.shape[0], len(groups)
        res = subprocess.run([exe, str(d)] + [str(v) for v in (N, P, pred.shape[1], truth.shape[1], G, int(rows))],
                             capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        pix = np.fromfile(str(d / "pix_med.bin")).reshape(G, P)
        return pix, (np.fromfile(str(d / "row_med.bin")) if rows else None)
    return run


def test_reference_import_names_resolve_to_this_build():
    import Payne
    from Payne.testing import testspec
    from Payne.testing.testspec import TestSpec
    import thepayne_amd.testing.testspec as ts
    assert testspec is ts and TestSpec is ts.TestSpec and Payne.testing.testspec is ts
    assert TestSpec.__module__ == "thepayne_amd.testing.testspec"
    import inspect
    sig = inspect.signature(TestSpec.__init__)
    assert list(sig.parameters)[1:] == ["NNfilename", "NNtype", "c3kpath", "ystnn", "MISTpath", "continuum", "flux", "window1", "window2"]
    assert sig.parameters["NNtype"].default == "LinNet" and sig.parameters["window1"].default == [5150, 5200]
    assert vars(TestSpec)["runtest"] is vars(TestSpec)["report"]          # the reference's name for the report
    assert list(inspect.signature(TestSpec.report).parameters)[1:3] == ["output", "testnum"]


def test_ann_reads_the_test_set_only_when_asked(tmp_path, monkeypatch):
    """ANN(testing=True) exposes testlabels / testpred / testmedflux from an .npz (predictspec.py:51-54); without it nothing
    changes; a file without a test set is a KeyError.  (The device context is replaced by a stand-in: no GPU here.)"""
    from thepayne_amd import synth, nnio
    from thepayne_amd.predict import _spec, predictspec

    class NoEngine(object):
        def __init__(self, net, **kwargs):
            self.n_labels = net["layers"][0][0].shape[1]
    monkeypatch.setattr(_spec, "PayneEngine", NoEngine)
    raw = synth.make_torch_net("LinNet", npix=96, seed=2)
    net = synth.add_test_set(raw, lambda lab: np.full((len(lab), 96), 0.9), n=7, seed=4)
    assert net["testlabels"].shape == (7, 4) and net["testpred"].shape == (7, 96) and net["testpred"].dtype == np.float32
    assert np.all(net["testlabels"] >= raw["xmin"]) and np.all(net["testlabels"] <= raw["xmax"])
    assert 1e-4 < np.abs(net["testpred"] - np.float32(0.9)).mean() < 1e-2 and "testlabels" not in raw
    with pytest.raises(ValueError):
        synth.add_test_set(raw, lambda lab: np.zeros((1, 96)), labels=[[9000.0, 4.0, 0.0, 0.0]])
    net["testpred_medflux"] = np.arange(7.0)
    path = str(tmp_path / "nn.npz")
    nnio.save_npz(path, net)
    A = predictspec.ANN(nnpath=path, NNtype="LinNet", testing=True, verbose=True)
    assert A.nnpath == path and A.inlabels == ['teff', 'logg', 'feh', 'afe']
    assert np.array_equal(A.testlabels, net["testlabels"]) and np.array_equal(A.testpred, net["testpred"])
    assert np.array_equal(A.testmedflux, net["testpred_medflux"]) and np.array_equal(A.wavelength, raw["wavelength"])
    B = predictspec.ANN(nnpath=path, NNtype="LinNet")
    assert not any(hasattr(B, k) for k in ("testlabels", "testpred", "testmedflux"))
    del net["testpred_medflux"]
    assert not hasattr(predictspec.ANN(nnpath=net, testing=True), "testmedflux")
    bare = str(tmp_path / "bare.npz")
    nnio.save_npz(bare, raw)
    with pytest.raises(KeyError, match="testlabels"):
        predictspec.ANN(nnpath=bare, testing=True)


def test_label_bins_are_the_references_twelve():
    """testspec.py:125-208: three bins per label, '>' on the upper bin, '<=' closing the others; a value on an edge falls in
    the bin below it; every row is in exactly one bin of each label."""
    from thepayne_amd.testing.testspec import label_bins
    lab = np.array([[6500.0, 4.0, 0.0, 0.3], [6500.1, 4.01, 0.01, 0.31], [4500.0, 3.0, -1.0, 0.0], [4500.5, 3.5, -0.5, 0.1],
                    [3000.0, 1.0, -2.0, -0.1]])
    b = label_bins(lab)
    assert len(b) == 12
    got = np.array([v for v in b.values()]).astype(int)
    want = np.array([[0, 1, 0, 0, 0], [1, 0, 0, 1, 0], [0, 0, 1, 0, 1]] * 4)
    assert np.array_equal(got, want)
    assert np.all(got.reshape(4, 3, 5).sum(axis=1) == 1)


@pytest.mark.parametrize("N", MAD_N)
def test_selection_arithmetic_on_the_host(emul, N):
    """mad_core.hpp's radix selection, wave by wave in the kernels' order, against np.median of the fp64 residual: the same
    bits for every column of every row set and every row, for every P of the device test; NaN exactly where a member is NaN
    (and for the empty set); the padding beyond P is not touched."""
    groups = mad_groups(N)
    for P in MAD_P:
        for nan_column in (False, True):
            pred, truth = mad_case(N, P, nan_column)
            ref_pix, ref_row = mad_reference(pred, truth, P, groups)
            pix, row = emul(pred, truth, P, groups)
            assert same_bits(pix, ref_pix), (N, P, nan_column, np.argwhere(pix.view(np.uint64) != ref_pix.view(np.uint64))[:5])
            assert same_bits(row, ref_row), (N, P, nan_column)
            if not nan_column:                      # the single NaN: there and only there
                nan_pix = np.zeros((len(groups), P), dtype=bool)
                nan_pix[:, P // 2] = groups[:, N // 3] != 0
                nan_pix[~groups.astype(bool).any(axis=1)] = True           # (the empty set; for N = 1 also the even one)
                assert np.array_equal(np.isnan(pix), nan_pix) and np.array_equal(np.flatnonzero(np.isnan(row)), [N // 3])
            else:
                assert np.all(np.isnan(pix[:, P // 3])) and np.all(np.isnan(row))


def test_selection_without_row_sets_and_without_rows(emul):
    pred, truth = mad_case(5, 65)
    pix, row = emul(pred, truth, 65, np.zeros((0, 5), dtype=np.uint8))
    assert pix.shape == (0, 65) and same_bits(row, mad_reference(pred, truth, 65, [])[1])
    pix, row = emul(pred, truth, 65, mad_groups(5), rows=False)
    assert row is None and same_bits(pix, mad_reference(pred, truth, 65, mad_groups(5))[0])
