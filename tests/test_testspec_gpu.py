"""Network validation on the MI355X: payne_mad_stats (csrc/k_mad.hip) through the ABI, bit for bit against np.median of the
fp64 residual, and Payne.testing.testspec.TestSpec on synthetic LinNet / SMLP files with a 65-row test set.  The cases and
the numpy expression are those of tests/test_testspec.py, where the same arithmetic runs on the host."""
import os

import numpy as np
import pytest

import oracle as O
from thepayne_amd import synth, nnio
from test_gpu_parity import FLUX_TOL
from test_testspec import MAD_N, MAD_P, PAD, GROUP_NAMES, mad_case, mad_groups, mad_reference, same_bits

pytestmark = pytest.mark.gpu


def _mad(lib, pred_d, truth_d, N, P, groups_d, G, rows=True, ld_pred=None, ld_truth=None, pix=None):
    """One payne_mad_stats call on device tensors -> (rc, pix_med [G][P], row_med [N] | None), outputs pre-filled with -1."""
    import torch
    pix_d = torch.full((max(G, 0), P), -1.0, dtype=torch.float64, device="cuda:0") if pix is None else pix
    row_d = torch.full((N,), -1.0, dtype=torch.float64, device="cuda:0") if rows else None
    rc = lib.payne_mad_stats(0, None if pred_d is None else pred_d.data_ptr(), pred_d.stride(0) if ld_pred is None else ld_pred,
                             None if truth_d is None else truth_d.data_ptr(), truth_d.stride(0) if ld_truth is None else ld_truth,
                             N, P, None if groups_d is None else groups_d.data_ptr(), G,
                             None if pix_d is None else pix_d.data_ptr(), None if row_d is None else row_d.data_ptr(), None)
    return rc, (None if pix_d is None else pix_d.cpu().numpy()), (row_d.cpu().numpy() if rows else None)


@pytest.mark.parametrize("N", MAD_N)
def test_mad_stats_is_np_median_to_the_bit(N):
    """N in {1, 2, 5, 64, 65, 257} x P in {1, 63, 64, 65, 300}, ld = P + 7 with NaN / 1e35 in the padding; row sets: all, empty
    (NaN), one row, alternate rows, an even and an odd scattered set; residuals over 1e-30 .. 1e+30, exact ties, exact zeros,
    columns that differ in the last bits, one NaN (NaN in its column for the sets that hold its row, and in its row, nowhere
    else), then a column that is all NaN.  Every median has the bits of np.median(np.abs(t.astype(f8) - p.astype(f8))[rows]);
    a second call returns the same bytes."""
    import torch
    from thepayne_amd import _lib
    lib = _lib.load()
    groups = mad_groups(N)
    groups_d = torch.as_tensor(groups).to("cuda:0")
    for P in MAD_P:
        for nan_column in (False, True):
            pred, truth = mad_case(N, P, nan_column)
            assert pred.shape == (N, P + PAD)
            ref_pix, ref_row = mad_reference(pred, truth, P, groups)
            pred_d, truth_d = torch.as_tensor(pred).to("cuda:0"), torch.as_tensor(truth).to("cuda:0")
            rc, pix, row = _mad(lib, pred_d, truth_d, N, P, groups_d, len(groups))
            assert rc == 0
            bad = np.argwhere((pix.view(np.uint64) != ref_pix.view(np.uint64)) & ~(np.isnan(pix) & np.isnan(ref_pix)))
            assert same_bits(pix, ref_pix), (N, P, nan_column, [(GROUP_NAMES[g], j) for g, j in bad[:5]])
            assert same_bits(row, ref_row), (N, P, nan_column)
            rc2, pix2, row2 = _mad(lib, pred_d, truth_d, N, P, groups_d, len(groups))
            assert rc2 == 0 and pix2.tobytes() == pix.tobytes() and row2.tobytes() == row.tobytes()
            if not nan_column:
                nan_pix = np.zeros((len(groups), P), dtype=bool)
                nan_pix[:, P // 2] = groups[:, N // 3] != 0
                nan_pix[~groups.astype(bool).any(axis=1)] = True
                assert np.array_equal(np.isnan(pix), nan_pix) and np.array_equal(np.flatnonzero(np.isnan(row)), [N // 3])
            else:
                assert np.all(np.isnan(pix[:, P // 3])) and np.all(np.isnan(row))


def test_mad_stats_row_medians_alone_and_column_medians_alone():
    import torch
    from thepayne_amd import _lib
    lib = _lib.load()
    N, P = 65, 300
    pred, truth = mad_case(N, P)
    groups = mad_groups(N)
    ref_pix, ref_row = mad_reference(pred, truth, P, groups)
    pred_d, truth_d, groups_d = (torch.as_tensor(a).to("cuda:0") for a in (pred, truth, groups))
    one = torch.full((1, 1), -1.0, dtype=torch.float64, device="cuda:0")
    rc, pix, row = _mad(lib, pred_d, truth_d, N, P, None, 0, pix=one)           # G == 0: row medians only
    assert rc == 0 and same_bits(row, ref_row) and pix[0, 0] == -1.0
    rc, pix, row = _mad(lib, pred_d, truth_d, N, P, groups_d, len(groups), rows=False)
    assert rc == 0 and row is None and same_bits(pix, ref_pix)
    # the two matrices may have different leading dimensions
    truth_wide = torch.full((N, P + 40), float("nan"), dtype=torch.float32, device="cuda:0")
    truth_wide[:, :P] = truth_d[:, :P]
    rc, pix, row = _mad(lib, pred_d, truth_wide, N, P, groups_d, len(groups))
    assert rc == 0 and same_bits(pix, ref_pix) and same_bits(row, ref_row)


def test_mad_stats_refuses_malformed_calls():
    """PAYNE_E_INVALID, and nothing written: null pred / truth / pix_med, N < 1, P < 1, ld < P (either matrix), G < 0, groups == NULL
    with G > 0."""
    import torch
    from thepayne_amd import _lib
    lib = _lib.load()
    N, P = 5, 63
    pred, truth = mad_case(N, P)
    groups = mad_groups(N)
    G = len(groups)
    pred_d, truth_d, groups_d = (torch.as_tensor(a).to("cuda:0") for a in (pred, truth, groups))
    pix_d = torch.full((G, P), -1.0, dtype=torch.float64, device="cuda:0")
    row_d = torch.full((N,), -1.0, dtype=torch.float64, device="cuda:0")

    def call(pred_=pred_d, truth_=truth_d, N_=N, P_=P, ldp=P + PAD, ldt=P + PAD, groups_=groups_d, G_=G, pix_=pix_d):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.payne_mad_stats(0, ptr(pred_), ldp, ptr(truth_), ldt, N_, P_, ptr(groups_), G_, ptr(pix_), row_d.data_ptr(), None)
    bad = dict(null_pred=call(pred_=None), null_truth=call(truth_=None), null_pix=call(pix_=None), no_rows=call(N_=0),
               no_pixels=call(P_=0), short_pred=call(ldp=P - 1), short_truth=call(ldt=P - 1), negative_sets=call(G_=-1),
               null_sets=call(groups_=None))
    assert all(rc == _lib.E_INVALID for rc in bad.values()), bad
    torch.cuda.synchronize()
    assert bool((pix_d == -1.0).all()) and bool((row_d == -1.0).all())
    assert call() == 0 and not bool((pix_d == -1.0).any()) and not bool((row_d == -1.0).any())


# -- the class -----------------------------------------------------------------------------------------------------------
N_TEST = 65


def _test_labels():
    """65 label rows inside the synthetic networks' range: every bin edge (6500, 4500; 4.0, 3.0; 0.0, -1.0; 0.3, 0.0) is the
    value of exactly one row, and no row has [a/Fe] > 0.3 (that bin is empty)."""
    rng = np.random.default_rng(65)
    lab = np.column_stack([rng.uniform(3600.0, 7900.0, N_TEST), rng.uniform(0.1, 5.4, N_TEST), rng.uniform(-2.4, 0.4, N_TEST),
                           rng.uniform(-0.19, 0.29, N_TEST)])
    for k, (col, edge) in enumerate([(0, 6500.0), (0, 4500.0), (1, 4.0), (1, 3.0), (2, 0.0), (2, -1.0), (3, 0.3), (3, 0.0)]):
        lab[3 * k + 1, col] = edge
    for col, edges in enumerate([(6500.0, 4500.0), (4.0, 3.0), (0.0, -1.0), (0.3, 0.0)]):
        assert all(np.sum(lab[:, col] == e) == 1 for e in edges)
    assert not np.any(lab[:, 3] > 0.3)
    return lab


@pytest.fixture(scope="module", params=["LinNet", "SMLP"])
def problem(request, tmp_path_factory):
    """(TestSpec on a synthetic file, raw network, labels, testpred, the numpy oracle's predictions for the labels)."""
    from Payne.testing.testspec import TestSpec
    kind = request.param
    raw = synth.make_torch_net(kind, npix=300, seed=11)
    forward = lambda lab: np.array([O.torchnet_forward(raw, x) for x in lab])
    net = synth.add_test_set(raw, forward, labels=_test_labels(), seed=5)
    path = str(tmp_path_factory.mktemp("testspec") / (kind + ".npz"))
    nnio.save_npz(path, net)
    T = TestSpec(path, NNtype=kind)
    return T, raw, net["testlabels"], net["testpred"], forward(net["testlabels"])


def _numpy_stats(pred, truth, labels):
    from thepayne_amd.testing.testspec import label_bins
    bins = label_bins(labels)
    groups = np.stack([np.ones(len(labels), dtype=bool)] + list(bins.values()))
    pix, row = mad_reference(np.asarray(pred, dtype=np.float32), np.asarray(truth, dtype=np.float32), pred.shape[1], groups)
    return pix, row, bins


def _check(st, pix, row, bins, same):
    assert list(st["bins"].keys()) == list(bins.keys()) and len(bins) == 12
    assert same(st["pixel_mad"], pix[0]) and same(st["spec_mad"], row)
    for k, (name, rows) in enumerate(bins.items()):
        assert np.array_equal(st["bins"][name]["rows"], rows), name
        assert same(st["bins"][name]["pixel_mad"], pix[1 + k]), name


def test_stats_is_the_numpy_expression_on_the_device_predictions(problem):
    """stats() against np.median(np.abs(testpred - NN.eval(testlabels))[rows], axis=...) bit for bit: per pixel, per spectrum and
    in all twelve bins (every edge value present once, '[a/Fe] > 0.3' empty -> NaN); attributes as the reference's."""
    T, raw, labels, testpred, _ = problem
    assert T.NN.testpred.dtype == np.float32 and np.array_equal(T.wave, raw["wavelength"]) and T.resolution == raw["resolution"]
    st = T.stats()
    pix, row, bins = _numpy_stats(T.NN.eval(labels), testpred, labels)
    assert np.array_equal(st["labels"], labels) and np.array_equal(st["wave"], raw["wavelength"])
    _check(st, pix, row, bins, same_bits)
    assert not bins["[a/Fe] > 0.3"].any() and np.all(np.isnan(st["bins"]["[a/Fe] > 0.3"]["pixel_mad"]))
    assert np.all(np.isfinite(st["pixel_mad"])) and np.all(np.isfinite(st["spec_mad"]))
    assert [int(b.sum()) for b in bins.values()].count(0) == 1
    assert T.stats()["pixel_mad"].tobytes() == st["pixel_mad"].tobytes()


def test_stats_on_drawn_rows_keeps_the_duplicates(problem):
    T, raw, labels, testpred, _ = problem
    ind = np.random.default_rng(3).integers(0, N_TEST, 10)
    st = T.stats(testnum=10, rng=np.random.default_rng(3))
    assert np.array_equal(st["labels"], labels[ind]) and st["spec_mad"].shape == (10,)
    pix, row, bins = _numpy_stats(T.NN.eval(labels[ind]), testpred[ind], labels[ind])
    _check(st, pix, row, bins, same_bits)
    # 25 draws from 65 rows with this seed repeat a row: a duplicate counts twice
    ind = np.random.default_rng(4).integers(0, N_TEST, 25)
    assert len(np.unique(ind)) < 25
    st = T.stats(testnum=25, rng=np.random.default_rng(4))
    pix, row, bins = _numpy_stats(T.NN.eval(labels[ind]), testpred[ind], labels[ind])
    _check(st, pix, row, bins, same_bits)


def test_stats_against_the_references_arithmetic(problem):
    """The forward pass from the numpy oracle (torch's fp32 arithmetic restated) instead of the GPU's: a median of absolute
    residuals cannot move by more than the largest change of any one residual, so every median agrees within FLUX_TOL, the bound
    tests/test_gpu_parity.py holds stage-0 spectra to; NaN (the empty bin) in the same places."""
    T, raw, labels, testpred, oracle_pred = problem
    st = T.stats()
    pix, row, bins = _numpy_stats(oracle_pred, testpred, labels)
    worst = [0.0]

    def close(a, b):
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            return False
        d = np.abs(a - b)[~np.isnan(a)]
        worst[0] = max(worst[0], d.max() if d.size else 0.0)
        return bool(np.all(d <= FLUX_TOL))
    print("largest |prediction - oracle| %.3g" % np.abs(T.NN.eval(labels).astype(np.float64) - oracle_pred).max())
    try:
        _check(st, pix, row, bins, close)
    finally:
        print("largest difference of a median from the oracle's: %.3g (bound %.3g)" % (worst[0], FLUX_TOL))


def test_report_returns_the_numbers_and_draws_where_it_can(problem, tmp_path, capsys):
    """The reference's entry point (TestSpec.report, also under the reference's own name)."""
    T = problem[0]
    out = str(tmp_path / "test.pdf")
    st = T.report(output=out, testnum=20, rng=np.random.default_rng(1))
    assert st["spec_mad"].shape == (20,) and st["pixel_mad"].shape == (300,) and len(st["bins"]) == 12
    said = capsys.readouterr().out
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert "matplotlib is not installed" in said and not os.path.exists(out)
    else:
        assert os.path.getsize(out) > 1000 and "skipped the C3K comparison pages" in said


def test_stats_names_the_sizes_when_the_matrices_do_not_fit(problem, monkeypatch):
    import torch
    T = problem[0]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (100000, 200000))
    with pytest.raises(ValueError, match=r"65 x 300 fp32"):
        T.stats()
