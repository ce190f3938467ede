"""Slice sampling with the chain on the device (payne_slice_begin / _rounds / _batch, DeviceProposer.slice_walk): invariants of a
walk, the numpy restatement replayed against the device to the bit, independence of how rounds are grouped into calls, the caps,
the error paths and a fit."""
import ctypes as C

import numpy as np
import pytest

from thepayne_amd import synth
from thepayne_amd.sampler.slice_ref import slice_walk_ref
from helpers import lnl_tol
from test_api_gpu import _fit_objects, _save_yst

pytestmark = pytest.mark.gpu

K = 64


class Problem(object):
    pass


@pytest.fixture(scope="module")
def prob(tmp_path_factory):
    """The small problem, a proposer, K start points and the threshold at their median lnprob; the reference walks of the tests
    below start from these arrays and leave them unchanged."""
    from thepayne_amd.sampler.device import DeviceProposer
    p = Problem()
    p.L, p.P, p.OL = _fit_objects(tmp_path_factory.mktemp("slice"), photscale=True)
    p.prop = DeviceProposer(p.L, p.P, k_max=K)
    p.nd = p.L.ndim
    p.U0 = np.random.default_rng(5).uniform(0.3, 0.7, size=(K, p.nd))
    p.V0, lp0 = p.prop.lnprob_u(p.U0)
    p.lp0 = np.where(np.isnan(lp0), -np.inf, lp0)
    p.lstar = float(np.median(p.lp0[np.isfinite(p.lp0)]))
    p.axes = 0.05 * np.eye(p.nd)
    for a in (p.U0, p.V0, p.lp0, p.axes):
        a.setflags(write=False)
    yield p
    p.prop.close()


def _walk(p, slices, random_dirs, seed, **kw):
    kw.setdefault("axes", p.axes)
    axes = kw.pop("axes")
    lstar = kw.pop("lstar", p.lstar)
    return p.prop.slice_walk(p.U0, p.V0, p.lp0, axes, 1.0, lstar, slices, random_dirs, seed, **kw)


@pytest.mark.parametrize("method,slices", [("slice", 2), ("rslice", 3)])
def test_device_slice_walk_invariants(prob, method, slices):
    from thepayne_amd.fitting.fitstar import lnprob_batch
    p, nd = prob, prob.nd
    rd = method == "rslice"
    n_dir = slices if rd else slices * nd
    U, V, lp, ncall, nexpand, ncontract, n_active = _walk(p, slices, rd, 1234)
    assert n_active == 0
    assert np.all((U > 0) & (U < 1))
    moved = np.any(U != p.U0, axis=1)
    print(method, "moved", int(moved.sum()), "calls", int(ncall.sum()), "expand", int(nexpand.sum()), "contract", int(ncontract.sum()))
    assert np.all(moved[p.lp0 > p.lstar])             # from a point above the threshold every direction ends in a new point
    assert np.all(lp[moved] > p.lstar)
    assert np.array_equal(V[~moved], p.V0[~moved]) and np.array_equal(lp[~moved], p.lp0[~moved])
    np.testing.assert_allclose(V, p.P.priortrans_batch(U), rtol=1e-11, atol=1e-11)
    host = lnprob_batch(V, p.L, p.P)
    assert np.all(np.abs(lp[moved] - host[moved]) <= 1e-9 * np.abs(host[moved]) + 1e-9)
    ref = np.array([p.OL.lnlikefn(t) for t in V[moved][:16]]) + p.P.lnprior_batch(V[moved][:16])
    assert np.all(np.abs(lp[moved][:16] - ref) <= lnl_tol(ref))
    assert np.array_equal(ncall, nexpand + ncontract)
    assert np.all(nexpand >= 2 * n_dir)
    assert np.all(ncontract >= n_dir)                  # every direction samples its window at least once, moved or not
    # the window around the old point is never longer than one axis length per sweep plus one per expansion
    assert np.all(np.abs(U - p.U0) <= 1.0 * np.diag(p.axes)[None, :] * (slices + nexpand)[:, None])
    again = _walk(p, slices, rd, 1234)
    assert all(np.array_equal(a, b) for a, b in zip(again[:6], (U, V, lp, ncall, nexpand, ncontract)))
    other = _walk(p, slices, rd, 99)
    assert not np.array_equal(other[0], U)


def _lnprob_u_of(prop):
    def f(U):
        V, lp = prop.lnprob_u(U)
        return V, lp
    return f


@pytest.mark.parametrize("n_ell", [1, 3])
def test_numpy_restatement_replays_the_device_walk(prob, n_ell):
    """The permutation, the windows, the side test, the out-of-cube shortcuts and the multi-ellipsoid indexing: slice_ref driven
    by the device's own lnprob_u gives the device's unit-cube points to the bit."""
    p, nd = prob, prob.nd
    rng = np.random.default_rng(13)
    A = np.stack([np.tril(rng.normal(size=(nd, nd))) * 0.01 + 0.02 * np.eye(nd),
                  rng.normal(size=(nd, nd)) * 0.004 + 0.01 * np.eye(nd),
                  np.triu(rng.normal(size=(nd, nd))) * 0.02 + np.diag(np.linspace(0.005, 0.2, nd))])
    ell = rng.integers(0, 3, size=K).astype(np.int32)
    axes, kw = (A, {"ell": ell}) if n_ell == 3 else (A[0], {})
    # start points near a face of the cube for a third of the chains: window ends and shrink points outside it
    U0 = p.U0.copy()
    U0[::3, 1] = 0.004
    U0[1::3, 2] = 0.997
    V0, lp0 = p.prop.lnprob_u(U0)
    lp0 = np.where(np.isnan(lp0), -np.inf, lp0)
    lstar = float(np.median(lp0[np.isfinite(lp0)]))
    dev = p.prop.slice_walk(U0, V0, lp0, axes, 1.3, lstar, 2, False, 777, **kw)
    ref = slice_walk_ref(_lnprob_u_of(p.prop), U0, V0, lp0, axes, 1.3, lstar, 2, False, 777, **kw)
    assert dev[6] == 0 and ref[6] == 0
    print("n_ell", n_ell, "calls", int(dev[3].sum()), "moved", int(np.any(dev[0] != U0, axis=1).sum()))
    assert np.array_equal(dev[0], ref[0])
    for j in (3, 4, 5):
        assert np.array_equal(dev[j], ref[j]), j
    np.testing.assert_allclose(dev[1], ref[1], rtol=1e-11, atol=1e-11)
    assert np.all(np.abs(dev[2] - ref[2]) <= 1e-9 * np.abs(ref[2]) + 1e-9)
    assert np.any(dev[0] != U0)


def test_grouping_of_rounds_does_not_matter(prob):
    p = prob
    base = _walk(p, 2, False, 31, chunk=1)
    assert base[6] == 0
    for chunk in (7, 64):
        got = _walk(p, 2, False, 31, chunk=chunk)
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), chunk
    p.prop.slice_begin(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 2, False, 31)
    pieces, n_active, i = (3, 1, 10, 2, 17, 5), K, 0
    while n_active > 0:
        n_active = p.prop.slice_rounds(pieces[i % len(pieces)])
        i += 1
    got = p.prop.slice_finish()
    assert i > 3
    assert all(np.array_equal(a, b) for a, b in zip(got, base[:6]))
    # ... nor does what was walked before: the random walk and the slice walk stage their chains through ONE set of buffers, and
    # rwalk, slice_walk, rwalk on one proposer give, array for array, what each call gives on a fresh proposer
    from thepayne_amd.sampler.device import DeviceProposer
    calls = (lambda q: q.rwalk(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 4, 101),
             lambda q: q.slice_walk(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 2, False, 102),
             lambda q: q.rwalk(p.U0, p.V0, p.lp0, p.axes, 0.7, p.lstar, 4, 103))
    mixed = [f(p.prop) for f in calls]
    for f, got in zip(calls, mixed):
        fresh = DeviceProposer(p.L, p.P, k_max=K)
        try:
            want = f(fresh)
        finally:
            fresh.close()
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.any(got[0] != p.U0)


def test_caps(prob):
    p = prob
    c0 = p.prop.step_counters()
    U, V, lp, ncall, nexpand, ncontract, n_active = _walk(p, 1, True, 7, lstar=np.inf)
    assert n_active == 0
    assert np.array_equal(U, p.U0) and np.array_equal(V, p.V0) and np.array_equal(lp, p.lp0)
    assert np.all(ncontract == 200) and np.all(nexpand == 2) and np.all(ncall == 202)   # (start points in [0.3, 0.7], axes 0.05: every end in the cube)
    c1 = p.prop.step_counters()
    assert c1[0] == c0[0] and c1[1] - c0[1] >= 202                                     # rounds are launches of their own
    U, V, lp, ncall, nexpand, ncontract, n_active = _walk(p, 2, False, 8, max_rounds=5)
    assert n_active > 0
    assert np.all(ncall <= 5 + 0) and np.array_equal(ncall, nexpand + ncontract)
    same = np.all(U == p.U0, axis=1)
    assert np.array_equal(lp[same], p.lp0[same]) and np.all(lp[~same] > p.lstar)
    assert p.prop.step_counters()[1] - c1[1] == 5


def test_error_paths(prob):
    from thepayne_amd import _lib
    p, nd = prob, prob.nd
    prop, lib = p.prop, p.prop.lib
    t = prop.torch
    rows = np.arange(K + 1) % K                                   # K + 1 valid chains (the last repeats the first)
    u = t.as_tensor(p.U0[rows].copy()).to(prop.eng.device)
    v = t.as_tensor(p.V0[rows].copy()).to(prop.eng.device)
    lp = t.as_tensor(p.lp0[rows].copy()).to(prop.eng.device)
    cnt = t.zeros(3 * (K + 1), dtype=t.int32, device=prop.eng.device)
    ax = np.ascontiguousarray(np.stack([p.axes, p.axes]))
    ell_ok = np.zeros(K, dtype=np.int32)
    ell_bad = ell_ok.copy()
    ell_bad[5] = 2
    t.cuda.synchronize()
    c0 = prop.step_counters()

    def begin(Kc=K, n_ell=1, ell=None, slices=2):
        return lib.payne_slice_begin(prop._handle, u.data_ptr(), v.data_ptr(), lp.data_ptr(), Kc, ax.ctypes.data, n_ell,
                                     None if ell is None else ell.ctypes.data, 1.0, p.lstar, slices, 0, 1,
                                     cnt.data_ptr(), cnt.data_ptr() + 4 * (K + 1), cnt.data_ptr() + 8 * (K + 1), None)

    def message():
        return lib.payne_last_error(prop.eng._ctx).decode()

    na = C.c_int(-1)
    assert lib.payne_slice_rounds(prop._handle, 4, C.byref(na)) == _lib.E_INVALID and "outside a walk" in message()
    assert begin(Kc=K + 1) == _lib.E_BATCH and message()
    assert begin(slices=0) == _lib.E_INVALID and "slices" in message()
    assert begin(n_ell=2, ell=ell_bad) == _lib.E_INVALID and "ellipsoid" in message()
    assert begin(n_ell=2, ell=None) == _lib.E_INVALID and message()
    assert begin(n_ell=_lib_max_ell() + 1, ell=ell_ok) == _lib.E_INVALID and message()
    assert lib.payne_slice_rounds(prop._handle, 4, C.byref(na)) == _lib.E_INVALID and na.value == -1    # none of them opened a walk
    # a random walk is open: the two share the pending proposal's buffers
    prop.rwalk_begin(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 2, 3)
    assert begin() == _lib.E_INVALID and "random walk" in message()
    with pytest.raises(RuntimeError):
        _walk(p, 2, False, 1)
    for w in range(3):
        prop.rwalk_step(w)
    prop.rwalk_finish()
    c1 = prop.step_counters()
    assert c1[0] + c1[1] - c0[0] - c0[1] == 3                     # the random walk's three steps and nothing else
    # ... and the other way round
    assert begin(n_ell=2, ell=ell_ok) == 0
    with pytest.raises(RuntimeError):
        prop.rwalk_begin(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 2, 3)
    assert lib.payne_slice_rounds(prop._handle, 0, C.byref(na)) == _lib.E_INVALID
    n = 1
    while n > 0:
        assert lib.payne_slice_rounds(prop._handle, 8, C.byref(na)) == 0
        n = na.value
    U, V, lpw, nacc, ncalls = prop.rwalk(p.U0, p.V0, p.lp0, p.axes, 1.0, p.lstar, 2, 3)     # the sampler is free again
    assert np.all((U > 0) & (U < 1))


def _lib_max_ell():
    from thepayne_amd.sampler.nested import MAX_ELL
    return MAX_ELL


def test_fitpayne_slice_sampling_with_the_chain_on_the_device(tmp_path):
    """sampler['slice_device']: the fit of test_fitpayne_slice_sampling_on_the_device with every queue one payne_slice_batch call,
    against the truth and against the host-driven loop on the same seed."""
    from thepayne_amd.fitting.fitstar import FitPayne
    from helpers import yst_problem
    raw, obs, flux, eflux = yst_problem("small", H=64, line_depth=0.3)
    out = {}
    for dev in (True, False):
        inputdict = {
            'spec': {'obs_wave': obs, 'obs_flux': flux, 'obs_eflux': eflux, 'convertair': False},
            'specANNpath': _save_yst(tmp_path, raw), 'NNtype': 'YST1',
            'sampler': {'samplertype': 'Static', 'samplerbounds': 'multi', 'samplemethod': 'slice', 'slices': 2,
                        'npoints': 100, 'delta_logz_final': 0.5, 'bootstrap': 0, 'flushnum': 500, 'seed': 6,
                        'slice_device': dev},
            'priordict': synth.demo_priordict(), 'output': str(tmp_path / ('fit%d.dat' % dev)),
        }
        F = FitPayne()
        sampler = F.run(inputdict=inputdict, verbose=False)
        assert F.proposer is not None and sampler.method == 'slice' and sampler.slice_device is dev
        r = sampler.results
        out[dev] = (float(r.logz[-1]), float(r.logzerr[-1]), F.proposer.step_counters(), sampler.ncall)
        if dev:
            w = sampler.posterior_weights()
            mean = (w[:, None] * r.samples).sum(0)
            std = np.sqrt((w[:, None] * (r.samples - mean) ** 2).sum(0))
            T = synth.TRUTH
            truth = np.array([T["Teff"], T["logg"], T["feh"], T["afe"], T["vrad"], T["vrot"], T["inst_R"]])
            assert np.all(np.abs(mean - truth) < 5 * std + 1e-3 * np.abs(truth)), (mean, std, truth)
    print("device", out[True], "host", out[False])
    (zd, ed, cd, _), (zh, eh, ch, _) = out[True], out[False]
    assert abs(zd - zh) <= 3 * np.hypot(ed, eh), (zd, ed, zh, eh)
    assert cd[1] > 1000 and cd[0] == 0 and ch[1] == 0              # the rounds: launches of their own; the host loop makes none
