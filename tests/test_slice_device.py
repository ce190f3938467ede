"""Slice sampling as the device runs it (payne_slice_*), on analytic problems and without a GPU: the numpy restatement of the
device chain (thepayne_amd/sampler/slice_ref.py) is a correct slice sampler, and NestedSampler(slice_device=True) hands its
queues to the proposer's slice_walk."""
import numpy as np
import pytest

from thepayne_amd.sampler import NestedSampler
from thepayne_amd.sampler.slice_ref import slice_walk_ref

# a correlated Gaussian in five dimensions, well inside the unit cube
ND = 5
_rng0 = np.random.default_rng(3)
_Q = np.linalg.qr(_rng0.normal(size=(ND, ND)))[0]
COV = (_Q * np.array([0.10, 0.08, 0.06, 0.05, 0.04]) ** 2) @ _Q.T
CHOL = np.linalg.cholesky(COV)
CINV = np.linalg.inv(COV)
R2_MEDIAN = 4.351460191095526                      # median of chi^2 with 5 degrees of freedom: the Gaussian's median density level
LSTAR = -0.5 * R2_MEDIAN


def lnprob_gauss(U):
    d = np.atleast_2d(U) - 0.5
    return -0.5 * np.einsum('ki,ij,kj->k', d, CINV, d)


def lnprob_u_gauss(U):
    return np.array(U, dtype=np.float64), lnprob_gauss(U)


def region_samples(rng, n):
    """n points uniform in {lnprob > LSTAR} by rejection from the enlarged ellipsoid."""
    out = []
    have = 0
    while have < n:
        z = rng.standard_normal((2 * n, ND))
        z *= (rng.uniform(size=(2 * n, 1)) ** (1.0 / ND)) / np.linalg.norm(z, axis=1)[:, None]
        U = 0.5 + 1.15 * np.sqrt(R2_MEDIAN) * z @ CHOL.T
        U = U[lnprob_gauss(U) > LSTAR]
        out.append(U)
        have += len(U)
    U = np.concatenate(out)[:n]
    assert np.all((U > 0) & (U < 1))
    return U


@pytest.fixture(scope="module")
def fresh():
    return region_samples(np.random.default_rng(101), 200000)


@pytest.mark.parametrize("method", ["slice", "rslice"])
def test_reference_chain_leaves_the_uniform_distribution_alone(method, fresh):
    K, slices = 4000, 3
    U0 = region_samples(np.random.default_rng(7), K)
    lp0 = lnprob_gauss(U0)
    axes = CHOL * np.sqrt(R2_MEDIAN)               # columns = axes of the region's own ellipsoid
    U, V, lp, ncall, nexpand, ncontract, n_active = slice_walk_ref(
        lnprob_u_gauss, U0, U0, lp0, axes, 1.0, LSTAR, slices, method == "rslice", seed=2024)
    n_dir = slices if method == "rslice" else slices * ND
    assert n_active == 0
    assert np.all((U > 0) & (U < 1)) and np.all(lp > LSTAR)
    np.testing.assert_array_equal(V, U)
    np.testing.assert_allclose(lp, lnprob_gauss(U), rtol=0, atol=1e-12)
    assert np.array_equal(ncall, nexpand + ncontract)
    assert np.all(nexpand >= 2 * n_dir) and np.all(ncontract >= n_dir)
    assert not np.array_equal(U, U0)
    # still uniform in the region: every coordinate's mean and variance against 200 000 fresh samples, within four standard
    # errors of the K-chain estimate (the variance's from the fresh samples' fourth moment)
    mu, var = fresh.mean(axis=0), fresh.var(axis=0)
    m4 = ((fresh - mu) ** 4).mean(axis=0)
    se_mean, se_var = np.sqrt(var / K), np.sqrt((m4 - var ** 2) / K)
    dm, dv = U.mean(axis=0) - mu, ((U - mu) ** 2).mean(axis=0) - var
    print(method, "mean / se", dm / se_mean, "var / se", dv / se_var)
    assert np.all(np.abs(dm) <= 4 * se_mean), dm / se_mean
    assert np.all(np.abs(dv) <= 4 * se_var), dv / se_var


def test_reference_chain_does_not_depend_on_how_it_is_stopped_and_resumed():
    """max_rounds stops a walk with every chain at its start or above the threshold; the draws are the chain's own."""
    U0 = region_samples(np.random.default_rng(9), 64)
    lp0 = lnprob_gauss(U0)
    axes = CHOL * np.sqrt(R2_MEDIAN)
    full = slice_walk_ref(lnprob_u_gauss, U0, U0, lp0, axes, 1.0, LSTAR, 2, False, seed=5)
    cut = slice_walk_ref(lnprob_u_gauss, U0, U0, lp0, axes, 1.0, LSTAR, 2, False, seed=5, max_rounds=5)
    assert full[6] == 0 and cut[6] > 0
    same = np.all(cut[0] == U0, axis=1)
    assert np.all(cut[2][~same] > LSTAR) and np.array_equal(cut[2][same], lp0[same])
    again = slice_walk_ref(lnprob_u_gauss, U0, U0, lp0, axes, 1.0, LSTAR, 2, False, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(full[:6], again[:6]))
    other = slice_walk_ref(lnprob_u_gauss, U0, U0, lp0, axes, 1.0, LSTAR, 2, False, seed=6)
    assert not np.array_equal(other[0], full[0])


# ---- the sampler's side: a fake proposer whose slice_walk is the reference chain over an analytic lnprob -------------------------
SIG = 0.05
NDIM = 3
LOGZ_TRUE = NDIM * np.log(np.sqrt(2 * np.pi) * SIG)      # unnormalised Gaussian under U[0,1]^3


def loglike_batch(V):
    return -0.5 * np.sum(((V - 0.5) / SIG) ** 2, axis=1)


def ptform_batch(U):
    return U.copy()


class FakeProposer(object):
    def __init__(self):
        self.walks = 0

    def lnprob_u(self, U):
        U = np.array(U, dtype=np.float64)
        return U, loglike_batch(U)

    def slice_walk(self, U, V, lnprob, axes, scale, loglstar, slices, random_dirs, seed, ell=None, chunk=16, max_rounds=None):
        self.walks += 1
        return slice_walk_ref(self.lnprob_u, U, V, lnprob, axes, scale, loglstar, slices, random_dirs, seed, ell=ell,
                              max_rounds=max_rounds)


class HostOnlyProposer(object):
    def lnprob_u(self, U):
        U = np.array(U, dtype=np.float64)
        return U, loglike_batch(U)


@pytest.mark.parametrize("method", ["slice", "rslice"])
def test_nested_sampler_with_slice_walks_from_the_proposer(method, monkeypatch):
    prop = FakeProposer()
    s = NestedSampler(loglike_batch, ptform_batch, NDIM, nlive=300, bound='single', sample=method, slices=3, batched=True,
                      rstate=np.random.default_rng(17), queue_size=300, proposer=prop, slice_device=True)

    def never(*a, **k):
        raise AssertionError("_eval_u called in a run with slice_device=True")
    monkeypatch.setattr(s, "_eval_u", never)
    s.run_nested(dlogz=0.05)
    r = s.results
    print(method, "logz", r.logz[-1], "true", LOGZ_TRUE, "err", r.logzerr[-1], "walks", prop.walks)
    assert prop.walks > 0
    assert abs(r.logz[-1] - LOGZ_TRUE) <= 3 * r.logzerr[-1], (r.logz[-1], LOGZ_TRUE, r.logzerr[-1])
    assert np.all(np.diff(r.logl[:-300]) >= 0) and 1e-4 < s.scale < 8.0


def test_slice_device_needs_a_proposer_that_walks_and_is_off_by_default():
    kw = dict(nlive=50, bound='single', sample='slice', slices=2, batched=True, rstate=np.random.default_rng(1), queue_size=50)
    with pytest.raises(ValueError):
        NestedSampler(loglike_batch, ptform_batch, NDIM, slice_device=True, **kw)
    with pytest.raises(ValueError):
        NestedSampler(loglike_batch, ptform_batch, NDIM, slice_device=True, proposer=HostOnlyProposer(), **kw)
    prop = FakeProposer()
    s = NestedSampler(loglike_batch, ptform_batch, NDIM, proposer=prop, **kw)
    assert s.slice_device is False
    s.run_nested(dlogz=0.5, maxiter=200)
    assert prop.walks == 0
    s = NestedSampler(loglike_batch, ptform_batch, NDIM, proposer=prop, slice_device=False, **kw)
    s.run_nested(dlogz=0.5, maxiter=200)
    assert prop.walks == 0
