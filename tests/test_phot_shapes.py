"""The photometric networks at every width, filter count and tile size: the long-double reference, its forward-error bound and
the cases, shared with test_phot_shapes_gpu.py; here the bound is held against the numpy oracle, and the hidden-layer launch's
choice of the tile size (csrc/sed_core.hpp: sed_tile_cands, plain C++) is swept in a stand-alone program built with
g++ -fsanitize=address,undefined.

The bound (u = 2^-53, one fp64 rounding; first order in u, the result times MARGIN = 2 for the second-order terms).  The nets are
fastANN.eval (photANN.py:118-131): xs = (x - xmin) / (xmax - xmin), a1 = s(W1 xs + b1), a2 = s(W2 a1 + b2), BC = w3 a2 + b3 on
fp32 weights promoted to fp64, s(z) = 1 / (1 + exp(-z)).  For ANY order of the fp64 operations, fused or not:
  * a K-term dot product plus its bias is within (K + 2) u S of the exact one, S = sum |w_k a_k| + |b| (each term goes through
    its product's rounding and at most K additions; + 1 for what a blocked order adds);
  * errors already in the inputs a_k arrive as sum |w_k| da_k;
  * s is 1/4-Lipschitz, and its own evaluation is good to 4 u relative (what sed_sigmoid_n's comment claims, ~3e-16; libm's exp
    and an IEEE division are inside that): da = dz / 4 + 4 u a;
  * the encoding costs three roundings, dxs = 3 u |xs|, plus what the label itself carries: Teff = 10**logt from pow() is taken
    as good to 4 u Teff; a theta row's Teff is good to 8 u Teff because the reference program goes Teff -> log10 -> 10** and the
    kernels take the row's value (either is accepted).
So  dz1 = 8 u S1 + |W1| dxs,  da1 = dz1 / 4 + 4 u a1,  dz2 = (H + 2) u S2 + |W2| da1,  da2 = dz2 / 4 + 4 u a2,
    dBC = (H + 2) u S3 + |w3| da2.
The high-Av correction (highred.py:19-21) c0 + c1 av (c2 + c3 rv + c4 rv^2) and the magnitude formulae (predictsed.py:92-103)
are sums of a few terms, some of them much larger than the result (10 log10 Teff ~ 37 against a magnitude of a few): every term
goes through at most eight roundings (a logarithm counted as two), so they add 8 u T, T the sum of the terms' magnitudes.
chi^2 = sum ((m - o) / e)^2 (likelihood.py:109-112): d chi^2 = sum 2 |m - o| dm / e^2 + MARGIN (F + 6) u chi^2 (four roundings a
term, F additions, the sum with the spectrum's part and the factor -1/2).
The reference itself runs the same operations in long double (u_ld = 2^-64): its own error is 2^-11 of the bound at every width.
numpy's fp64 evaluation (oracle.fastann_forward / sed_mags) must lie inside the bound at every shape and row the GPU file uses --
checked here -- or the derivation is wrong; for orientation it is within 5e-16 of the long-double values at the synthetic weights."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from thepayne_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -53
MARGIN = 2.0
CAP = 1e-9                     # the project's tolerance on magnitudes: an outer cap, the derived bound is what bites
LOG5770 = np.log10(LD(5770.0))

# (F, H) of the stand-alone entry points, and the saturated nets (H, factor on w1) with their F
SHAPES = [(1, 1), (2, 15), (1, 16), (3, 17), (3, 32), (5, 48), (3, 63), (7, 64), (3, 65), (4, 80), (2, 100), (2, 2048), (63, 16),
          (64, 16), (65, 16), (255, 16)]
SATURATED = [(H, k) for H in (16, 64, 20) for k in (400.0, 3000.0)]
SAT_F = 3
# the joint likelihood: tile form, fall-backs, post-kernel consumers, the phot-only likelihood, F = 256, the public API
TILE_SHAPES = [(255, 16), (60, 32), (7, 48), (7, 64), (1, 64)]
TILE_B = [1, 10, 20, 40, 70, 130, 200]
FALLBACK_H = [15, 20, 80]
POST_F = [63, 64, 65, 255]
# every (F, H, rows, seed of the rows, factor on w1) of the joint cases: the 200 rows of seed 3 serve all cases on the small spectrum
JOINT_CASES = ([(F, H, 200, 3, 1.0) for F, H in TILE_SHAPES + [(7, H) for H in FALLBACK_H] + [(7, 32)] + [(F, 16) for F in POST_F if F != 255] + [(256, 16), (3, 48)]] +
               [(SAT_F, H, 200, 3, k) for H, k in SATURATED] + [(5, 16, 300, 12, 1.0), (3, 32, 5, 9, 1.0), (1, 16, 129, 4, 1.0), (65, 16, 129, 4, 1.0)])
AVS = (0.0, 4.999, 5.0, 7.5, np.nan)


def make_nets(F, H, seed=None, w1_factor=1.0, nan_row=True):
    """synth.make_phot_nets with F filters of width H, and the high-Av table as an explicit [F, 5] array of random values with one
    all-NaN row (a filter missing from the table; nan_row=False: none -- a likelihood is NaN at Av >= 5 with one, so the joint
    cases that compare values there go without, and one of them keeps it for the NaN pattern)."""
    seed = 1000 * F + H if seed is None else seed
    phot = synth.make_phot_nets(filters=["f%03d" % i for i in range(F)], H=H, seed=seed)
    rng = np.random.default_rng(seed + 1)
    phot["hiav"] = rng.normal(0.0, 0.5, (F, 5))
    if nan_row:
        phot["hiav"][F // 2] = np.nan
    if w1_factor != 1.0:
        phot["w1"] = (phot["w1"] * np.float32(w1_factor)).astype(np.float32)
    return phot


def shape_nets(F, H):
    """The nets of one (F, H) of SHAPES: a single filter whose only row is NaN has no value at Av >= 5 at all, so F = 1 runs a
    second time with its row present."""
    return [make_nets(F, H)] + ([make_nets(F, H, nan_row=False)] if F == 1 else [])


def _sig(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def ref_forward(phot, X, dX=None):
    """fastANN.eval in long double for labels X [B, 6] (dX: what the labels themselves carry, absolute): BC [B, F] long double
    and its first-order bound dBC [B, F] (without MARGIN; fp64 is plenty for a bound).  Rows with a NaN label are NaN: they are
    taken out first, x87 arithmetic on NaN operands is a hundred times slower."""
    X = np.asarray(X, dtype=LD)
    bad = np.isnan(np.asarray(X, dtype=np.float64)).any(axis=1)
    xmin = phot["xmin"].astype(LD)
    den = phot["xmax"].astype(LD) - xmin
    xs = (np.where(bad[:, None], xmin, X) - xmin) / den                                  # [B, 6]
    dxs = (3 * U * np.abs(xs) + (0.0 if dX is None else np.where(bad[:, None], 0.0, np.asarray(dX, dtype=LD)) / np.abs(den))).astype(np.float64)
    w1, w2, w3 = (phot[k].astype(LD) for k in ("w1", "w2", "w3"))
    b1, b2 = (phot[k].astype(LD)[:, None, :, 0] for k in ("b1", "b2"))                    # [F, 1, H]
    b3 = phot["b3"].astype(LD)[:, 0, 0]                                                   # [F]
    a_w1, a_w2, a_w3 = (np.abs(phot[k]).astype(np.float64) for k in ("w1", "w2", "w3"))
    H = w1.shape[1]

    def act(z, dz):
        a = _sig(z)
        return a, dz / 4 + 4 * U * a.astype(np.float64)
    z1 = np.einsum("fhd,bd->fbh", w1, xs) + b1                                            # [F, B, H]
    dz1 = 8 * U * (np.einsum("fhd,bd->fbh", a_w1, np.abs(xs).astype(np.float64)) + np.abs(b1).astype(np.float64)) + np.einsum("fhd,bd->fbh", a_w1, dxs)
    a1, da1 = act(z1, dz1)
    z2 = np.einsum("fhk,fbk->fbh", w2, a1) + b2
    a_w2t = a_w2.transpose(0, 2, 1)
    dz2 = (H + 2) * U * (np.matmul(a1.astype(np.float64), a_w2t) + np.abs(b2).astype(np.float64)) + np.matmul(da1, a_w2t)
    a2, da2 = act(z2, dz2)
    bc = np.einsum("fk,fbk->bf", w3[:, 0, :], a2) + b3                                    # [B, F]
    dbc = (H + 2) * U * (np.einsum("fk,fbk->bf", a_w3[:, 0, :], a2.astype(np.float64)) + np.abs(b3).astype(np.float64)) + np.einsum("fk,fbk->bf", a_w3[:, 0, :], da2)
    return np.where(bad[:, None], LD(np.nan), bc), np.where(bad[:, None], np.nan, dbc)


def _ref_mags(phot, x, dteff, logt, av, rv, logl, dist, logA, t_extra):
    """predictsed.py:75-103 on columns (long double): magnitudes [B, F] and their bound (MARGIN applied), float64 both.
    logl: the dist formula's luminosity where both it and dist are given; t_extra: what went into logl, as magnitudes of terms."""
    hi = ~(av < 5.0)                                                                      # predictsed.py:86-90
    x = x.copy()
    x[hi, 4] = 0.0
    x[hi, 5] = LD(3.1)
    dX = np.zeros(x.shape, dtype=LD)
    dX[:, 0] = dteff
    bc, dbc = ref_forward(phot, x, dX)
    c = np.asarray(phot["hiav"], dtype=LD)                                                # [F, 5]
    a, r = av[:, None], rv[:, None]
    off = c[:, 0] + c[:, 1] * a * (c[:, 2] + c[:, 3] * r + c[:, 4] * (r * r))             # highred.py:19-21
    t_off = np.abs(c[:, 0]) + np.abs(c[:, 1] * a) * (np.abs(c[:, 2]) + np.abs(c[:, 3] * r) + np.abs(c[:, 4] * (r * r)))
    bc = np.where(hi[:, None], bc - off, bc)
    dbc = np.where(hi[:, None], dbc + 8 * U * (t_off + np.abs(bc)), dbc)
    with np.errstate(invalid="ignore", divide="ignore"):
        lgd = np.log10(dist)
    m_d = (-2.5 * logl + LD(4.74) - bc.T).T + (5.0 * lgd - 5.0)[:, None]
    t_d = (2.5 * np.abs(logl) + 4.74 + 5.0 * np.abs(lgd) + 5.0 + t_extra)[:, None] + np.abs(bc)
    m_a = (5.0 * logA - 10.0 * (logt - LOG5770) - LD(0.26))[:, None] - bc
    t_a = (5.0 * np.abs(logA) + 10.0 * np.abs(logt) + 10.0 * LOG5770 + 0.26)[:, None] + np.abs(bc)
    use_d = (~np.isnan(logl) & ~np.isnan(dist))[:, None]
    use_a = ~use_d & ~np.isnan(logA)[:, None]
    m = np.where(use_d, m_d, np.where(use_a, m_a, np.nan))
    t = np.where(use_d, t_d, t_a)
    dm = MARGIN * (dbc + 8 * U * t)
    return m, dm


def ref_bc(phot, X):
    """fastANN.eval (payne_bc_batch): X [B, 6] = Teff, logg, feh, afe, av, rv -> BC [B, F] long double, bound [B, F]."""
    bc, dbc = ref_forward(phot, X)
    return bc, MARGIN * dbc


def ref_sed(phot, rows):
    """FastPayneSEDPredict.sed (payne_sed_batch): rows [B, 9] = logt, logg, feh, afe, av, rv, logl, dist, logA (NaN = absent)."""
    r = np.asarray(rows, dtype=LD)
    teff = np.power(LD(10.0), r[:, 0])
    x = np.column_stack([teff, r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]])
    return _ref_mags(phot, x, 4 * U * np.abs(teff), r[:, 0], r[:, 4], r[:, 5], r[:, 6], r[:, 7], r[:, 8], 0.0)


def ref_theta(phot, th, photscale):
    """GenMod.genphot / genphot_scaled on rows th [B, 7] = Teff, logg, feh, afe, logR | logA, Dist, Av (genmod.py:110-187; Rv = 3.1)."""
    r = np.asarray(th, dtype=LD)
    B = len(r)
    with np.errstate(invalid="ignore"):
        logt = np.log10(r[:, 0])
    nanc = np.full(B, np.nan, dtype=LD)
    x = np.column_stack([r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 6], np.full(B, LD(3.1))])
    if photscale:
        logl, dist, logA, t_extra = nanc, nanc, r[:, 4], 0.0
    else:
        logl = 2.0 * r[:, 4] + 4.0 * (logt - LOG5770)                                     # genmod.py:126
        dist, logA = r[:, 5], nanc
        t_extra = 5.0 * np.abs(r[:, 4]) + 10.0 * np.abs(logt) + 10.0 * LOG5770
    return _ref_mags(phot, x, 8 * U * np.abs(r[:, 0]), logt, r[:, 6], np.full(B, LD(3.1)), logl, dist, logA, t_extra)


def ref_lnl(m, dm, obs_mag, obs_err):
    """-1/2 sum ((m - o) / e)^2 (likelihood.py:109-117) in long double and its bound."""
    o, e = np.asarray(obs_mag, dtype=LD), np.asarray(obs_err, dtype=LD)
    d = m - o
    chi2 = np.sum((d * d) / (e * e), axis=1)
    dchi = np.sum(2.0 * np.abs(d) * dm / (e * e), axis=1) + MARGIN * (len(o) + 6) * U * chi2
    return -0.5 * chi2, 0.5 * dchi


# ---- the rows --------------------------------------------------------------------------------------------------------------
def sed_rows(phot, seed=0, n=40):
    """rows [n, 9] for payne_sed_batch: labels inside xmin .. xmax and a fifth of them up to 20 % of the range outside; Av in
    {0, 4.999, 5.0, 7.5, NaN} x Rv given | NaN x both magnitude formulae; the row before the last has a NaN label, the last one
    neither formula's inputs."""
    rng = np.random.default_rng(seed)
    lo, hi = phot["xmin"][:4].copy(), phot["xmax"][:4].copy()
    u = rng.uniform(0.0, 1.0, (n, 4))
    out = rng.uniform(size=n) < 0.2
    out[:5] = [False, True, False, False, True]
    side = rng.uniform(size=(n, 4)) < 0.5
    u = np.where(out[:, None], np.where(side, -0.2 * u, 1.0 + 0.2 * u), u)
    lab = lo + (hi - lo) * u
    lab[:, 0] = np.maximum(lab[:, 0], 1200.0)
    rows = np.full((n, 9), np.nan)
    rows[:, 0] = np.log10(lab[:, 0])
    rows[:, 1:4] = lab[:, 1:4]
    i = np.arange(n)
    rows[:, 4] = np.array(AVS)[i % 5]
    rows[:, 5] = np.where(np.isin(i // 5, (1, 6)), np.nan, rng.uniform(2.0, 5.0, n))    # (NaN: once through the Av values per formula)
    dist_form = (i // 10) % 2 == 0
    rows[:, 6] = np.where(dist_form, rng.uniform(-1.0, 3.0, n), np.nan)
    rows[:, 7] = np.where(dist_form, rng.uniform(10.0, 3000.0, n), np.nan)
    rows[:, 8] = np.where(dist_form, np.nan, rng.uniform(-2.0, 3.0, n))
    rows[n - 2, 2] = np.nan
    rows[n - 1, 6:9] = np.nan
    return rows


def bc_rows(rows):
    """The same rows as payne_bc_batch takes them: Teff, logg, feh, afe, av, rv."""
    return np.column_stack([10.0 ** rows[:, 0], rows[:, 1:6]])


def theta_rows(B, seed=3):
    """th [B, 7] = Teff, logg, feh, afe (the demo priors' box, inside the spectral net's), log(R) | log(A), Dist, Av on both sides of
    5; row 5 (where there is one) has a NaN label: its neighbours in the same 16-row tile must stay finite."""
    rng = np.random.default_rng(seed)
    th7 = synth.draw_candidates(B, seed=seed)
    th = np.column_stack([th7[:, :4], rng.uniform(-0.5, 1.0, B), rng.uniform(10.0, 3000.0, B), np.array([0.3, 4.999, 5.0, 7.5, 0.0, 1.7])[np.arange(B) % 6]])
    if B > 5:
        th[5, 2] = np.nan
    return th, th7


def obs_phot(phot, seed=5):
    """Observed magnitudes near the model's, errors that differ tenfold between filters."""
    F = len(phot["filters"])
    rng = np.random.default_rng(seed)
    return {f: (float(m), float(e)) for f, m, e in zip(phot["filters"], rng.uniform(3.0, 7.0, F), np.where(np.arange(F) % 2 == 0, 0.05, 0.5))}


# ---- the oracle inside the bound ---------------------------------------------------------------------------------------------
def check(what, got, ref, bound, cap=None):
    """|got - ref| <= bound wherever ref is a number, the NaN patterns identical; prints and returns the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(np.asarray(ref, dtype=np.float64))
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:4])
    if nan.all():
        print("%s: all NaN" % what)
        return 0.0
    err = np.abs(np.where(nan, 0.0, got - ref)).astype(np.float64)
    bnd = np.where(nan, 1.0, bound).astype(np.float64)
    ratio = float((err / bnd).max())
    print("%s: max |d| = %.3g, max |d| / bound = %.3g (median bound %.3g)" % (what, err.max(), ratio, np.median(bnd[~nan])))
    k = np.unravel_index(np.argmax(err / bnd), err.shape)
    assert np.all(err <= bnd), (what, k, err[k], bnd[k])
    if cap is not None:
        assert err.max() <= cap, (what, err.max())
    return ratio


def oracle_sed(phot, rows):
    out = np.full((len(rows), len(phot["filters"])), np.nan)
    for i, r in enumerate(rows):
        kw = {}
        if not (np.isnan(r[6]) or np.isnan(r[7])):
            kw = dict(logl=r[6], dist=r[7])
        elif not np.isnan(r[8]):
            kw = dict(logA=r[8])
        else:
            continue
        with np.errstate(over="ignore"):
            out[i] = O.sed_mags(phot, r[0], r[1], r[2], r[3], av=r[4], rv=r[5], **kw)
    return out


def oracle_bc(phot, X):
    with np.errstate(over="ignore"):
        return np.array([np.atleast_1d(O.fastann_forward(phot, x)) for x in X])


def _oracle_in_bound(what, phot):
    rows = sed_rows(phot)
    m, dm = ref_sed(phot, rows)
    assert np.isfinite(np.asarray(m, dtype=np.float64)).sum() >= m.size // (3 if np.isfinite(phot["hiav"]).any() else 8), what
    r1 = check(what + " sed_mags", oracle_sed(phot, rows), m, dm, CAP)
    X = bc_rows(rows)
    bc, dbc = ref_bc(phot, X)
    r2 = check(what + " fastann_forward", oracle_bc(phot, X), bc, dbc, CAP)
    return max(r1, r2)


@pytest.mark.parametrize("F,H", SHAPES, ids=["F%d-H%d" % s for s in SHAPES])
def test_oracle_is_inside_the_bound_of_the_long_double_reference(F, H):
    for phot in shape_nets(F, H):
        _oracle_in_bound("F=%d H=%d" % (F, H), phot)


@pytest.mark.parametrize("H,k", SATURATED, ids=["H%d-x%d" % s for s in SATURATED])
def test_oracle_is_inside_the_bound_on_saturated_nets(H, k):
    """w1 times 400 and 3000: pre-activations beyond +-700, where numpy's exp overflows (sigmoid 0 or 1) and long double does not."""
    phot = make_nets(SAT_F, H, w1_factor=k)
    rows = sed_rows(phot)
    xs = (bc_rows(rows)[:, :4] - phot["xmin"][:4]) / (phot["xmax"][:4] - phot["xmin"][:4])
    z = np.abs(np.einsum("fhd,bd->bfh", phot["w1"][:, :, :4].astype(np.float64), np.nan_to_num(xs)))
    assert z.max() > 750.0, z.max()
    _oracle_in_bound("saturated H=%d x%d" % (H, k), phot)


@pytest.mark.parametrize("F,H,B,seed,k", JOINT_CASES, ids=["F%d-H%d-B%d-seed%d-x%d" % c for c in JOINT_CASES])
def test_oracle_is_inside_the_bound_on_theta_rows(F, H, B, seed, k):
    """The rows of the joint likelihood (genphot / genphot_scaled) and their chi^2, for both parametrisations."""
    phot = make_nets(F, H, w1_factor=k, nan_row=False)
    op = obs_phot(phot)
    mo, me = np.array([v[0] for v in op.values()]), np.array([v[1] for v in op.values()])
    th, _ = theta_rows(B, seed=seed)
    for photscale in (True, False):
        m, dm = ref_theta(phot, th, photscale)
        fn = O.genphot_scaled if photscale else O.genphot
        with np.errstate(over="ignore"):
            got = np.array([np.atleast_1d(fn(phot, list(t[:4]) + ([t[4], t[6]] if photscale else [t[4], t[5], t[6]]))) for t in th])
        check("F=%d H=%d x%d photscale=%d mags" % (F, H, k, photscale), got, m, dm, CAP)
        lnl, dlnl = ref_lnl(m, dm, mo, me)
        got_l = -0.5 * np.sum(((got - mo) ** 2.0) / (me ** 2.0), axis=1)
        check("F=%d H=%d x%d photscale=%d lnL" % (F, H, k, photscale), got_l, lnl, dlnl)
        assert np.isfinite(got_l).sum() == B - (1 if B > 5 else 0) and (B <= 5 or np.isnan(got_l[5]))


def test_the_reference_is_the_oracle_at_the_projects_tolerance():
    """... and not merely inside a bound of its own making: at the default nets (F = 7, H = 64) the two agree to 5e-16 of the BCs."""
    phot = make_nets(7, 64)
    X = bc_rows(sed_rows(phot))
    bc, dbc = ref_bc(phot, X)
    got = oracle_bc(phot, X)
    ok = ~np.isnan(got)
    assert np.abs(got[ok] - bc[ok]).max() <= 5e-16 and np.median(np.asarray(dbc, dtype=np.float64)[ok]) < 1e-12


# ---- the tile size -----------------------------------------------------------------------------------------------------------
PLANNER = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "thepayne_amd/csrc/sed_core.hpp"
// every (filter, row) pair that the tiles of one launch take, as the hidden-layer kernel numbers them (workgroup j: filter j % F,
// block j / F, rows block * cb .. + cb - 1 below B): each exactly once?
static bool covered_once(int B, int F, int cb) {
  std::vector<unsigned char> n((size_t)B * F, 0);
  const int tiles = F * ((B + cb - 1) / cb);
  for (int j = 0; j < tiles; ++j) {
    const int f = j % F, c0 = (j / F) * cb;
    if (c0 >= B) return false;                                  // a tile without a live row
    for (int r = 0; r < cb; ++r) if (c0 + r < B) ++n[(size_t)(c0 + r) * F + f];
  }
  for (size_t i = 0; i < n.size(); ++i) if (n[i] != 1) return false;
  return true;
}
int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "sweep")) {
    long long bad = 0, seen = 0;
    for (int B = 1; B <= 4096; ++B)
      for (int F = 1; F <= 255; ++F)
        for (int slots = -600; slots <= 600; ++slots) {
          const int cb = sed_tile_cands(B, F, slots);
          const int blocks = (B + cb - 1) / cb;
          // (the blocks tile 0 .. B - 1: the last one starts below B and ends at or past it)
          const bool ok = cb >= 16 && cb <= 48 && cb % 16 == 0 && (long long)(blocks - 1) * cb < B && (long long)blocks * cb >= B;
          if (!ok && !bad++) std::printf("first violation: B=%d F=%d slots=%d cb=%d\n", B, F, slots, cb);
          ++seen;
        }
    static const int Bs[] = {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97, 130, 200, 511, 512, 513, 4095, 4096};
    static const int Fs[] = {1, 2, 7, 63, 64, 65, 255};
    static const int Ss[] = {-600, -1, 0, 1, 6, 7, 8, 63, 64, 65, 254, 255, 256, 495, 510, 600};
    for (int B : Bs) for (int F : Fs) for (int s : Ss)
      if (!covered_once(B, F, sed_tile_cands(B, F, s)) && !bad++) std::printf("first violation (rows): B=%d F=%d slots=%d\n", B, F, s);
    std::printf("%lld %lld\n", seen, bad);
    return bad ? 1 : 0;
  }
  int B, F, slots;
  while (std::scanf("%d %d %d", &B, &F, &slots) == 3) std::printf("%d\n", sed_tile_cands(B, F, slots));
  return 0;
}'''


def build_planner(d):
    """sed_core.hpp's host part with a main() of its own, under ASan and UBSan; returns the program."""
    main, exe = os.path.join(str(d), "sed_cands.cpp"), os.path.join(str(d), "sed_cands_san")
    with open(main, "w") as fh:
        fh.write(PLANNER)
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", ROOT,
                    main, "-o", exe], check=True)
    return exe


def tile_cands(exe, cases):
    """cb for every (B, F, slots) of `cases`."""
    res = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = [int(v) for v in res.stdout.split()]
    assert len(out) == len(cases)
    return out


def free_slots(n_cu, B, H_spec, records=True):
    """What launch_hidden leaves for the photometric tiles: two workgroups a CU less the 32 x 32 GEMM tiles and the record writers."""
    return 2 * n_cu - ((B + 31) // 32) * ((H_spec + 31) // 32) - ((B + 255) // 256 if records else 0)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(tmp_path_factory.mktemp("sed_cands"))


def test_tile_size_over_every_batch_filter_count_and_free_slots(planner):
    """B in 1 .. 4096, F in 1 .. 255, slots in -600 .. 600: 16 <= cb <= 48, a multiple of 16, and the F * ceil(B / cb) tiles cover
    every (filter, row) exactly once; the sanitizers stay silent."""
    res = subprocess.run([planner, "sweep"], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, (res.stdout[-500:], res.stderr[-2000:])
    seen, bad = (int(v) for v in res.stdout.split()[-2:])
    assert seen == 4096 * 255 * 1201 and bad == 0


def test_tile_size_is_what_the_launch_computed_before(planner):
    """The function is the three lines launch_hidden had (restated here), value for value on a random sample."""
    rng = np.random.default_rng(0)
    cases = [(int(b), int(f), int(s)) for b, f, s in zip(rng.integers(1, 4097, 20000), rng.integers(1, 256, 20000), rng.integers(-600, 601, 20000))]

    def before(B, F, idle):
        nblk = idle // F if idle >= F else 1
        cb = ((B + nblk - 1) // nblk + 15) & ~15
        return 16 if cb < 16 else min(cb, 48)
    assert tile_cands(planner, cases) == [before(*c) for c in cases]


def test_tile_size_at_c3_and_at_the_edges(planner):
    """C3 (B = 512, F = 7, 2 x 300 spectral net on 256 CUs) keeps its 16-candidate tiles; no free slot at all is one block over the batch."""
    slots = free_slots(256, 512, 300)
    assert slots == 2 * 256 - 160 - 2
    cases = [(512, 7, slots), (512, 7, 0), (512, 7, -5), (20, 7, 6), (20, 7, 7), (33, 255, 510), (33, 255, 509), (100, 1, 2), (100, 1, 3)]
    assert tile_cands(planner, cases) == [16, 48, 48, 32, 32, 32, 48, 48, 48]
