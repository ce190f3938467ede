"""The Chebyshev blaze polynomial (payne_opts.npoly; pc_0 .. pc_{n-1} in theta columns 8 .. 8 + npoly - 1; stage 3 = genspec, and
the chi^2 of a modpoly fit) at every order through every kernel that applies it.

Clenshaw's recurrence is written out twice (obs_loop in post_core.hpp for every post kernel, and payne_lsf_kernel's own copy that
reads theta directly), each with a branch for one coefficient, one for two and a loop from three up; two loaders fill
CandState::poly (the record made ahead by the hidden-layer launch, and phase_setup inside the kernel); npoly != 0 switches the fused
observed-grid tails off, so a blaze fit takes the general observed-grid phase of every post kernel; and the photometric block of
theta sits behind the coefficients.  The reference is always the numpy oracle in fp64.

Bounds (the project's own): stage 3 identical NaN pattern and |dflux| <= 2e-6 (what test_api_gpu.py / test_fuzz_gpu.py allow where
the blaze multiplies); |dlnL| <= lnl_tol(ref); lnL against -chi^2/2 recomputed in fp64 from the same context's stage-3 rows
<= 2e-5 |lnL| + 5e-3 (test_full_size_properties).  Every comparison says which rows are NaN by design; all others must be finite."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from thepayne_amd import synth, nnio, _lib
from helpers import SPEC_PARS, theta_full, yst_problem, lnl_tol

pytestmark = pytest.mark.gpu
BLAZE_FLUX_TOL = 2e-6
SPEC6 = [p for p in SPEC_PARS if p != 'Inst_R']


@pytest.fixture(scope="module")
def Engine():
    from thepayne_amd.engine import PayneEngine
    return PayneEngine


def _net(raw):
    return nnio.normalize_spec_net(raw)


def _pc_names(npoly):
    return ["pc_%d" % i for i in range(npoly)]


def _coefficients(B, npoly, seed):
    """pc_0 ~ U(0.9, 1.1), the others N(0, 0.05): a blaze within about 0.7 .. 1.3, different in every row."""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0.9, 1.1, B), rng.normal(0.0, 0.05, (B, npoly - 1))])


def _chi_from_rows(spec, flux, eflux):
    return -0.5 * (((spec.astype(np.float64) - flux) / eflux) ** 2).sum(axis=1)


def _compare(got3, lnl, ref3, ref_l, flux, eflux, nan_rows, partial_rows=(), tag=None):
    """Stage-3 rows and lnL against the oracle's, and lnL against the chi^2 of the stage-3 rows.  nan_rows: lnL NaN by design;
    partial_rows: of those, the rows whose spectrum keeps finite pixels.  Returns (max |dflux|, max |dlnL| / lnl_tol)."""
    B = len(ref_l)
    want_nan = np.zeros(B, bool); want_nan[list(nan_rows)] = True
    assert np.array_equal(np.isnan(ref_l), want_nan), (tag, np.flatnonzero(np.isnan(ref_l)))      # (the design is what the oracle says)
    fin_rows = ~want_nan
    assert np.isfinite(ref3[fin_rows]).all()
    for r in partial_rows:
        assert np.isnan(ref3[r]).any() and np.isfinite(ref3[r]).any(), (tag, r)
    assert np.array_equal(np.isnan(got3), np.isnan(ref3)), tag
    ok = np.isfinite(ref3)
    dflux = np.abs(got3.astype(np.float64) - ref3)[ok].max()
    assert np.array_equal(np.isnan(lnl), want_nan), (tag, lnl)
    rel = (np.abs(lnl - ref_l)[fin_rows] / lnl_tol(ref_l[fin_rows])).max()
    print("%s: %d finite rows, max |dflux| = %.3g, max |dlnL| / lnl_tol = %.3g" % (tag, fin_rows.sum(), dflux, rel))
    assert dflux <= BLAZE_FLUX_TOL, (tag, dflux)
    assert rel <= 1.0, (tag, rel)
    chi = _chi_from_rows(got3[fin_rows], flux, eflux)
    assert np.all(np.abs(chi - lnl[fin_rows]) <= 2e-5 * np.abs(lnl[fin_rows]) + 5e-3), (tag, np.abs(chi - lnl[fin_rows]).max())
    return dflux, rel


# ---- a. orders on the LDS post kernels ----------------------------------------------------------------------------------------------
LEAN10, FULL10 = "payne_post_kernel<10, true, true>", "payne_post_kernel<10, true>"
# variant -> (post kernel of a likelihood call, of a predict call, the rows' domain) on the 1024-pixel geometric grid
LDS_VARIANTS = {
    "default": (0, LEAN10, FULL10, "frequency"),
    "no_prep": (_lib.V_NO_PREP, FULL10, FULL10, "frequency"),                   # (no records: the likelihood-only build needs them)
    "post_full": (_lib.V_POST_FULL, FULL10, FULL10, "frequency"),
    "post_generic": (_lib.V_POST_GENERIC, "payne_post_kernel<0, true>", "payne_post_kernel<0, true>", "pixels"),
    "rows_pixel": (_lib.V_ROWS_PIXEL, LEAN10, FULL10, "pixels"),
    "tw_global": (_lib.V_TW_GLOBAL, "payne_post_kernel<0, false>", "payne_post_kernel<0, false>", "pixels"),
}
# shape -> (npix, nobs, H, post kernel of a likelihood call, of a predict call, rows) on variant 0
LDS_SHAPES = {
    "resampled": (1000, 700, 50, LEAN10, FULL10, "frequency"),                  # (frequency rows that carry the resampling)
    "runtime_geometry": (300, 250, 32, "payne_post_kernel<0, true>", "payne_post_kernel<0, true>", "pixels"),
}
_lds_problems, _lds_references, _lds_stage2_npoly0 = {}, {}, {}     # shape / (shape, npoly) / (shape, variant, rows kept)
ALL_ROWS = tuple(range(12))
NAN_BY_DESIGN = (3, 4, 5)


def _lds_problem(shape):
    """(raw, obs, flux, eflux, th7) with the designed rows: 1 does not rotate, 2 has no instrumental stage (plain interpolation),
    3 has Inst_R above the network's resolution (lnL NaN by contract), 4 is Doppler-shifted by +300 km/s so that the model leaves
    part of the observed grid (NaN pixels, NaN lnL).  Row 5's NaN coefficient is set where the coefficients are drawn."""
    if shape not in _lds_problems:
        if shape == "small":
            raw, obs, flux, eflux = yst_problem("small", H=64, line_depth=0.3)
        else:
            npix, nobs, H = LDS_SHAPES[shape][:3]
            raw = synth.make_yst_net(npix=npix, H=H, seed=11, line_depth=0.1)
            obs = synth.obs_grid(raw["wavelength"], nobs, inset=0.06 * (raw["wavelength"][-1] - raw["wavelength"][0]))
            th0 = synth.draw_candidates(1, seed=npix)
            flux = O.genspec(raw, list(theta_full(th0)[0, :8]), outwave=obs)[1] + np.random.default_rng(3).normal(0, 0.01, nobs)
            eflux = np.full(nobs, 0.01)
        th7 = synth.draw_candidates(12, seed=61)
        th7[1, 5] = 0.0
        th7[2, 6] = np.nan
        th7[3, 6] = 1.2 * raw["resolution"] / 2.355
        th7[4, 4] = 300.0
        th7.setflags(write=False)
        _lds_problems[shape] = (raw, obs, flux, eflux, th7)
    return _lds_problems[shape]


def _lds_reference(shape, npoly):
    key = (shape, npoly)
    if key not in _lds_references:
        raw, obs, flux, eflux, th7 = _lds_problem(shape)
        pcs = _coefficients(12, npoly, seed=200 + npoly)
        pcs[5, min(1, npoly - 1)] = np.nan                          # row 5: pc_1 (pc_0 where it is the only one) absent
        th = theta_full(th7, npoly=npoly, pc=pcs)
        L = O.OracleLikelihood(raw, obs, flux, eflux, SPEC_PARS + _pc_names(npoly), modpoly=True)
        with np.errstate(all="ignore"):
            ref3 = np.array([O.genspec(raw, list(t[:8 + npoly]), outwave=obs, modpoly=True)[1] for t in th])
            ref_l = np.array([L.lnlikefn(list(t) + list(p)) for t, p in zip(th7, pcs)])
        assert np.isnan(ref3[5]).all()
        for a in (th, ref3, ref_l):
            a.setflags(write=False)
        _lds_references[key] = (th, ref3, ref_l)
    return _lds_references[key]


def _run_lds(Engine, shape, npoly, variant, post_lnl, post_pred, rows, tag, keep=ALL_ROWS):
    """Every check of group a on the designed rows `keep` (all twelve unless said otherwise).  `rows` is the domain the HOST plans
    the rows in (kernels_used): on a resampled grid a candidate that does not rotate makes its launch fall back to pixels on the
    device, which that word does not show.  Returns the likelihoods."""
    raw, obs, flux, eflux, th7 = _lds_problem(shape)
    th, ref3, ref_l = (a[list(keep)].copy() for a in _lds_reference(shape, npoly))
    th7 = th7[list(keep)]
    B = len(th)
    nan_rows = tuple(keep.index(r) for r in NAN_BY_DESIGN)
    eng = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=16, variant=variant)
    assert eng.ncols == 8 + npoly + 4
    lnl = eng.lnlike_batch(th).cpu().numpy()
    used = eng.kernels_used()
    assert used["post"] == post_lnl and used["rows"] == rows, (tag, used)
    got3 = eng.predict_batch(th, stage=3, fwhm_R=True).cpu().numpy()
    used = eng.kernels_used()
    assert used["post"] == post_pred and used["rows"] == rows, (tag, used)
    _compare(got3, lnl, ref3, ref_l, flux, eflux, nan_rows=nan_rows, partial_rows=(keep.index(4),), tag=tag)
    # stage 2 does not see the coefficients: the bytes of a context without a polynomial on the same first eight columns
    s2 = eng.predict_batch(th, stage=2, fwhm_R=True).cpu().numpy()
    if (shape, variant, keep) not in _lds_stage2_npoly0:
        e0 = Engine(_net(raw), obs=(obs, flux, eflux), npoly=0, b_max=16, variant=variant)
        _lds_stage2_npoly0[(shape, variant, keep)] = e0.predict_batch(theta_full(th7), stage=2, fwhm_R=True).cpu().numpy()
        e0.close()
    plain = _lds_stage2_npoly0[(shape, variant, keep)]
    assert np.isfinite(plain[keep.index(5)]).all() and np.array_equal(s2, plain, equal_nan=True), tag
    # determinism and independence of the position in the batch
    rev = th[::-1].copy()
    assert np.array_equal(eng.lnlike_batch(rev).cpu().numpy()[::-1], lnl, equal_nan=True), tag
    assert np.array_equal(eng.predict_batch(rev, stage=3, fwhm_R=True).cpu().numpy()[::-1], got3, equal_nan=True), tag
    # a batch larger than b_max is chunked by the host layer
    big = np.tile(th, (3, 1))[:2 * B + 3]
    l3 = eng.lnlike_batch(big).cpu().numpy()
    s3 = eng.predict_batch(big, stage=3, fwhm_R=True).cpu().numpy()
    for k in range(len(big)):
        assert np.array_equal(l3[k], lnl[k % B], equal_nan=True) and np.array_equal(s3[k], got3[k % B], equal_nan=True), (tag, k)
    eng.close()
    return lnl


@pytest.mark.parametrize("loader", ["default", "no_prep"])
@pytest.mark.parametrize("npoly", [1, 2, 3, 4, 7, 12])
def test_every_order_through_both_coefficient_loaders(Engine, npoly, loader):
    """One coefficient, two, and the loop from three to PAYNE_MAX_POLY, loaded by the record made ahead (prep_candidate: twelve loads
    with a clamped column) and inside the kernel (PAYNE_V_NO_PREP: phase_setup)."""
    v, post_lnl, post_pred, rows = LDS_VARIANTS[loader]
    _run_lds(Engine, "small", npoly, v, post_lnl, post_pred, rows, "a/%s/npoly=%d" % (loader, npoly))


@pytest.mark.parametrize("variant", ["post_full", "post_generic", "rows_pixel", "tw_global"])
@pytest.mark.parametrize("npoly", [1, 2, 12])
def test_short_and_full_orders_on_every_lds_kernel_form(Engine, npoly, variant):
    v, post_lnl, post_pred, rows = LDS_VARIANTS[variant]
    _run_lds(Engine, "small", npoly, v, post_lnl, post_pred, rows, "a/%s/npoly=%d" % (variant, npoly))


ALL_ROTATE = tuple(r for r in ALL_ROWS if r != 1)


@pytest.mark.parametrize("shape,batch", [("resampled", "all_rotate"), ("resampled", "one_does_not"), ("runtime_geometry", "one_does_not")])
@pytest.mark.parametrize("npoly", [1, 2, 12])
def test_short_and_full_orders_on_other_grids(Engine, npoly, shape, batch):
    """300 model pixels: the runtime-geometry kernel by itself.  1000 model pixels: rows in the frequency domain that carry the
    rotation stage's resampling -- as long as every candidate of the launch rotates.  One that does not (designed row 1) makes the
    records' writer flag its launch, and the output layer and the post kernel of that launch run on pixels, decided on the device;
    kernels_used() shows the host's plan, "frequency", either way.  So the resampled grid runs twice, every check each time: the
    designed rows without row 1 (every launch, the reversed batch and both chunks included, stays on frequency rows) and all twelve
    (every launch falls back).  What ran on the device is read off the bytes: the fall-back IS the pixel path, so its likelihoods are
    those of PAYNE_V_ROWS_PIXEL to the bit (test_rows_of_a_resampled_grid_vs_oracle), the frequency rows' are not."""
    post_lnl, post_pred, rows = LDS_SHAPES[shape][3:]
    keep = ALL_ROTATE if batch == "all_rotate" else ALL_ROWS
    lnl = _run_lds(Engine, shape, npoly, 0, post_lnl, post_pred, rows, "a/%s/%s/npoly=%d" % (shape, batch, npoly), keep=keep)
    if shape == "resampled":
        raw, obs, flux, eflux, _ = _lds_problem(shape)
        th = _lds_reference(shape, npoly)[0][list(keep)].copy()
        pix = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=16, variant=_lib.V_ROWS_PIXEL)
        lp = pix.lnlike_batch(th).cpu().numpy()
        assert pix.kernels_used()["rows"] == "pixels"
        pix.close()
        assert np.array_equal(np.isnan(lp), np.isnan(lnl)) and int(np.isfinite(lp).sum()) == len(keep) - 3
        assert np.array_equal(lnl, lp, equal_nan=True) == (batch == "one_does_not"), batch


# ---- b. blaze with an LSF vector ---------------------------------------------------------------------------------------------------
def _lsf_vector(obs):
    return 0.075 * (1.0 + 0.3 * (obs - obs.mean()) / (obs.max() - obs.min()))


LSF_FORMS = {"lds": (0, "payne_lsf_kernel<false>"), "global": (_lib.V_LSF_GLOBAL, "payne_lsf_kernel<true>")}
_lsf_stage2_npoly0 = {}                                                 # form -> stage-2 rows of a context without a polynomial


@pytest.mark.parametrize("npoly", [1, 2, 3, 12])
def test_blaze_behind_an_lsf_vector(Engine, npoly):
    """payne_lsf_kernel's own Clenshaw copy (coefficients straight from theta), its multiply and its (m - 1) p + (p - 1) residual, in
    the LDS form and in the global form, which walks 300 candidates as launches of 256 and 44 with theta at an offset: every row
    of both against the oracle's LSF branch, and the two forms against each other."""
    raw, obs, flux, eflux = yst_problem("small", H=64)
    lsf = _lsf_vector(obs)
    B = 300
    th7 = synth.draw_candidates(B, seed=12)
    th7[:, 6] = np.nan                                              # (ignored while the vector is bound)
    th7[7, 5] = 0.0; th7[290, 5] = 0.0                              # one candidate that does not rotate in each launch of the global form
    pcs = _coefficients(B, npoly, seed=300 + npoly)
    th = theta_full(th7, npoly=npoly, pc=pcs)
    L = O.OracleLikelihood(raw, obs, flux, eflux, SPEC6 + _pc_names(npoly), fixedpars={'Inst_R': lsf}, modpoly=True)
    with np.errstate(all="ignore"):
        ref3 = np.array([O.genspec(raw, list(t[:7]) + [lsf] + list(p), outwave=obs, modpoly=True)[1] for t, p in zip(th, pcs)])
        ref_l = np.array([L.lnlikefn(list(t[:6]) + list(p)) for t, p in zip(th7, pcs)])
    res = {}
    for form, (variant, name) in LSF_FORMS.items():
        tag = "b/%s/npoly=%d" % (form, npoly)
        eng = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=B, variant=variant)
        eng.set_lsf(lsf)
        lnl = eng.lnlike_batch(th).cpu().numpy()
        assert eng.kernels_used()["post"] == name, eng.kernels_used()
        got3 = eng.predict_batch(th, stage=3, fwhm_R=True).cpu().numpy()
        assert eng.kernels_used()["post"] == name, eng.kernels_used()
        _compare(got3, lnl, ref3, ref_l, flux, eflux, nan_rows=(), tag=tag)
        # stage 2 with the vector bound: the bytes of a context without a polynomial with the same vector
        s2 = eng.predict_batch(th, stage=2, fwhm_R=True).cpu().numpy()
        eng.close()
        if form not in _lsf_stage2_npoly0:
            e0 = Engine(_net(raw), obs=(obs, flux, eflux), npoly=0, b_max=B, variant=variant)
            e0.set_lsf(lsf)
            _lsf_stage2_npoly0[form] = e0.predict_batch(theta_full(th7), stage=2, fwhm_R=True).cpu().numpy()
            e0.close()
        assert np.isfinite(s2).all() and np.array_equal(s2, _lsf_stage2_npoly0[form]), tag
        res[form] = lnl
    # the two forms against each other (the same arithmetic apart from the median's algorithm)
    assert np.allclose(res["lds"], res["global"], rtol=1e-9, atol=1e-6), np.abs(res["lds"] - res["global"]).max()


def test_blaze_behind_an_lsf_vector_on_a_long_row(Engine, golden):
    """A 20 000-pixel model takes the global form by itself (n1 > 8192): five coefficients, three candidates, the observed grid and
    the LSF vector of the frozen long-row vectors (g12)."""
    g = golden("g12_long_rows")
    raw = synth.make_yst_net(npix=20000, H=16, seed=41, line_depth=0.3)
    obs, lsf = np.ascontiguousarray(g["lsf_obs"], dtype=np.float64), np.ascontiguousarray(g["lsf_lsfs"][0], dtype=np.float64)
    npoly, B = 5, 3
    lab = g["lsf_label"]
    th7 = np.array([[lab[0], lab[1], lab[2], lab[3], vrad, vrot, np.nan] for vrad, vrot in ((12.0, 4.0), (-8.0, 0.0), (3.0, 7.5))])
    pcs = _coefficients(B, npoly, seed=305)
    th = theta_full(th7, npoly=npoly, pc=pcs)
    with np.errstate(all="ignore"):
        ref3 = np.array([O.genspec(raw, list(t[:7]) + [lsf] + list(p), outwave=obs, modpoly=True)[1] for t, p in zip(th, pcs)])
    eflux = np.full(len(obs), 0.01)
    flux = ref3[0] + np.random.default_rng(5).normal(0, 0.01, len(obs))
    L = O.OracleLikelihood(raw, obs, flux, eflux, SPEC6 + _pc_names(npoly), fixedpars={'Inst_R': lsf}, modpoly=True)
    ref_l = np.array([L.lnlikefn(list(t[:6]) + list(p)) for t, p in zip(th7, pcs)])
    eng = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=4)
    eng.set_lsf(lsf)
    lnl = eng.lnlike_batch(th).cpu().numpy()
    assert eng.kernels_used()["post"] == "payne_lsf_kernel<true>", eng.kernels_used()
    got3 = eng.predict_batch(th, stage=3, fwhm_R=True).cpu().numpy()
    eng.close()
    _compare(got3, lnl, ref3, ref_l, flux, eflux, nan_rows=(), tag="b/long_row/npoly=5")


# ---- c. spectra larger than LDS -----------------------------------------------------------------------------------------------------
# npix -> (nobs, lam0, R, B, the post kernel of variant 0, the rows' domain there): test_spectra_larger_than_lds_vs_oracle's shapes.
# The vsini maps of the two power-of-two grids are the identity, so their frequency rows need no fall-back for the candidate that
# does not rotate; PAYNE_V_BIG_WORKSPACE takes pixel rows.
BIG_SHAPES = {40000: (30000, 5150.0, 32000.0, 3, "payne_post_chip_kernel", "pixels"),
              65536: (60000, 4000.0, 100000.0, 5, "payne_post_chip_kernel", "frequency"),
              25600: (20000, 5150.0, 32000.0, 5, "payne_post_chip2_kernel", "pixels"),
              32768: (30000, 4500.0, 60000.0, 5, "payne_post_chip2_kernel", "frequency")}
BIG_RUNS = [(npix, 5, ws) for npix in BIG_SHAPES for ws in (False, True)] + [(npix, n, False) for npix in (32768, 65536) for n in (1, 2, 12)]


@pytest.mark.parametrize("npix,npoly,workspace", BIG_RUNS)
def test_blaze_on_spectra_larger_than_lds(Engine, npix, npoly, workspace):
    """n1 > 16384: payne_post_chip_kernel (65 536 points), payne_post_chip2_kernel (32 768) and, with PAYNE_V_BIG_WORKSPACE,
    payne_post_big_kernel.  A polynomial switches the observed-grid loop on the compute unit off (obs_on_chip), so these are the
    general observed-grid phase of the three kernels; b_max = 2 < B: the host layer walks the batch."""
    nobs, lam0, R, B, post0, rows0 = BIG_SHAPES[npix]
    raw = synth.make_yst_net(npix=npix, lam0=lam0, R_fwhm=R, H=16, seed=31, line_depth=0.1)
    obs = synth.obs_grid(raw["wavelength"], nobs, inset=0.0005, relative=True)
    th7 = synth.draw_candidates(B, seed=npix)
    th7[:, 6] = np.linspace(0.6, 0.85, B) * R                       # instrument R below the ANN's own
    th7[1, 5] = 0.0                                                 # one candidate that does not rotate
    flux = O.genspec(raw, list(theta_full(th7[0])[0, :8]), outwave=obs)[1] + np.random.default_rng(1).normal(0, 0.01, nobs)
    eflux = np.full(nobs, 0.01)
    pcs = _coefficients(B, npoly, seed=400 + npoly)
    th = theta_full(th7, npoly=npoly, pc=pcs)
    L = O.OracleLikelihood(raw, obs, flux, eflux, SPEC_PARS + _pc_names(npoly), modpoly=True)
    ref3 = np.array([O.genspec(raw, list(t[:8 + npoly]), outwave=obs, modpoly=True)[1] for t in th])
    ref_l = np.array([L.lnlikefn(list(t) + list(p)) for t, p in zip(th7, pcs)])
    eng = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=2, variant=_lib.V_BIG_WORKSPACE if workspace else 0)
    lnl = eng.lnlike_batch(th).cpu().numpy()
    post, rows = ("payne_post_big_kernel", "pixels") if workspace else (post0, rows0)
    used = eng.kernels_used()
    assert used["post"] == post and used["rows"] == rows, used
    got3 = eng.predict_batch(th, stage=3, fwhm_R=True).cpu().numpy()
    used = eng.kernels_used()
    assert used["post"] == post and used["rows"] == rows, used
    eng.close()
    _compare(got3, lnl, ref3, ref_l, flux, eflux, nan_rows=(), tag="c/%d/npoly=%d/%s" % (npix, npoly, "workspace" if workspace else "default"))


# ---- d. joint likelihood: the photometric block behind the coefficients -------------------------------------------------------------
@pytest.mark.parametrize("launch", ["rides", "own_launch"])
@pytest.mark.parametrize("photscale", [True, False], ids=["scaled", "dist"])
@pytest.mark.parametrize("npoly", [1, 12])
def test_photometric_block_behind_the_coefficients(Engine, npoly, photscale, launch):
    """The photometric columns start at 8 + npoly: the SED tiles of the hidden-layer launch and payne_sed_kernel as a launch of its
    own (PAYNE_V_SED_OWN_LAUNCH) are both told so.  Photometric values that differ from row to row and from every coefficient; the
    joint lnL against the oracle, and the magnitudes by themselves (sed_batch) so that a failure says which half moved."""
    from thepayne_amd.engine import highav_coefficients
    raw, obs, flux, eflux = yst_problem("small", H=64)
    phot = synth.make_phot_nets()
    phot["hiav"] = highav_coefficients(phot["filters"])
    obs_phot = {f: (5.0 + 0.1 * i, 0.05) for i, f in enumerate(phot["filters"])}
    B = 16
    th7 = synth.draw_candidates(B, seed=71)
    rng = np.random.default_rng(72)
    av = rng.uniform(0.0, 1.0, B)
    if photscale:
        names, pp = ['log(A)', 'Av'], np.column_stack([rng.uniform(-3.0, 7.0, B), av])
    else:
        names, pp = ['log(R)', 'Dist', 'Av'], np.column_stack([rng.uniform(-0.5, 0.5, B), rng.uniform(10.0, 1000.0, B), av])
    pcs = _coefficients(B, npoly, seed=500 + npoly)
    eng = Engine(_net(raw), obs=(obs, flux, eflux), phot=phot, obs_phot=obs_phot, photscale=photscale, npoly=npoly, b_max=B,
                 variant=_lib.V_SED_OWN_LAUNCH if launch == "own_launch" else 0)
    assert eng.phot_off == 8 + npoly and eng.ncols == 8 + npoly + 4
    th = theta_full(th7, npoly=npoly, pc=pcs)
    if photscale:
        th[:, eng.phot_off], th[:, eng.phot_off + 2] = pp[:, 0], pp[:, 1]
    else:
        th[:, eng.phot_off], th[:, eng.phot_off + 1], th[:, eng.phot_off + 2] = pp[:, 0], pp[:, 1], pp[:, 2]
    L = O.OracleLikelihood(raw, obs, flux, eflux, SPEC_PARS + names + _pc_names(npoly), modpoly=True, phot=phot, obs_phot=obs_phot,
                           photscale=photscale)
    with np.errstate(all="ignore"):
        ref = np.array([L.lnlikefn(list(t) + list(q) + list(p)) for t, q, p in zip(th7, pp, pcs)])
    assert np.isfinite(ref).all()
    lnl = eng.lnlike_batch(th).cpu().numpy()
    used = eng.kernels_used()
    assert (used["sed"] == "payne_sed_kernel") == (launch == "own_launch"), used
    rel = (np.abs(lnl - ref) / lnl_tol(ref)).max()
    print("d/%s/%s/npoly=%d: max |dlnL| / lnl_tol = %.3g" % ("scaled" if photscale else "dist", launch, npoly, rel))
    assert np.isfinite(lnl).all() and rel <= 1.0, rel
    # the magnitudes by themselves, on the same parameters
    logt = np.log10(th7[:, 0])
    nanc = np.full(B, np.nan)
    if photscale:
        sp = np.column_stack([logt, th7[:, 1], th7[:, 2], th7[:, 3], av, np.full(B, 3.1), nanc, nanc, pp[:, 0]])
        mref = np.array([O.sed_mags(phot, r[0], r[1], r[2], r[3], av=r[4], rv=3.1, logA=r[8]) for r in sp])
    else:
        logl = 2.0 * pp[:, 0] + 4.0 * (logt - np.log10(5770.0))
        sp = np.column_stack([logt, th7[:, 1], th7[:, 2], th7[:, 3], av, np.full(B, 3.1), logl, pp[:, 1], nanc])
        mref = np.array([O.sed_mags(phot, r[0], r[1], r[2], r[3], av=r[4], rv=3.1, logl=r[6], dist=r[7]) for r in sp])
    assert np.abs(eng.sed_batch(sp).cpu().numpy() - mref).max() <= 1e-9
    eng.close()


# ---- e. ABI -------------------------------------------------------------------------------------------------------------------------
def test_theta_columns_and_the_range_of_npoly(Engine):
    raw, obs, flux, eflux = yst_problem("tiny", H=32)
    for npoly in (0, 1, _lib.PAYNE_MAX_POLY):
        eng = Engine(_net(raw), obs=(obs, flux, eflux), npoly=npoly, b_max=4)
        assert eng.ncols == 8 + npoly + 4                           # (payne_theta_cols of the new context)
        # a theta with too few columns (a row without its photometric block; a row of another order) is refused, not read past its end
        for ncols in (8 + npoly, 8 + npoly + 3, 8 + npoly + 5):
            with pytest.raises(ValueError, match=r"theta must be \[B, %d\]" % (8 + npoly + 4)):
                eng.lnlike_batch(np.zeros((2, ncols)))
            with pytest.raises(ValueError, match="theta must be"):
                eng.predict_batch(np.zeros((2, ncols)), stage=3)
        eng.close()
    # payne_ctx_create outside 0 .. PAYNE_MAX_POLY: PAYNE_E_INVALID, a message, no context.  (opts are checked before the model is
    # looked at: an empty descriptor will do; were that order to change, the message would not name npoly.)
    lib = _lib.load()
    for bad in (_lib.PAYNE_MAX_POLY + 1, -1):
        mdesc, opts, ctx = _lib.ModelDesc(), _lib.Opts(4, bad, 0, 0), C.c_void_p(0xdead)
        rc = lib.payne_ctx_create(mdesc, None, None, C.byref(opts), 0, C.byref(ctx))
        assert rc == _lib.E_INVALID and not ctx.value, (bad, rc, ctx.value)
        assert b"npoly" in lib.payne_last_error(None)
        with pytest.raises(RuntimeError, match="npoly"):
            Engine(_net(raw), obs=(obs,), npoly=bad, b_max=4)
