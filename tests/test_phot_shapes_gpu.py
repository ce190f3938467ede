"""The photometric networks on the MI355X at every width, filter count and tile size, against the long-double reference of
test_phot_shapes.py within its derived forward-error bound (that file's docstring; the oracle is held inside the same bound there):
  * payne_sed_kernel through the stand-alone entry points (payne_sed_batch, payne_bc_batch) at widths on both sides of every loop
    of the kernel, and on saturated nets;
  * the joint likelihood's photometric half ISOLATED: the spectrum is bound with eflux = 1e15 (1 / eflux^2 = 1e-30, a normal fp32),
    so the spectral chi^2 is below 1e-20 -- asserted on the oracle's spectrum -- and lnL IS -1/2 chi^2_phot, comparable at the
    bound of the fp64 arithmetic instead of the spectral path's fp32 tolerance: sed_tile at every width and row-tile count, the
    fall-backs onto payne_sed_kernel, every post kernel's way of consuming the magnitudes, the phot-only likelihood, F = 256,
    and the public API once.
Every comparison prints its worst |d| / bound (NOTES.md quotes them)."""
import numpy as np
import pytest

import oracle as O
from thepayne_amd import synth, nnio, _lib
from helpers import theta_full, yst_problem
from test_phot_shapes import (SHAPES, SATURATED, SAT_F, TILE_SHAPES, TILE_B, FALLBACK_H, POST_F, CAP, make_nets, shape_nets, sed_rows, bc_rows,
                              theta_rows, obs_phot, ref_sed, ref_bc, ref_theta, ref_lnl, check, build_planner, tile_cands, free_slots)

pytestmark = pytest.mark.gpu
EFLUX = 1e15
SPEC_H = 32


@pytest.fixture(scope="module")
def Engine():
    from thepayne_amd.engine import PayneEngine
    return PayneEngine


def _spectral_term(raw, obs, flux, th7):
    """The oracle's chi^2_spec of every row at eflux = 1e15."""
    return np.array([O.chi2_spec(O.genspec(raw, list(theta_full(t)[0, :8]), outwave=obs)[1], flux, np.full(len(obs), EFLUX)) for t in th7])


@pytest.fixture(scope="module")
def small():
    """The spectral side of the joint cases: yst_problem('small', H = 32) with eflux = 1e15, the 200 rows every case takes its first
    B of, and the proof that the spectrum does not count: the oracle's spectral term of every row is below 1e-20."""
    raw, obs, flux, _ = yst_problem("small", H=SPEC_H)
    thp, th7 = theta_rows(200)
    term = _spectral_term(raw, obs, flux, th7)
    assert np.all(term < 1e-20) and np.all(term >= 0.0), term.max()
    return dict(raw=raw, net=nnio.normalize_spec_net(raw), obs=(obs, flux, np.full(len(obs), EFLUX)), thp=thp, th7=th7)


def joint_theta(th7, thp, photscale):
    """ABI rows [B, 12]: the spectral columns of th7, the labels' NaN of thp, the photometric block log(A) | log(R), Dist, Av."""
    t = theta_full(th7)
    t[:, 0:4] = thp[:, 0:4]
    t[:, 8] = thp[:, 4]
    if not photscale:
        t[:, 9] = thp[:, 5]
    t[:, 10] = thp[:, 6]
    return t


class Joint(object):
    """One photometric model on the isolated spectrum: the reference's lnL and its bound for the rows, once."""

    def __init__(self, phot, thp, photscale):
        self.phot, self.photscale = phot, photscale
        self.op = obs_phot(phot)
        m, dm = ref_theta(phot, thp, photscale)
        self.lnl, self.dlnl = ref_lnl(m, dm, [v[0] for v in self.op.values()], [v[1] for v in self.op.values()])

    def engine(self, Engine, net, obs, **kw):
        return Engine(net, obs=obs, phot=self.phot, obs_phot=self.op, photscale=self.photscale, **kw)

    def check(self, what, lnl, rows=slice(None)):
        ref = self.lnl[rows]
        ok = np.isfinite(np.asarray(ref, dtype=np.float64))
        assert ok.sum() >= max(1, (len(ref) * 2) // 3), what               # (not a comparison of NaN with NaN)
        return check(what, lnl, ref, self.dlnl[rows])


# ---- 2. the stand-alone entry points ------------------------------------------------------------------------------------------
def _entry_points(Engine, what, phot):
    rows = sed_rows(phot)
    X = bc_rows(rows)
    eng = Engine(phot=phot, b_max=64)
    mags = eng.sed_batch(rows).cpu().numpy()
    bc = eng.bc_batch(X).cpu().numpy()
    assert eng.kernels_used()["sed"] == "payne_sed_kernel"
    m, dm = ref_sed(phot, rows)
    r1 = check(what + " payne_sed_batch", mags, m, dm, CAP)
    b, db = ref_bc(phot, X)
    r2 = check(what + " payne_bc_batch", bc, b, db, CAP)
    # the NaN row of the high-Av table shows at Av >= 5 only, and in payne_sed_batch only (fastANN.eval has no such branch)
    hi = ~(rows[:, 4] < 5.0)
    f = np.flatnonzero(np.isnan(phot["hiav"]).all(axis=1))
    if len(f):
        assert np.isnan(mags[hi][:, f]).all()
    assert np.array_equal(eng.sed_batch(rows).cpu().numpy().tobytes(), mags.tobytes()) and np.array_equal(eng.bc_batch(X).cpu().numpy().tobytes(), bc.tobytes())
    eng.close()
    return max(r1, r2)


@pytest.mark.parametrize("F,H", SHAPES, ids=["F%d-H%d" % s for s in SHAPES])
def test_entry_points_at_every_width_and_filter_count(Engine, F, H):
    """payne_sed_batch and payne_bc_batch on 40 rows (labels inside and outside the nets' range, Av in {0, 4.999, 5, 7.5, NaN}, Rv
    given and NaN, both magnitude formulae, a NaN label, no formula at all): inside the derived bound of the long-double reference,
    the same NaN pattern, the same bytes on a second call."""
    for phot in shape_nets(F, H):
        _entry_points(Engine, "F=%d H=%d" % (F, H), phot)


@pytest.mark.parametrize("H,k", SATURATED, ids=["H%d-x%d" % s for s in SATURATED])
def test_saturated_nets(Engine, small, H, k):
    """w1 times 400 and 3000: pre-activations beyond +-700 -- past sed_sigmoid_n's clamp, where exp() overflows and the sigmoid must be
    0 or 1 and never NaN -- through payne_sed_kernel (the entry points) and, joint, through the tile's own sigmoid (H = 16, 64;
    H = 20 takes the wave kernel there too)."""
    phot = make_nets(SAT_F, H, w1_factor=k)
    _entry_points(Engine, "saturated H=%d x%d" % (H, k), phot)
    B = 20
    J = Joint(make_nets(SAT_F, H, w1_factor=k, nan_row=False), small["thp"][:B], True)
    eng = J.engine(Engine, small["net"], small["obs"], b_max=64)
    lnl = eng.lnlike_batch(joint_theta(small["th7"][:B], small["thp"][:B], True)).cpu().numpy()
    assert (eng.kernels_used()["sed"] == "payne_sed_kernel") == (H == 20)
    J.check("saturated H=%d x%d joint" % (H, k), lnl)


def test_creation_limits(Engine):
    """hidden = 2049 (one past the ABI's maximum) and n_filters = 0 are refused at creation: PAYNE_E_INVALID and a message."""
    for F, H in ((1, 2049), (0, 16)):
        with pytest.raises(RuntimeError) as e:
            Engine(phot=make_nets(F, H, nan_row=False), b_max=8)
        assert "failed (%d)" % _lib.E_INVALID in str(e.value) and "phot.n_filters/hidden out of range" in str(e.value)
    Engine(phot=make_nets(1, 2048, nan_row=False), b_max=8).close()


# ---- 3. the joint likelihood's photometric half ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(tmp_path_factory.mktemp("sed_cands"))


def _tile_table(planner):
    """(F, H, B, cb) of every tile-form case on this device: the free workgroup slots as launch_hidden counts them, cb from
    sed_tile_cands itself (the stand-alone program of test_phot_shapes.py)."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [(F, H, B) for F, H in TILE_SHAPES for B in TILE_B]
    cbs = tile_cands(planner, [(B, F, free_slots(n_cu, B, SPEC_H)) for F, H, B in cases])
    return n_cu, [c + (cb,) for c, cb in zip(cases, cbs)]


def test_tile_cases_reach_every_body_of_the_tile(planner):
    """On this device's CU count the table below runs sed_tile with one, two and three row tiles (cb = 16, 32, 48), a last tile whose
    live rows are no multiple of 16, and more than one tile per filter.  A device on which it does not is a failure, not a skip."""
    n_cu, table = _tile_table(planner)
    seen = {cb for *_, cb in table}
    missing = [cb for cb in (16, 32, 48) if cb not in seen]
    assert not missing, "no case with cb in %s on %d CUs: %s" % (missing, n_cu, table)
    assert any((B % cb) % 16 != 0 for _, _, B, cb in table), "no partial last tile on %d CUs: %s" % (n_cu, table)
    assert any(B > cb for _, _, B, cb in table), "no case with more than one tile per filter on %d CUs: %s" % (n_cu, table)
    # ... and each of the three bodies meets a partial last tile and a second block
    for want in (16, 32, 48):
        assert any(cb == want and B % 16 != 0 for _, _, B, cb in table), (want, n_cu)
    assert any(cb == 48 and B > cb for _, _, B, cb in table) and any(cb == 16 and B > cb for _, _, B, cb in table), (n_cu, table)


@pytest.mark.parametrize("F,H", TILE_SHAPES, ids=["F%d-H%d" % s for s in TILE_SHAPES])
def test_tile_form_at_every_width_and_row_tile_count(Engine, small, planner, F, H):
    """sed_tile (riding in the hidden-layer launch) at H = 16 .. 64 -- idle waves, fewer k-steps and weight pieces than the tile's
    maximum -- and B = 1 .. 200: every row's lnL inside the bound of the reference's photometric chi^2, the NaN-label row NaN and its
    neighbours in the same 16-row tile correct."""
    _, table = _tile_table(planner)
    cb_of = {(f, h, b): cb for f, h, b, cb in table}
    worst = 0.0
    for photscale in ((True, False) if (F, H) in TILE_SHAPES[:3] else (True,)):
        J = Joint(make_nets(F, H, nan_row=False), small["thp"], photscale)
        eng = J.engine(Engine, small["net"], small["obs"], b_max=256)
        th = joint_theta(small["th7"], small["thp"], photscale)
        for B in TILE_B:
            lnl = eng.lnlike_batch(th[:B]).cpu().numpy()
            assert eng.kernels_used()["sed"] != "payne_sed_kernel" and eng.kernels_used()["hidden"]
            worst = max(worst, J.check("tile F=%d H=%d photscale=%d B=%d cb=%d" % (F, H, photscale, B, cb_of[(F, H, B)]), lnl, slice(0, B)))
            if B > 6:
                assert np.isnan(lnl[5]) and np.isfinite(lnl[:5]).all() and np.isfinite(lnl[6:min(B, 16)]).all()
        eng.close()
    print("tile F=%d H=%d: worst |dlnL| / bound = %.3g" % (F, H, worst))


def _two_layer(net):
    (W0, b0, a0), _, (W2, b2, _) = net["layers"]
    out = dict(net)
    out["layers"] = [(W0, b0, a0), (W2, b2, _lib.ACT_NONE)]
    return out


def test_fall_backs_onto_the_wave_kernel(Engine, small):
    """Where the tile does not apply the likelihood launches payne_sed_kernel itself: H = 15, 20, 80 (sed_tile_ok says no), H = 32 with
    PAYNE_V_SED_OWN_LAUNCH, and H = 32 beside a two-layer spectral net (no hidden-layer launch to ride in).  The same rows as the tile
    cases; at H = 32 the two routes agree within twice the bound.  This net keeps the NaN row of its high-Av table: rows at Av >= 5
    are NaN on both routes."""
    B = 40
    thp, th7 = small["thp"][:B], small["th7"][:B]
    th = joint_theta(th7, thp, True)
    for H in FALLBACK_H:
        J = Joint(make_nets(7, H, nan_row=False), thp, True)
        eng = J.engine(Engine, small["net"], small["obs"], b_max=64)
        lnl = eng.lnlike_batch(th).cpu().numpy()
        assert eng.kernels_used()["sed"] == "payne_sed_kernel"
        J.check("fall-back H=%d" % H, lnl)
    for nan_row in (False, True):
        phot = make_nets(7, 32, nan_row=nan_row)
        m, dm = ref_theta(phot, thp, True)
        op = obs_phot(phot)
        ref, dref = ref_lnl(m, dm, [v[0] for v in op.values()], [v[1] for v in op.values()])
        kw = dict(obs=small["obs"], phot=phot, obs_phot=op, photscale=True, b_max=64)
        got = {}
        for what, net, variant in (("tile", small["net"], 0), ("own launch", small["net"], _lib.V_SED_OWN_LAUNCH), ("two-layer net", _two_layer(small["net"]), 0)):
            eng = Engine(net, variant=variant, **kw)
            got[what] = eng.lnlike_batch(th).cpu().numpy()
            assert (eng.kernels_used()["sed"] == "payne_sed_kernel") == (what != "tile"), (what, eng.kernels_used())
            if what == "two-layer net":                          # the oracle has no such net: the isolation on the device's own spectra
                sp = eng.predict_batch(th, stage=2, fwhm_R=True).cpu().numpy().astype(np.float64)
                ok = np.isfinite(sp).all(axis=1)
                assert ok.sum() >= B - 1 and np.all((((sp[ok] - small["obs"][1]) / EFLUX) ** 2).sum(axis=1) < 1e-20)
            check("H=32 %s%s" % (what, " (NaN row)" if nan_row else ""), got[what], ref, dref)
            eng.close()
        assert np.isnan(got["tile"]).sum() == (1 + np.sum(~(thp[:, 6] < 5.0) & ~np.isnan(thp[:, 2])) if nan_row else 1)
        ok = np.isfinite(got["tile"])
        for what in ("own launch", "two-layer net"):
            assert np.all(np.abs(got[what][ok] - got["tile"][ok]) <= 2.0 * dref[ok]), what


@pytest.mark.parametrize("F", POST_F)
@pytest.mark.parametrize("variant", [0, _lib.V_POST_FULL], ids=["lean", "full"])
def test_post_kernel_consumes_every_filter(Engine, small, F, variant):
    """The post kernel's one-lane-per-filter terms (F <= 64) and the serial sum (F > 64), up to the 255 filters its packed arguments
    hold, in the likelihood-only instantiation and the full one (PAYNE_V_POST_FULL); B = 33."""
    B = 33
    J = Joint(make_nets(F, 16, nan_row=False), small["thp"][:B], True)
    eng = J.engine(Engine, small["net"], small["obs"], b_max=64, variant=variant)
    lnl = eng.lnlike_batch(joint_theta(small["th7"][:B], small["thp"][:B], True)).cpu().numpy()
    assert (eng.kernels_used()["post"].count(",") == 2) == (variant == 0), eng.kernels_used()      # payne_post_kernel<LOG2N, TW_LDS[, LEAN]>
    J.check("post kernel (%s) F=%d" % ("full" if variant else "lean", F), lnl)


def test_lsf_chunks_read_the_magnitudes_at_their_offset(Engine, small):
    """An LSF vector bound, the global-memory form (256 candidates a launch) and a batch of 300: the second launch reads the
    magnitudes at `off * F` -- F = 5 here (the construction of test_gpu_parity's LSF-chunk test, where F = 7)."""
    B, F = 300, 5
    thp, th7 = theta_rows(B, seed=12)
    obs = small["obs"][0]
    J = Joint(make_nets(F, 16, nan_row=False), thp, True)
    eng = J.engine(Engine, small["net"], small["obs"], b_max=320, variant=_lib.V_LSF_GLOBAL)
    eng.set_lsf(0.075 * (1.0 + 0.3 * (obs - obs.mean()) / (obs.max() - obs.min())))
    term = _spectral_term(small["raw"], obs, small["obs"][1], th7[250:])      # (without the LSF: any spectrum within a few units of the data does)
    assert np.all(term < 1e-20)
    lnl = eng.lnlike_batch(joint_theta(th7, thp, True)).cpu().numpy()
    assert "lsf" in eng.kernels_used()["post"]
    J.check("LSF chunks F=%d B=%d" % (F, B), lnl)
    J.check("LSF chunks F=%d, second launch" % F, lnl[256:], slice(256, B))


@pytest.mark.parametrize("npix,nobs,lam0,R,B,variant,kernel", [(32768, 30000, 4500.0, 60000.0, 5, 0, "payne_post_chip2_kernel"),
                                                               (40000, 30000, 5150.0, 32000.0, 3, 0, "payne_post_chip_kernel"),
                                                               (40000, 30000, 5150.0, 32000.0, 3, _lib.V_BIG_WORKSPACE, "payne_post_big_kernel")],
                         ids=["chip2", "chip", "big"])
def test_kernels_for_spectra_larger_than_lds_consume_the_magnitudes(Engine, npix, nobs, lam0, R, B, variant, kernel):
    """The grids of test_gpu_parity's test_spectra_larger_than_lds_vs_oracle: 32 768 points (payne_post_chip2_kernel, two candidates a
    workgroup, b_max = 2 < B: an odd batch walked in chunks) and 40 000 pixels (payne_post_chip_kernel, and payne_post_big_kernel with
    its workspace in global memory), F = 3, H = 32."""
    raw = synth.make_yst_net(npix=npix, lam0=lam0, R_fwhm=R, H=16, seed=31, line_depth=0.1)
    obs = synth.obs_grid(raw["wavelength"], nobs, inset=0.0005, relative=True)
    flux = np.ones(nobs)
    thp = theta_rows(5, seed=9)[0][:B]
    th7 = synth.draw_candidates(B, seed=npix)
    th7[:, :4] = thp[:, :4]
    th7[:, 6] = np.linspace(0.6, 0.85, B) * R
    th7[1, 5] = 0.0
    assert np.all(_spectral_term(raw, obs, flux, th7[:2]) < 1e-20)
    J = Joint(make_nets(3, 32, nan_row=False), thp, True)
    eng = J.engine(Engine, nnio.normalize_spec_net(raw), (obs, flux, np.full(nobs, EFLUX)), b_max=2, variant=variant)
    lnl = eng.lnlike_batch(joint_theta(th7, thp, True)).cpu().numpy()
    assert eng.kernels_used()["post"] == kernel, eng.kernels_used()
    J.check("%s F=3 H=32 B=%d" % (kernel, B), lnl)


@pytest.mark.parametrize("F", [1, 65])
def test_phot_only_likelihood(Engine, F):
    """No spectral model (spec=False fits): payne_sed_kernel and payne_photonly_kernel, B on both sides of its 128-thread blocks."""
    thp, th7 = theta_rows(129, seed=4)
    for photscale in (True, False):
        J = Joint(make_nets(F, 16, nan_row=False), thp, photscale)
        eng = Engine(phot=J.phot, obs_phot=J.op, photscale=photscale, b_max=256)
        th = joint_theta(th7, thp, photscale)
        for B in (1, 127, 128, 129):
            J.check("phot-only F=%d photscale=%d B=%d" % (F, photscale, B), eng.lnlike_batch(th[:B]).cpu().numpy(), slice(0, B))
        assert eng.kernels_used()["sed"] == "payne_sed_kernel"
        eng.close()


def test_256_filters(Engine, small):
    """One filter more than the post kernel's packed arguments hold (8 bits).  payne_sed_batch and the phot-only likelihood have no
    such limit and are correct; the JOINT likelihood REFUSES the call (RuntimeError: '... filters beyond what the post kernel's packed
    arguments hold') -- pinned here: a refusal, never a number from the first 0 filters."""
    F, B = 256, 20
    phot = make_nets(F, 16)
    _entry_points(Engine, "F=256 H=16", phot)
    thp, th7 = small["thp"][:B], small["th7"][:B]
    J = Joint(make_nets(F, 16, nan_row=False), thp, True)
    th = joint_theta(th7, thp, True)
    eng = Engine(phot=J.phot, obs_phot=J.op, photscale=True, b_max=64)
    J.check("phot-only F=256", eng.lnlike_batch(th).cpu().numpy())
    eng.close()
    eng = J.engine(Engine, small["net"], small["obs"], b_max=64)
    with pytest.raises(RuntimeError, match="filters beyond what the post kernel's packed arguments hold"):
        eng.lnlike_batch(th)
    eng.close()


def test_public_api_at_another_shape():
    """FastPayneSEDPredict(usebands=, nnpath=dict).sed and GenMod.genphot / genphot_scaled at (F, H) = (3, 48)."""
    from thepayne_amd.predict.predictsed import FastPayneSEDPredict
    from thepayne_amd.fitting.genmod import GenMod
    phot = make_nets(3, 48)
    S = FastPayneSEDPredict(usebands=phot["filters"], nnpath=phot)
    rows = sed_rows(phot)[:20]
    m, dm = ref_sed(phot, rows)
    got = np.array([S.sed(logt=r[0], logg=r[1], feh=r[2], afe=r[3], av=r[4], rv=r[5], logl=None if np.isnan(r[6]) else r[6],
                          dist=None if np.isnan(r[7]) else r[7], logA=None if np.isnan(r[8]) else r[8]) for r in rows])
    check("FastPayneSEDPredict.sed", got, m, dm, CAP)
    GM = GenMod()
    GM._initphotnn(phot["filters"], nnpath=phot)
    thp = theta_rows(200)[0][:12]
    for photscale in (False, True):
        m, dm = ref_theta(phot, thp, photscale)
        fn = GM.genphot_scaled if photscale else GM.genphot
        got = np.array([[fn(list(t[:4]) + ([t[4], t[6]] if photscale else [t[4], t[5], t[6]]))[f] for f in phot["filters"]] for t in thp])
        check("GenMod.genphot%s" % ("_scaled" if photscale else ""), got, m, dm, CAP)
