"""The quick-look classes of Payne/fitting/fitutils.py (RVcalc, BROADcalc, PCcalc, SEDopt) -- what runs without a GPU:
the import names, the host-only polynomial fit against the reference's frozen result (g17, tools/freeze_quicklook_golden.py),
the arithmetic of the two scan kernels (csrc/quicklook_core.hpp) executed on the host under ASan / UBSan, and the argument
errors of the two scans.  The kernels themselves: tests/test_quicklook_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOBS = (1, 63, 257)


def below_reference(rows, n, flux, eflux, threshold):
    """BROADcalc.chisq_broad's tail in numpy, with the reference's pairing: the kept model values and the kept fluxes against
    the FIRST n_kept entries of the unmasked error vector."""
    chisq, kept = [], []
    for row in rows:
        m = row[:n].astype(np.float64)
        with np.errstate(invalid="ignore"):
            cond = m < threshold
        mk, fk = m[cond], flux[:n][cond]
        ek = eflux[:len(mk)]
        chisq.append(np.sum((mk - fk) ** 2 / ek ** 2))
        kept.append(len(mk))
    return np.array(chisq), np.array(kept, dtype=np.int32)


def below_cases():
    """(rows fp32 [G, ld], n, flux, eflux) for n in {1, 64, 1000}, ld > n: rows with NaN runs at both ends, scattered NaNs, a row
    with nothing kept, a row with everything kept; the padding beyond n holds values below the threshold that must not count."""
    rng = np.random.default_rng(17)
    out = []
    for n in (1, 64, 1000):
        ld = n + 7
        rows = rng.uniform(0.6, 1.05, (6, ld)).astype(np.float32)
        rows[1, :n] = 1.0                                   # nothing kept
        rows[2, :n] = 0.5                                   # everything kept
        rows[3, :min(n, 70)] = np.nan                       # NaN runs at both ends (all of the row for n <= 70)
        rows[3, max(0, n - 70):n] = np.nan
        rows[4, :n][rng.random(n) < 0.3] = np.nan           # scattered NaNs
        rows[5, :n] = np.nan                                # only NaN: nothing kept
        rows[:, n:] = 0.1
        flux = rng.uniform(0.6, 1.0, n)
        eflux = 0.003 * 10.0 ** rng.uniform(0.0, 2.0, n)
        out.append((rows, n, flux, eflux))
    return out


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """tests/emul/quicklook_emul.cpp built with the sanitizers; returns run(mode, arrays..., args) -> the files it wrote."""
    build = tmp_path_factory.mktemp("quicklook_emul")
    exe = str(build / "quicklook_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "emul", "quicklook_emul.cpp")],
                   check=True)
    count = [0]

    def run(mode, arrays, args):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        for name, a in arrays.items():
            np.ascontiguousarray(a).tofile(str(d / (name + ".bin")))
        res = subprocess.run([exe, mode, str(d)] + [repr(a) for a in args], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        return d
    return run


def test_reference_import_names_resolve_to_this_build():
    from Payne.fitting.fitutils import RVcalc, BROADcalc, PCcalc, SEDopt
    import thepayne_amd.fitting.fitutils as fu
    assert (RVcalc, BROADcalc, PCcalc, SEDopt) == (fu.RVcalc, fu.BROADcalc, fu.PCcalc, fu.SEDopt)
    assert all(c.__module__ == "thepayne_amd.fitting.fitutils" for c in (RVcalc, BROADcalc, PCcalc, SEDopt))
    assert {"RVcalc", "BROADcalc", "PCcalc", "SEDopt", "polycalc"} <= set(fu.__all__)


@pytest.mark.parametrize("numpoly", [2, 4])
def test_pccalc_reaches_the_minimum_the_reference_reaches(golden, numpoly):
    """Nelder-Mead's path depends on rounding, its end point does not: the result lies as close to the closed-form weighted
    least-squares minimiser as the reference's own run does (delta_ref, times 4 for two runs stopping on opposite sides, floor
    1e-9), and its chi^2 is no worse than the reference's at the reference's result."""
    from thepayne_amd.fitting.fitutils import PCcalc
    g = golden("g17_quicklook")
    k = "pc%d_" % numpoly
    P = PCcalc(inwave=g[k + "wave"], influx=g[k + "flux"], einflux=g[k + "eflux"], modflux=g["rv_modflux_clean"],
               modwave=g["rv_modwave"], numpoly=numpoly)
    out = P()
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == (numpoly,)
    delta_ref = np.linalg.norm(g[k + "ref"] - g[k + "exact"])
    delta = np.linalg.norm(out[0] - g[k + "exact"])
    chisq = P.chisq_pc(out[0])
    print("numpoly %d: delta %.3g, delta_ref %.3g, chisq %.17g, reference %.17g" % (numpoly, delta, delta_ref, chisq, float(g[k + "ref_chisq"])))
    assert delta <= max(4.0 * delta_ref, 1e-9)
    assert chisq <= float(g[k + "ref_chisq"]) * (1 + 1e-9)
    # the objective itself, at the reference's result
    assert abs(P.chisq_pc(g[k + "ref"]) - float(g[k + "ref_chisq"])) <= 1e-9 * float(g[k + "ref_chisq"])


@pytest.mark.parametrize("nobs", NOBS)
def test_velocity_scan_arithmetic_on_the_host(emul, golden, nobs):
    """quicklook_core.hpp's interpolate-and-sum, thread by thread in the kernel's order, against the reference's chisq_rv on
    the whole grid: relative 1e-10 (reordering a sum of <= 300 positive terms costs <= 300 * 2^-53 ~ 3e-14; the cancellation
    in m - o amplifies the interpolation's rounding by <= 1e3 on these inputs), NaN where the reference is NaN."""
    g = golden("g17_quicklook")
    rv, ref = g["rv_grid"], g["rv%d_chisq" % nobs]
    d = emul("rv", dict(modwave=g["rv_modwave"], modflux=g["rv_modflux"], wave=g["rv%d_wave" % nobs], flux=g["rv%d_flux" % nobs],
                        eflux=g["rv%d_eflux" % nobs], rv=rv), [len(g["rv_modwave"]), nobs, len(rv)])
    got = np.fromfile(str(d / "chisq.bin"))
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    rel = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    print("nobs %d: max relative difference %.3g at rv %g" % (nobs, rel.max(), rv[fin][rel.argmax()]))
    assert np.all(rel <= 1e-10), (nobs, rv[fin][rel > 1e-10])


def test_compaction_arithmetic_on_the_host(emul, golden):
    """The ballot / prefix-count compaction and its chi^2 against numpy: synthetic rows (NaN runs, nothing kept, everything
    kept; one chunk, exactly one wave, several chunks) and the reference's broadened rows of g17 rounded to fp32."""
    g = golden("g17_quicklook")
    cases = below_cases() + [(g["br_rows"].astype(np.float32), g["br_rows"].shape[1], g["br_flux"], g["br_eflux"])]
    for rows, n, flux, eflux in cases:
        ref_chisq, ref_kept = below_reference(rows, n, flux, eflux, 0.95)
        d = emul("below", dict(rows=rows, flux=flux, eflux=eflux), [rows.shape[1], n, rows.shape[0], 0.95])
        chisq, kept = np.fromfile(str(d / "chisq.bin")), np.fromfile(str(d / "kept.bin"), dtype=np.int32)
        assert np.array_equal(kept, ref_kept), n
        assert np.all(np.abs(chisq - ref_chisq) <= 1e-12 * np.abs(ref_chisq)), n
    assert np.array_equal(below_reference(g["br_rows"].astype(np.float32), 1024, g["br_flux"], g["br_eflux"], 0.95)[1], g["br_kept"])


def test_scan_argument_errors(golden):
    """What the two scans refuse before any GPU work: a model grid that does not increase, an observed spectrum that is not on
    the model's grid (BROADcalc masks it with the model's pixels)."""
    from thepayne_amd.fitting.fitutils import RVcalc, BROADcalc
    g = golden("g17_quicklook")
    mw, mf = g["rv_modwave"], g["rv_modflux_clean"]
    w, f, e = g["rv63_wave"], g["rv63_flux"], g["rv63_eflux"]
    bad = mw.copy()
    bad[10] = bad[9]
    with pytest.raises(ValueError):
        RVcalc(inwave=w, influx=f, einflux=e, modflux=mf, modwave=bad).scan([0.0])
    with pytest.raises(ValueError):
        RVcalc(inwave=w, influx=f, einflux=e, modflux=mf, modwave=mw[::-1].copy()).chisq_rv(0.0)
    with pytest.raises(ValueError):
        RVcalc(inwave=w, influx=f[:-1], einflux=e, modflux=mf, modwave=mw).scan([0.0])
    with pytest.raises(ValueError):                                  # 63 observed pixels against 1000 model pixels
        BROADcalc(inwave=w, influx=f, einflux=e, modflux=mf, modwave=mw, modres=1e5).scan([5e4])
    with pytest.raises(ValueError):                                  # the right length on another grid
        BROADcalc(inwave=mw + 0.01, influx=mf, einflux=np.full(len(mw), 0.01), modflux=mf, modwave=mw, modres=1e5).scan([5e4])
    with pytest.raises(ValueError):
        BROADcalc(inwave=bad, influx=mf, einflux=np.full(len(mw), 0.01), modflux=mf, modwave=bad, modres=1e5).chisq_broad(5e4)
    # values outside [0, modres) are inf without any GPU work (fitutils.py:138-141)
    B = BROADcalc(inwave=mw, influx=mf, einflux=np.full(len(mw), 0.01), modflux=mf, modwave=mw, modres=1e5)
    assert np.all(np.isinf(B.scan([-1.0, 1e5, 2e5]))) and B.chisq_broad(-3.0) == np.inf


def test_fits_name_scipy_when_it_is_missing(monkeypatch, golden):
    import sys
    from thepayne_amd.fitting.fitutils import PCcalc
    g = golden("g17_quicklook")
    P = PCcalc(inwave=g["pc2_wave"], influx=g["pc2_flux"], einflux=g["pc2_eflux"], modflux=g["rv_modflux_clean"],
               modwave=g["rv_modwave"], numpoly=2)
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.delitem(sys.modules, "scipy.optimize", raising=False)
    with pytest.raises(ImportError, match="scipy"):
        P()
