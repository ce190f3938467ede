"""The C2 post kernel asks for a thread's observed-pixel records in front of the instrumental stage's FORWARD transform
(post_seq.hpp stage_and_obs) instead of in front of the inverse one.  A request is not arithmetic: the likelihoods must be what
the build before that change gave, TO THE BIT -- on the path that took the change and on each fall-back beside it that did not:

  c2      the headline problem: 4096-point window, 3600 observed pixels, no blaze     -> stage_and_obs
  blaze   the same with a three-term Chebyshev blaze in theta (npoly = 3)             -> conv_stage + the general loop
  sparse  2500 observed pixels: whole blocks of records would be 39 % padding
          (obs_fast_ok is false)                                                       -> conv_stage + the general loop

tests/golden/g16_obs_records_ahead.npz holds the values of the commit before the change, written by that commit's library on an
MI355X with `python tests/test_obs_records_ahead_gpu.py OUT.npz` (no variant bit of one library can switch a request site off
without a second instantiation of the kernel, so the earlier build itself is the reference).  The kernels are deterministic and
every rounding in them is written out, so the comparison is `array_equal`, not a tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu
CASES = ("c2", "blaze", "sparse")


def _theta_full(theta7, npoly=0, pc=None):
    theta7 = np.atleast_2d(theta7)
    out = np.full((len(theta7), 8 + npoly + 4), np.nan)
    out[:, 0:6] = theta7[:, 0:6]
    out[:, 7] = theta7[:, 6]
    if npoly:
        out[:, 8:8 + npoly] = pc
    return out


def problem(case):
    """(Engine keyword arguments, theta rows) of one case; everything from the C2 network and the reference's C2 golden vectors."""
    from thepayne_amd import synth, nnio
    g = np.load(os.path.join(GOLDEN, "g4_lnlike_c2.npz"), allow_pickle=False)
    cfg = synth.CONFIGS["C2"]
    net = nnio.normalize_spec_net(synth.make_yst_net(npix=cfg["npix"], lam0=cfg["lam0"], R_fwhm=cfg["R"], seed=0), "YST1")
    obs = (g["obs_wave"], g["obs_flux"], g["obs_eflux"])
    if case == "c2":
        return dict(spec_net=net, obs=obs, b_max=512), _theta_full(g["theta"])
    if case == "blaze":
        n = 128
        k = np.arange(n)
        pc = np.column_stack([1.0 + 1e-3 * np.cos(k), 0.02 * np.sin(0.7 * k), -0.01 * np.cos(1.3 * k)])
        return dict(spec_net=net, obs=obs, npoly=3, b_max=n), _theta_full(g["theta"][:n], npoly=3, pc=pc)
    if case == "sparse":
        nobs = 2500
        assert 2 * (4096 - nobs) > nobs                      # obs_fast_ok(T, 8 * 512) is false
        sel = np.round(np.linspace(0, len(g["obs_wave"]) - 1, nobs)).astype(int)
        return dict(spec_net=net, obs=tuple(a[sel] for a in obs), b_max=128), _theta_full(g["theta"][:128])
    raise KeyError(case)


def evaluate(case):
    from thepayne_amd.engine import PayneEngine
    kw, th = problem(case)
    eng = PayneEngine(**kw)
    lnl = eng.lnlike_batch(th).cpu().numpy()
    used = eng.kernels_used()
    eng.close()
    return lnl, used


@pytest.mark.parametrize("case", CASES)
def test_likelihoods_are_those_of_the_build_before_the_early_request(case):
    ref = np.load(os.path.join(GOLDEN, "g16_obs_records_ahead.npz"), allow_pickle=False)[case]
    lnl, used = evaluate(case)
    assert used["post"] == "payne_post_kernel<12, true, true>", used     # the likelihood-only C2 kernel, every case
    assert np.isfinite(ref).sum() >= len(ref) - 4             # (the reference itself is a set of real likelihoods)
    same = (lnl == ref) | (np.isnan(lnl) & np.isnan(ref))
    print(case, "candidates:", len(ref), "differing:", int((~same).sum()),
          "max |d|:", float(np.nanmax(np.abs(lnl - ref))) if len(ref) else 0.0)
    assert same.all(), (case, int((~same).sum()), np.flatnonzero(~same)[:8])


if __name__ == "__main__":                                    # writes the reference values with whatever library is loaded
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **{c: evaluate(c)[0] for c in CASES})
