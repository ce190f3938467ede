"""payne_tmatch_match_pairs on the host (thepayne_amd/csrc/tmatch_pair_core.hpp through tests/emul/tmatch_pair_emul.cpp, built with
ASan + UBSan): the chi^2 of every (star, primary, template) inside the derived bound of the long double solve and direct sum, the NaN
rules, the lists and their edge cases, the recovery of a planted pair; fitting/tmatch.py's and optfit.py's host side (the argument
checks of ``match_pairs`` and ``fit_binary_from_bank``); and the inputs of the end-to-end test on the g20 fixture network, whose
reference loop runs here.  tests/test_tmatch_pair_gpu.py runs the same inputs through the library."""
import os
import subprocess

import numpy as np
import pytest

from thepayne_amd import _lib
from test_lmfit import CONVERGED, RECOVERY_MAX_EVALS, sigma_distance
from test_tmatch import CHUNK, TOPKS, U, check_lists, match_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 64                                            # payne_tmatch_pair_rows(); payne_tmatch_pair_chunk() is CHUNK
SHAPE_N_PIX = (1, 2, 5, 37, 1000)
SHAPE_NK = ((1, 1), (5, 3), (23, 3), (5, 16))        # (N, kA); 23 x 3 = 69 rows: star 21 straddles the 64-row tile boundary
SHAPE_M = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
COLLINEAR = 2.0 ** -20
L = np.longdouble


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def pair_case(rng, N, M, n, kA, ld_t=None, ld_f=None):
    """test_tmatch.match_case's templates, weights and NaN rules; each star's flux is c (0.7 m_a + 0.3 m_b) plus its noise, c in
    [0.8, 1.6], a != b where M > 1.  cand int32 [N, kA] is numpy's single-template-with-scale ranking (shortlist_numpy).  Returns
    (templates, flux, w, cand, truth [N, 2])."""
    templates, flux, w = match_case(rng, N, M, n, ld_t=ld_t, ld_f=ld_f)
    a = rng.integers(0, M, N)
    b = (a + 1 + rng.integers(0, max(M - 1, 1), N)) % M
    c = rng.uniform(0.8, 1.6, N)
    ok = w[:, :n] != 0.0
    sigma = np.where(ok, 1.0 / np.sqrt(np.where(ok, w[:, :n], 1.0)), 0.0)
    ta, tb = (np.where(np.isfinite(templates[i, :n]), templates[i, :n], 0.0).astype(np.float64) for i in (a, b))
    mix = c[:, None] * (0.7 * ta + 0.3 * tb) + sigma * rng.normal(size=(N, n))
    flux[:, :n] = np.where(ok, mix, np.nan).astype(np.float32)
    return templates, flux, w, shortlist_numpy(templates, flux, w, n, kA), np.stack([a, b], axis=1)


def sums64(templates, flux, w, n):
    """(ok [N, n], f, ww [N, n] zero where the pixel does not count, T [M, n] zero where not finite, poisoned [N, M]) in fp64."""
    ok = w[:, :n] != 0.0
    f = np.where(ok, flux[:, :n], 0.0).astype(np.float64)
    ww = np.where(ok, w[:, :n], 0.0)
    fin = np.isfinite(templates[:, :n])
    T = np.where(fin, templates[:, :n], 0.0).astype(np.float64)
    return ok, f, ww, T, (ok.astype(np.int64) @ (~fin).astype(np.int64).T) > 0


def shortlist_numpy(templates, flux, w, n, kA):
    """The kA templates of lowest c0 - B^2 / S per star (one template with a free scale), fp64, stable; -1 where fewer qualify."""
    ok, f, ww, T, poisoned = sums64(templates, flux, w, n)
    B, S = (ww * f) @ T.T, ww @ (T * T).T
    with np.errstate(all="ignore"):
        chi = np.where(poisoned | ~(S > 0.0), np.nan, (ww * f * f).sum(axis=1)[:, None] - B * B / S)
    cand = np.full((flux.shape[0], kA), -1, dtype=np.int32)
    for s in range(flux.shape[0]):
        order = np.argsort(chi[s], kind="stable")
        order = order[~np.isnan(chi[s][order])][:kA]
        cand[s, :len(order)] = order
    return cand


# ---- the long double reference ---------------------------------------------------------------------------------------------------------
def reference(templates, flux, w, n, cand):
    """Per (star, slot, template) in long double: (alpha, beta) from the normal equations with one refinement step, chi^2 as the direct
    sum of w (f - alpha m_a - beta m_b)^2, NaN by the rules of include/payne_hip.h, the bound (2 n + 16) 2^-53 S_p with
    S_p = sum w f^2 + 2 (|alpha| sum |w f m_a| + |beta| sum |w f m_b|) + alpha^2 Sa + 2 |alpha beta| |X| + beta^2 Sb, and which pairs are
    borderline: |D / (Sa Sb) - 2^-20| < 1e-9 or min(alpha, beta) / (alpha + beta) within +-1e-9.
    Returns dict(chi, bound, alpha, beta [N, kA, M] long double, borderline bool)."""
    N, kA = cand.shape
    M = templates.shape[0]
    ok, f, ww, T, poisoned = sums64(templates, flux, w, n)
    f, ww, T = f.astype(L), ww.astype(L), T.astype(L)
    out = dict(chi=np.full((N, kA, M), np.nan, dtype=L), bound=np.zeros((N, kA, M), dtype=L), alpha=np.full((N, kA, M), np.nan, dtype=L),
               beta=np.full((N, kA, M), np.nan, dtype=L), borderline=np.zeros((N, kA, M), dtype=bool))
    with np.errstate(all="ignore"):
        for s in range(N):
            wf = ww[s] * f[s]
            c0 = (wf * f[s]).sum()
            B, S, absB = T @ wf, (T * T) @ ww[s], np.abs(T) @ np.abs(wf)
            for j in range(kA):
                a = int(cand[s, j])
                if not (0 <= a < M):
                    continue
                ma = T[a]
                X = T @ (ww[s] * ma)
                D = S[a] * S - X * X
                al, be = (B[a] * S - B * X) / D, (B * S[a] - B[a] * X) / D
                r = f[s][None, :] - al[:, None] * ma[None, :] - be[:, None] * T
                ga, gb = (r * ma[None, :]) @ ww[s], (r * T) @ ww[s]
                al, be = al + (ga * S - gb * X) / D, be + (gb * S[a] - ga * X) / D
                r = f[s][None, :] - al[:, None] * ma[None, :] - be[:, None] * T
                chi = (r * r) @ ww[s]
                earlier = np.isin(np.arange(M), cand[s, :j])
                base = ~(poisoned[s] | poisoned[s, a] | earlier | (np.arange(M) == a)) & (S[a] > 0) & (S > 0)
                valid = base & (D > L(COLLINEAR) * S[a] * S) & (al > 0) & (be > 0) & np.isfinite(chi)
                near = np.abs(D / (S[a] * S) - L(COLLINEAR)) < 1e-9
                near |= (D > L(COLLINEAR) * S[a] * S) & (np.abs(np.minimum(al, be) / (al + be)) < 1e-9)
                out["borderline"][s, j] = base & near
                Sp = c0 + 2.0 * (np.abs(al) * absB[a] + np.abs(be) * absB) + al * al * S[a] + 2.0 * np.abs(al * be) * np.abs(X) + be * be * S
                out["chi"][s, j] = np.where(valid, chi, np.nan)
                out["alpha"][s, j], out["beta"][s, j] = np.where(valid, al, np.nan), np.where(valid, be, np.nan)
                out["bound"][s, j] = np.where(valid, (2 * n + 16) * L(U) * Sp, 0.0)
    return out


def check_values(every, ref, what):
    """every [N, kA, M] inside the bound of the reference; NaN exactly where the reference is, except at borderline pairs, of which
    there may be at most 1 %."""
    border = ref["borderline"]
    nan = np.isnan(ref["chi"])
    assert border.sum() <= 0.01 * border.size, (what, int(border.sum()), border.size)
    assert np.array_equal(np.isnan(every)[~border], nan[~border]), (what, np.argwhere((np.isnan(every) != nan) & ~border)[:5])
    both = ~nan & ~np.isnan(every)
    err, bound = np.abs(every.astype(L) - ref["chi"])[both], ref["bound"][both]
    some = bound > 0
    ratio = float((err[some] / bound[some]).max()) if some.any() else 0.0
    print("%s: max |dchi2| / bound = %.3g over %d pairs, %d borderline" % (what, ratio, int(both.sum()), int(border.sum())))
    assert np.all(err <= bound), (what, ratio)
    return ratio


def own_lists(every, cand, k):
    """The lists a stable sort of every [N, kA, M] in (chi^2, j, b) gives: (idx_a, idx_b int32 [N, k], chisq [N, k], flat [N, k])."""
    N, kA, M = every.shape
    idx_a, idx_b, flat = (np.full((N, k), -1, dtype=np.int32) for _ in range(3))
    chisq = np.full((N, k), np.inf)
    for s in range(N):
        row = every[s].reshape(-1)
        order = np.argsort(row, kind="stable")
        order = order[~np.isnan(row[order])][:k]
        flat[s, :len(order)], chisq[s, :len(order)] = order, row[order]
        idx_a[s, :len(order)], idx_b[s, :len(order)] = cand[s, order // M], order % M
    return idx_a, idx_b, chisq, flat


def check_pair_lists(got, cand, ref, n, what):
    """idx_a, idx_b, chisq exactly the stable sort of the own rows; the amplitudes NaN exactly in the empty slots and within
    (2 n + 16) 2^-53 2^22 (|alpha| + |beta|) of the reference's (the sums' relative error times the condition number that the
    collinearity rule admits, (1 + cos) / (1 - cos) < 4 / 2^-20); against the reference's lists as test_tmatch.check_lists does."""
    N, kA, M = got["all"].shape
    k = got["idx_a"].shape[1]
    idx_a, idx_b, chisq, flat = own_lists(got["all"], cand, k)
    assert np.array_equal(got["idx_a"], idx_a) and np.array_equal(got["idx_b"], idx_b) and np.array_equal(got["chisq"], chisq), what
    empty = idx_b < 0
    assert np.all(np.isnan(got["amp"][empty])) and np.all(got["amp"][~empty] > 0.0), what
    for s in range(N):
        for e in np.flatnonzero(~empty[s]):
            j, b = divmod(int(flat[s, e]), M)
            want = np.array([ref["alpha"][s, j, b], ref["beta"][s, j, b]], dtype=np.float64)
            if np.all(np.isfinite(want)):
                assert np.all(np.abs(got["amp"][s, e] - want) <= (2 * n + 16) * U * 2.0 ** 22 * np.abs(want).sum()), (what, s, e, got["amp"][s, e], want)
    return check_lists(flat, got["chisq"], got["all"].reshape(N, kA * M), ref["chi"].reshape(N, kA * M), ref["bound"].reshape(N, kA * M), what)


def shape_cases(n, NK):
    """The template counts and top-k of one (n, (N, kA)): every M; topk walks 1, 3, 8 so that over the grid every (M, topk) occurs."""
    start = SHAPE_N_PIX.index(n) + SHAPE_NK.index(NK)
    return [(M, TOPKS[(start + j) % 3]) for j, M in enumerate(SHAPE_M)]


# ---- the emulator -------------------------------------------------------------------------------------------------------------------
KEYS = ("idx_a", "idx_b", "chisq", "amp", "all")


def build_pair_emulator(build, sanitize=True):
    """tests/emul/tmatch_pair_emul.cpp -> run(templates, flux, w, n, cand, topk, want_all=True) -> dict(idx_a, idx_b [N, topk], chisq
    [N, topk], amp [N, topk, 2], all [N, kA, M] or None)."""
    exe = str(build / "tmatch_pair_emul")
    if sanitize:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    else:                                                           # (for the device tests, which compare bytes: fma is exact either way)
        flags = ["-O2"]
        try:
            if " fma " in open("/proc/cpuinfo").read():
                flags.append("-mfma")
        except OSError:
            pass
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emul", "tmatch_pair_emul.cpp")], check=True)
    count = [0]

    def run(templates, flux, w, n, cand, topk, want_all=True, expect=0):
        count[0] += 1
        d = build / ("call%d" % count[0])
        d.mkdir()
        (M, ld_t), (N, ld_f), kA = templates.shape, flux.shape, cand.shape[1]
        assert w.shape == flux.shape and cand.shape[0] == N
        with open(str(d / "cfg.txt"), "w") as f:
            f.write("%d %d %d %d %d %d %d %d\n" % (N, M, n, ld_t, ld_f, kA, topk, int(want_all)))
        for nm, a, dt in (("templates", templates, np.float32), ("flux", flux, np.float32), ("w", w, np.float64), ("cand", cand, np.int32)):
            np.ascontiguousarray(a, dtype=dt).tofile(str(d / (nm + ".bin")))
        res = subprocess.run([exe, str(d)], capture_output=True, text=True)
        assert res.returncode == expect, (res.returncode, res.stderr[-2000:])
        assert open(str(d / "tile.txt")).read().split() == [str(ROWS), str(CHUNK)]
        if expect:
            return None
        every = np.fromfile(str(d / "all.bin")).reshape(N, kA, M)
        if not want_all:
            assert np.all(every == -777.25)
        return dict(idx_a=np.fromfile(str(d / "idx_a.bin"), dtype=np.int32).reshape(N, topk), idx_b=np.fromfile(str(d / "idx_b.bin"), dtype=np.int32).reshape(N, topk),
                    chisq=np.fromfile(str(d / "chisq.bin")).reshape(N, topk), amp=np.fromfile(str(d / "amp.bin")).reshape(N, topk, 2),
                    all=every if want_all else None)
    return run


def same_bytes(a, b, rows=slice(None)):
    return all(a[k].tobytes() == b[k][rows].tobytes() for k in KEYS if a[k] is not None and b[k] is not None)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_pair_emulator(tmp_path_factory.mktemp("tmatch_pair_emul"))


# ---- 1. values, NaN pattern and lists on the shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("NK", SHAPE_NK, ids=["N%d-kA%d" % nk for nk in SHAPE_NK])
@pytest.mark.parametrize("n", SHAPE_N_PIX)
def test_values_and_lists_on_the_host(emul, n, NK):
    """Every chi^2 within (2 n + 16) 2^-53 S_p of the long double solve's direct sum; the NaN pattern the reference's; the lists exact
    against the own rows, and against the reference's; all_dev NULL and the last star alone give the same bytes."""
    N, kA = NK
    rng = np.random.default_rng(1000 * n + 10 * N + kA)
    differ, worst = 0, 0.0
    for M, topk in shape_cases(n, NK):
        templates, flux, w, cand, _ = pair_case(rng, N, M, n, kA)
        got = emul(templates, flux, w, n, cand, topk)
        what = "host n=%d N=%d kA=%d M=%d topk=%d" % (n, N, kA, M, topk)
        ref = reference(templates, flux, w, n, cand)
        worst = max(worst, check_values(got["all"], ref, what))
        differ += check_pair_lists(got, cand, ref, n, what)
        assert same_bytes(emul(templates, flux, w, n, cand, topk, want_all=False), got), (what, "all NULL")
        if N > 1:
            assert same_bytes(emul(templates, flux[N - 1:], w[N - 1:], n, cand[N - 1:], topk), got, slice(N - 1, N)), (what, "a star alone")
    print("n=%d N=%d kA=%d: worst |dchi2| / bound %.3g; %d list entries differ from the long double rows'" % (n, N, kA, worst, differ))
    # (two amplitudes fit two pixels exactly, and of five pixels a star may count three: there the listed chi^2 are zero or tiny
    # against their bounds, and check_lists has shown that each entry that differs is such a tie)
    assert differ == 0 or n <= 5


# ---- 2. edge cases -------------------------------------------------------------------------------------------------------------------
def edge_case():
    """n = 37, M = CHUNK + 5, kA = 3, topk = 8, six stars:
      0  c (0.7 m_7 + 0.3 m_2), primaries (7, 2, 9); template CHUNK + 1 is a copy of template 2: (2, CHUNK + 1) is exactly collinear,
         NaN; the pairs (7, 2) and (7, CHUNK + 1) have one chi^2 and are listed in index order, across the chunk boundary; (2, 7) in
         slot 1 is the pair of slot 0, listed once
      1  no counting pixel: lists nothing
      2  exactly two counting pixels
      3, 4  template 11 is NaN at pixel 3, which star 3 counts and star 4 does not; both have primaries (11, 12, 13)
      5  primaries (4, -1, M): one unused slot, one index outside the bank."""
    rng = np.random.default_rng(55)
    n, M, N, kA = 37, CHUNK + 5, 6, 3
    templates, flux, w, cand, truth = pair_case(rng, N, M, n, kA)
    templates[:, :n] = np.where(np.isnan(templates[:, :n]), np.float32(0.9), templates[:, :n])
    templates[CHUNK + 1] = templates[2]
    t = templates[:, :n].astype(np.float64)
    w[0, :n], flux[0, :n], cand[0] = 1e4, (1.1 * (0.7 * t[7] + 0.3 * t[2])).astype(np.float32), (7, 2, 9)
    w[1, :n] = 0.0
    w[2, :n] = 0.0
    w[2, [5, 20]], flux[2, [5, 20]] = 1e4, (1.0, 0.9)
    for s in (3, 4):
        w[s, :n], flux[s, :n], cand[s] = 1e4, (0.9 * (0.7 * t[12] + 0.3 * t[13])).astype(np.float32), (11, 12, 13)
    templates[11, 3] = np.nan
    w[4, 3] = 0.0
    w[5, :n], flux[5, :n], cand[5] = 1e4, (1.3 * (0.7 * t[4] + 0.3 * t[30])).astype(np.float32), (4, -1, M)
    cand[2] = (0, 1, 3)
    return templates, flux, w, cand, n


def check_edge_case(got, cand):
    every, ia, ib, chisq, amp = got["all"], got["idx_a"], got["idx_b"], got["chisq"], got["amp"]
    M = every.shape[2]
    assert np.isnan(every[0, 1, CHUNK + 1]) and np.isnan(every[0, 1, 2])                    # collinear with its copy; with itself
    assert every[0, 0, 2] == every[0, 0, CHUNK + 1] and (ia[0, :2].tolist(), ib[0, :2].tolist()) == ([7, 7], [2, CHUNK + 1]) and chisq[0, 0] == chisq[0, 1]
    assert abs(amp[0, 0, 0] - 0.77) < 1e-4 and abs(amp[0, 0, 1] - 0.33) < 1e-4 and np.isnan(every[0, 1, 7]) and np.isfinite(every[0, 0, 2])
    assert np.all(np.isnan(every[1])) and np.all(ia[1] == -1) and np.all(ib[1] == -1) and np.all(np.isinf(chisq[1])) and np.all(np.isnan(amp[1]))
    assert np.all(np.isnan(every[3, 0])) and np.all(np.isnan(every[3, :, 11])) and 11 not in ia[3] and 11 not in ib[3]
    assert np.isfinite(every[4, 0]).any() and (ia[3, 0], ib[3, 0]) == (12, 13) and (ia[4, 0], ib[4, 0]) == (12, 13)
    assert np.all(np.isnan(every[5, 1:])) and (ia[5, 0], ib[5, 0]) == (4, 30) and np.all(ia[5][ia[5] >= 0] == 4)
    assert np.all(chisq[:, :-1] <= chisq[:, 1:])
    assert all(np.isnan(every[s, j, cand[s, j]]) for s in range(6) for j in range(3) if 0 <= cand[s, j] < M)    # a template with itself


def test_edge_cases_of_the_rules_and_the_selection(emul):
    templates, flux, w, cand, n = edge_case()
    got = emul(templates, flux, w, n, cand, 8)
    check_edge_case(got, cand)
    ref = reference(templates, flux, w, n, cand)
    check_values(got["all"], ref, "edge case")
    differ = check_pair_lists(got, cand, ref, n, "edge case")        # (star 2's two pixels are fitted exactly by every pair: its list is all ties)
    print("edge case: %d list entries differ from the long double rows', every one a tie within the bounds" % differ)
    assert differ <= 8
    assert same_bytes(emul(templates, flux, w, n, cand, 8, want_all=False), got)
    assert same_bytes(emul(templates, flux[5:], w[5:], n, cand[5:], 8), got, slice(5, 6))


def few_pairs_case():
    """topk = 8 > the two pairs that M = 3 templates and one primary leave."""
    rng = np.random.default_rng(66)
    templates, flux, w, cand, truth = pair_case(rng, 3, 3, 37, 1)
    cand[:, 0] = truth[:, 0]
    return templates, flux, w, cand, 37


def test_more_slots_than_pairs(emul):
    templates, flux, w, cand, n = few_pairs_case()
    got = emul(templates, flux, w, n, cand, 8)
    filled = (got["idx_b"] >= 0).sum(axis=1)
    assert np.all(filled >= 1) and np.all(filled <= 2) and np.all(got["idx_b"][:, 2:] == -1) and np.all(np.isinf(got["chisq"][:, 2:])) and np.all(np.isnan(got["amp"][:, 2:]))
    assert np.all(got["idx_a"][:, 2:] == -1) and np.all(got["idx_a"][:, 0] == cand[:, 0])
    ref = reference(templates, flux, w, n, cand)
    check_values(got["all"], ref, "few pairs")
    assert check_pair_lists(got, cand, ref, n, "few pairs") == 0


def test_arguments_the_library_rejects(emul):
    templates, flux, w, cand, _ = pair_case(np.random.default_rng(9), 2, 3, 5, 2)
    for n, topk, c in ((5, 0, cand), (5, 9, cand), (9, 1, cand), (0, 1, cand), (5, 1, np.zeros((2, 17), dtype=np.int32))):
        emul(templates, flux, w, n, c, topk, expect=3)


# ---- 3. recovery ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (37, 1000))
def test_the_planted_pair_is_first(emul, n):
    """primaries = 4: the pair the flux was mixed from is rank 0, the brighter amplitude belongs to the 0.7 component and the light ratio
    is within 0.05 of 0.3."""
    rng = np.random.default_rng(7000 + n)
    N, M = 23, CHUNK + 1
    templates, flux, w, cand, truth = pair_case(rng, N, M, n, 4)
    got = emul(templates, flux, w, n, cand, 3)
    amp = got["amp"][:, 0]
    bright = np.where(amp[:, 0] >= amp[:, 1], got["idx_a"][:, 0], got["idx_b"][:, 0])
    faint = np.where(amp[:, 0] >= amp[:, 1], got["idx_b"][:, 0], got["idx_a"][:, 0])
    ratio = amp.min(axis=1) / amp.sum(axis=1)
    print("n=%d: primaries' slot of the 0.7 component %s; ratio %.3f .. %.3f" % (n, [int(np.flatnonzero(cand[s] == truth[s, 0])[0]) if truth[s, 0] in cand[s] else -1 for s in range(N)],
                                                                                 ratio.min(), ratio.max()))
    assert np.array_equal(bright, truth[:, 0]) and np.array_equal(faint, truth[:, 1])
    assert np.all(np.abs(ratio - 0.3) <= 0.05)


# ---- 4. fitting/tmatch.py and optfit.py on the host ------------------------------------------------------------------------------------
def test_match_pairs_and_fit_binary_from_bank_argument_checks():
    from thepayne_amd.fitting import optfit, tmatch
    assert all(s in _lib.SYMBOLS for s in ("payne_tmatch_create_pairs", "payne_tmatch_match_pairs", "payne_tmatch_pair_rows", "payne_tmatch_pair_chunk"))
    assert _lib.TMATCH_MAX_PRIMARIES == 16
    assert tmatch.check_pair_args(1, 4, 100) == (1, 4, None) and tmatch.check_pair_args(8, 8, 100)[:2] == (8, 8)
    k, kA, sl = tmatch.check_pair_args(2, 5, 10, shortlist=[[3, 3, 11, -7, 4], [0, 1, 0, 1, 9]])
    assert (k, kA) == (2, 5) and sl.dtype == np.int32 and sl.tolist() == [[3, -1, -1, -1, 4], [0, 1, -1, -1, 9]]
    assert tmatch.check_pair_args(1, 16, 100, shortlist=np.zeros((2, 16), dtype=np.int64))[2].shape == (2, 16)
    for bad in (dict(topk=0), dict(topk=9), dict(topk=True), dict(primaries=0), dict(primaries=17), dict(primaries=9), dict(primaries=2.5),
                dict(shortlist=np.zeros((2, 3), dtype=np.int32)), dict(shortlist=np.zeros((2, 4))), dict(shortlist=np.zeros((3, 4), dtype=np.int32), N=2)):
        with pytest.raises(ValueError):
            tmatch.check_pair_args(**dict(dict(topk=1, primaries=4, M=10), **bad))
    assert tmatch.PAIR_WORKSPACE_BYTES == 256 * 1024 * 1024
    B = object.__new__(tmatch.TemplateBank)
    B.templates = None
    with pytest.raises(RuntimeError):
        B.match_pairs(np.ones((3, 10)), np.ones((3, 10)))
    assert hasattr(tmatch.TMatchHandle, "match_pairs")
    # fit_binary_from_bank: another grid, something that is no bank, starts of the caller's
    nobs = 10
    flux, eflux = np.ones((3, nobs)), np.full((3, nobs), 0.01)
    F = object.__new__(optfit.OptFit)
    F.obs_wave = np.linspace(5200.0, 5201.0, nobs)
    B.obs_wave = F.obs_wave + 0.01
    with pytest.raises(ValueError):
        F.fit_binary_from_bank(flux, eflux, B)
    B.obs_wave = F.obs_wave[:-1]
    with pytest.raises(ValueError):
        F.fit_binary_from_bank(flux, eflux, B)
    with pytest.raises(TypeError):
        F.fit_binary_from_bank(flux, eflux, object())
    B.obs_wave = F.obs_wave.copy()
    for name, value in (("start_a", np.zeros((3, 8))), ("start_b", np.zeros((3, 8))), ("ratio", 0.3), ("coef", np.ones((3, 1)))):
        with pytest.raises(TypeError):
            F.fit_binary_from_bank(flux, eflux, B, **{name: value})


# ---- 5. the end-to-end inputs of tests/test_tmatch_pair_gpu.py: binaries against a lattice bank -----------------------------------------
BINARY_N, BINARY_NOBS, BINARY_Q, BINARY_DV, BINARY_TIE = 4, 100, 0.3, 40.0, ("feh", "afe")
BINARY_STEPS, BINARY_VRAD, BINARY_VROT, BINARY_INST_R = (3, 2, 1, 1, 1), (-20.0, 0.0, 20.0), 10.0, 20000.0
BINARY_SEED, BINARY_OFF, BINARY_VOFF = 4, 0.02, 0.25                  # the truths' distance from their nodes: in cells per label, in km/s
_BINARY_BANK = {}


def pair_search_numpy(templates, flux, w, primaries=4):
    """The pair search in numpy fp64 on host templates [M, n]: per star (a, b, scale, ratio, chi^2, the single template's chi^2) of the
    best pair among the `primaries` best single templates with a scale against the whole bank, A the brighter."""
    n = templates.shape[1]
    cand = shortlist_numpy(templates, flux, w, n, primaries)
    ref = reference(templates, flux, w, n, cand)
    out = []
    for s in range(flux.shape[0]):
        chi = np.asarray(ref["chi"][s], dtype=np.float64)
        j, b = np.unravel_index(np.nanargmin(chi), chi.shape)
        a, al, be = int(cand[s, j]), float(ref["alpha"][s, j, b]), float(ref["beta"][s, j, b])
        if be > al:
            a, b, al, be = b, a, be, al
        ok = w[s] != 0.0
        f, T = np.where(ok, flux[s], 0.0).astype(np.float64), templates.astype(np.float64)
        B, S = T @ (w[s] * f), (T * T) @ w[s]
        out.append((int(a), int(b), al + be, be / (al + be), float(chi[j, b] if be <= al else np.nanmin(chi)), float(((w[s] * f * f).sum() - B * B / S).min())))
    return out


def binary_bank_inputs(g20):
    """Four double-lined binaries on g20's SMLP and a lattice bank that does not hold them.  Components 40 km/s apart (B's Vrad is A's
    -+ 40, the sign alternating), q = 0.3, a constant scale in [0.8, 1.6], one composition (feh and afe tied), 100 pixels, S/N 100 errors,
    noiseless spectra of the fp64 oracle chain rounded to fp32.  The bank: the cell centres of a lattice of 3 Teff x 2 logg cells (one cell
    in the other labels) times Vrad -20, 0, 20 (18 templates), one Vrot and Inst_R.  The components sit 0.25 km/s off the nodes -+20, which
    span them, and 2 % of a cell off their cells' centres in every label, so no template is a truth; B lies in another Teff cell than A.
    The lattice was chosen on the CPU: this fixture network's templates of neighbouring cells are so alike that on finer lattices (3 3 2 2,
    3 3 1 1) the single-template search leaves the primary's cell out of its best four for most binaries, and with it the pair (numpy:
    about one binary in ten found there; three of four here, seeds 1 .. 8 finding 1 to 4).  Of the seeds whose binaries numpy finds, seed 2
    finds all four but two of its reference loops need 15 and 19 evaluations; on one of those the device's fit ended CONVERGED 1.7e-2
    conditional sigma from the minimum (the fp32-fed numpy loop: 6e-3), the others within 1.8e-3.  Seed 4 leaves one binary out.
    Returns dict(net, nntype, obs_wave, theta, templates (the oracle's), args, tie, truth_a, truth_b, ztruth, cell_a, cell_b (the bank
    rows of the truths' cells), scale, flux fp32, eflux, found, pairs [4, 2] (numpy's pair search), results (the fp64 loop started there,
    with ``polished``, the same loop carried on to xtol 1e-6; or None where the search missed the cells), kept (the binaries whose cells
    the search finds and whose loop ends CONVERGED within RECOVERY_MAX_EVALS evaluations, tests/test_lmfit.py's and test_lmfit_pair.py's
    criterion for recovery inputs: a loop that needs more creeps along a flat valley, where fp32 decides where a fit stops)."""
    if "case" not in _BINARY_BANK:
        from test_lmfit import CONVERGED, OracleModel, lm_reference, recovery_net
        from thepayne_amd.fitting import optfit
        from thepayne_amd.fitting.tmatch import lattice_theta
        net, nntype = recovery_net(g20, "smlp")
        xmin, xmax = net["xmin"], net["xmax"]
        D, S, nobs = len(xmin), BINARY_N, BINARY_NOBS
        lab = [0, 1, 2, 3] + ([6] if D == 5 else [])
        steps = np.array(BINARY_STEPS[:D])
        wave = net["wavelength"]
        width = wave[-1] - wave[0]
        obs_wave = np.linspace(wave[0] + 0.2 * width, wave[-1] - 0.2 * width, nobs)
        theta = lattice_theta(xmin, xmax, steps, vrad=BINARY_VRAD, vrot=(BINARY_VROT,), inst_R=(BINARY_INST_R,))
        assert len(theta) <= 400
        rng = np.random.default_rng(BINARY_SEED)
        cell_w = (xmax - xmin) / steps
        ca = np.stack([rng.integers(0, steps) for _ in range(S)])
        cb = ca.copy()                                               # one composition; B in another Teff cell
        cb[:, 0] = (ca[:, 0] + 1 + rng.integers(0, steps[0] - 1, S)) % steps[0]
        off = BINARY_OFF * rng.choice([-1.0, 1.0], (S, D))
        ta, tb = np.full((S, 8), np.nan), np.full((S, 8), np.nan)
        ta[:, lab], tb[:, lab] = xmin + (ca + 0.5 + off) * cell_w, xmin + (cb + 0.5 + off) * cell_w
        tb[:, [2, 3]] = ta[:, [2, 3]]
        sign = np.where(np.arange(S) % 2 == 0, -1.0, 1.0)
        va = -0.5 * sign * BINARY_DV + BINARY_VOFF * rng.choice([-1.0, 1.0], S)
        ta[:, 4], tb[:, 4] = va, va + sign * BINARY_DV
        ta[:, 5] = tb[:, 5] = BINARY_VROT
        ta[:, 7] = tb[:, 7] = BINARY_INST_R
        node = lambda t: int(np.argmin(np.abs((theta[:, lab] - t[lab]) / cell_w).sum(axis=1) + np.abs(theta[:, 4] - t[4]) / 20.0))   # noqa: E731
        cell_a, cell_b = np.array([node(t) for t in ta]), np.array([node(t) for t in tb])
        eflux = np.full((S, nobs), 0.01)
        args = optfit.check_binary_args(np.ones((S, nobs)), eflux, ta, tb, nobs, D, xmin, xmax, ratio=BINARY_Q, tie=BINARY_TIE, fit_vrad=True, npoly=1)
        cols, Ka, Kl, ia, ib, b_pos = args["cols"], args["Ka"], args["Kl"], args["ia"], args["ib"], args["b_pos"]
        free_b = [k for k in range(Ka) if b_pos[k] >= Ka]
        om = OracleModel(net, nntype, obs_wave, theta[0], fit_vrad=True)
        templates = np.array([om(t[cols])[0] for t in theta])
        scale = rng.uniform(0.8, 1.6, S)
        flux = np.array([scale[s] * ((1.0 - BINARY_Q) * om(ta[s][cols])[0] + BINARY_Q * om(tb[s][cols])[0]) for s in range(S)]).astype(np.float32)
        w = 1.0 / eflux ** 2
        found = pair_search_numpy(templates, flux, w)
        def make_fun(model):
            def fun(z):
                mA, JA = model(z[:Ka])
                mB, JB = model(z[b_pos])
                qq, p = z[Kl], z[Kl + 1]
                mix = (1.0 - qq) * mA + qq * mB
                J = [p * ((1.0 - qq) * (JA[ia[k]] if ia[k] >= 0 else 0.0) + qq * (JB[ib[k]] if ib[k] >= 0 else 0.0)) for k in range(Kl)]
                return p * mix, np.array(J + [p * (mB - mA), mix])
            return fun
        results, kept = [], []
        for s, (a, b, c, q, chi, single) in enumerate(found):
            res = None
            if (a, b) == (cell_a[s], cell_b[s]):
                z0 = np.concatenate([theta[a][cols], theta[b][[cols[k] for k in free_b]], [np.clip(q, 0.01, 0.99)], [c]])

                fun = make_fun(om)
                res = lm_reference(fun, z0, args["lo"], args["hi"], flux[s].astype(np.float64), w[s])
                if res["status"] == CONVERGED:
                    # the same loop carried on from its end with xtol 1e-6: the minimum itself.  At the default xtol = 1e-3 a loop that
                    # creeps along a valley stops up to several 1e-3 sigma short of it (binary 3: 15 evaluations, 6e-3 sigma from
                    # the truth), which would take more than half of the 1e-2 sigma that the device's fit is allowed against it.
                    pol = res["polished"] = lm_reference(fun, res["x"], args["lo"], args["hi"], flux[s].astype(np.float64), w[s], xtol=1e-6, maxiter=200)
                    if pol["status"] == CONVERGED and res["niter"] <= RECOVERY_MAX_EVALS:
                        kept.append(s)
            results.append(res)
        ztruth = np.concatenate([ta[:, cols], tb[:, [cols[k] for k in free_b]], np.full((S, 1), BINARY_Q), scale[:, None]], axis=1)
        _BINARY_BANK["case"] = dict(ztruth=ztruth, net=net, nntype=nntype, obs_wave=obs_wave, theta=theta, templates=templates, args=args, tie=BINARY_TIE, truth_a=ta, truth_b=tb,
                                    cell_a=cell_a, cell_b=cell_b, scale=scale, flux=flux, eflux=eflux, found=found,
                                    pairs=np.array([[f[0], f[1]] for f in found]), results=results, kept=kept)
    return _BINARY_BANK["case"]


def test_numpy_pair_search_finds_the_cells_and_the_reference_loop_converges(golden):
    """The inputs tests/test_tmatch_pair_gpu.py fits through fit_binary_from_bank: numpy's pair search on the oracle's templates puts the
    pair of the truths' cells first, and the fp64 reference loop on the mixed model started there ends CONVERGED -- on three of the four
    binaries; one is left out (below)."""
    case = binary_bank_inputs(golden("g20_trainspec"))
    for s, f in enumerate(case["found"]):
        r = case["results"][s]
        print("binary %d: cells (%d, %d), found (%d, %d) scale %.4f (truth %.4f) ratio %.4f, chi^2 %.4g against the single template's %.4g; reference: %s"
              % (s, case["cell_a"][s], case["cell_b"][s], f[0], f[1], f[2], case["scale"][s], f[3], f[4], f[5],
                 "none" if r is None else "status %d after %d evaluations, chi^2 %.3g, q %.4f" % (r["status"], r["niter"], r["chisq"], r["x"][case["args"]["Kl"]])))
    assert len(case["theta"]) <= 400
    for s in range(BINARY_N):
        r = case["results"][s]
        if r is None:
            continue
        p = r["polished"]
        print("binary %d: the loop's end is %.3g sigma from the truth; carried on to xtol 1e-6 (status %d, %d evaluations, chi^2 %.3g) %.3g sigma"
              % (s, sigma_distance(r["x"], case["ztruth"][s], r["A"]), p["status"], p["niter"], p["chisq"], sigma_distance(p["x"], case["ztruth"][s], p["A"])))
        assert r["status"] == CONVERGED and p["status"] == CONVERGED and sigma_distance(p["x"], case["ztruth"][s], p["A"]) <= 1e-3      # (the flux is rounded to fp32)
    # ONE BINARY IS LEFT OUT, binary 1: numpy's pair search does not put the pair of its cells first (the primary's cell is not among the
    # four best single templates).  The other three are found and their loops converge within RECOVERY_MAX_EVALS evaluations.
    assert case["kept"] == [0, 2, 3]
    found = case["pairs"][case["kept"]]
    assert np.array_equal(found, np.stack([case["cell_a"], case["cell_b"]], axis=1)[case["kept"]])
