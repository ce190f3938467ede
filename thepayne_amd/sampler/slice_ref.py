"""The device's slice-sampling chain (slice_round_wave in csrc/sampler_core.hpp) restated in numpy, for one walk.

Test infrastructure: the same hash (``mix64`` / ``u01`` on uint64), the same permutation rule, the same phase machine and the
same caps, the geometry in the same order of fp64 operations, so that a walk driven by the device's own likelihood values
reproduces the device's unit-cube points to the bit.  Nothing in the product imports this module and it is the fallback of
nothing: the values come from the callable ``lnprob_u(P) -> (V, lp)`` it is handed.
"""
import numpy as np

__all__ = ["mix64", "u01", "slice_key", "wave_sum", "slice_walk_ref", "MAX_SHRINK"]

MAX_SHRINK = 200                                  # kSliceMaxShrink
NEW, LEFT, RIGHT, SHRINK, DONE = range(5)
_U = np.uint64


def mix64(x):
    """splitmix64's finaliser on uint64 arrays (wraps)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=_U) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def _stream(seed, chain, step):
    return _U(seed) ^ ((np.asarray(chain, dtype=_U) << _U(32)) | np.asarray(step, dtype=_U))


def u01(seed, chain, step, draw):
    """The device's u01(seed, chain, step, draw): uniform in (0, 1), 53 bits."""
    with np.errstate(over="ignore"):
        x = mix64(mix64(_stream(seed, chain, step)) + np.asarray(draw, dtype=_U))
    return ((x >> _U(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def slice_key(seed, chain, sweep, d):
    """The key dimension d sorts by in sweep `sweep` of a chain ('slice': the axes in the order of their keys, ties by index)."""
    with np.errstate(over="ignore"):
        return mix64(mix64(_stream(~_U(seed), chain, sweep)) + np.asarray(d, dtype=_U))


_LANES = np.arange(64)


def wave_sum(X):
    """Row sums of X[n, nd <= 64] as a 64-lane butterfly adds them (partner distances 32, 16, .. 1)."""
    x = np.zeros((len(X), 64))
    x[:, :X.shape[1]] = X
    for j in (32, 16, 8, 4, 2, 1):
        x = x + x[:, _LANES ^ j]
    return x[:, 0]


def slice_walk_ref(lnprob_u, U, V, lnprob, axes, scale, loglstar, slices, random_dirs, seed, ell=None, max_rounds=None):
    """One walk of K lock-step chains.  ``axes``: [nd, nd] or [n_ell, nd, nd], columns = axes, with ``ell[K]`` naming each
    chain's matrix.  Returns (U, V, lnprob, ncall, nexpand, ncontract, n_active) as DeviceProposer.slice_walk does."""
    U = np.array(U, dtype=np.float64)
    V = np.array(V, dtype=np.float64)
    lnprob = np.array(lnprob, dtype=np.float64)
    K, nd = U.shape
    A = np.asarray(axes, dtype=np.float64)
    if A.ndim == 2:
        A = A[None]
    ell = np.zeros(K, dtype=np.int64) if ell is None or len(A) == 1 else np.asarray(ell, dtype=np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    scale, lstar = float(scale), float(loglstar)
    n_dir = int(slices) if random_dirs else int(slices) * nd
    chain = np.arange(K)
    dims = np.arange(nd)
    phase = np.full(K, NEW)
    dirn, attempt, nshrink = (np.zeros(K, dtype=np.int64) for _ in range(3))
    ncall, nexpand, ncontract = (np.zeros(K, dtype=np.int64) for _ in range(3))
    left, right, axis, cand = (np.zeros((K, nd)) for _ in range(4))
    vprop, lp_pend = np.zeros((K, nd)), np.full(K, -np.inf)
    pending = np.zeros(K, dtype=bool)

    def advance(m):
        dirn[m] += 1
        attempt[m] = 0
        nshrink[m] = 0
        phase[m] = np.where(dirn[m] >= n_dir, DONE, NEW)

    def shrink(m, P):
        if not m.any():
            return
        side = wave_sum((P[m] - U[m]) * (right[m] - left[m]))
        neg = np.zeros(K, dtype=bool)
        neg[m] = side < 0.0
        left[m & neg] = P[m & neg]
        right[m & ~neg] = P[m & ~neg]
        nshrink[m] += 1
        advance(m & (nshrink >= MAX_SHRINK))

    def settle():
        with np.errstate(invalid="ignore"):
            above = lp_pend > lstar
        p1, p2, p3 = (pending & (phase == k) for k in (LEFT, RIGHT, SHRINK))
        left[p1 & above] -= axis[p1 & above]
        phase[p1 & ~above] = RIGHT
        right[p2 & above] += axis[p2 & above]
        phase[p2 & ~above] = SHRINK
        acc = p3 & above
        U[acc], V[acc], lnprob[acc] = cand[acc], vprop[acc], lp_pend[acc]
        advance(acc)
        shrink(p3 & ~above, cand)
        pending[:] = False

    def new_direction(m):
        c, d = chain[m], dirn[m]
        if not random_dirs:
            sweep, j = d // nd, d % nd
            keys = slice_key(seed, c[:, None], sweep[:, None], dims[None, :])
            col = np.argsort(keys, axis=1, kind="stable")[np.arange(len(c)), j]
            ax = scale * A[ell[m], :, col]
        else:
            a = u01(seed, c[:, None], d[:, None], attempt[m][:, None] + 2 * dims[None, :])
            b = u01(seed, c[:, None], d[:, None], attempt[m][:, None] + 2 * dims[None, :] + 1)
            attempt[m] += 2 * nd
            z = np.sqrt(-2.0 * np.log(a)) * np.cos(2.0 * np.pi * b)
            z = z / np.sqrt(wave_sum(z * z))[:, None]
            s = np.zeros((len(c), nd))
            Am = A[ell[m]]
            for k in range(nd):
                s = s + Am[:, :, k] * z[:, k:k + 1]
            ax = scale * s
        r = u01(seed, c, d, attempt[m])[:, None]
        attempt[m] += 1
        axis[m] = ax
        left[m] = U[m] - r * ax
        right[m] = U[m] + (1.0 - r) * ax
        phase[m] = LEFT

    rounds = 0
    while (phase != DONE).any() and (max_rounds is None or rounds < max_rounds):
        if pending.any():
            settle()
        todo = phase != DONE
        emit = np.zeros(K, dtype=bool)
        while todo.any():
            m = todo & (phase == NEW)
            if m.any():
                new_direction(m)
            sh = todo & (phase == SHRINK)
            ex = todo & ~sh
            ncall[todo] += 1
            nexpand[ex] += 1
            ncontract[sh] += 1
            if sh.any():
                t = u01(seed, chain[sh], dirn[sh], attempt[sh])[:, None]
                attempt[sh] += 1
                cand[sh] = left[sh] + t * (right[sh] - left[sh])
            cand[ex] = np.where((phase[ex] == LEFT)[:, None], left[ex], right[ex])
            inside = np.all((cand > 0.0) & (cand < 1.0), axis=1)
            ok = todo & inside
            emit |= ok
            out = todo & ~inside
            phase[out & ex] += 1                      # outside the cube: -inf without a call
            shrink(out & sh, cand)
            todo = out & (phase != DONE)
        if emit.any():
            pv, pl = lnprob_u(cand[emit])
            vprop[emit], lp_pend[emit] = pv, pl
        pending = emit
        rounds += 1
    if pending.any():
        settle()
    return U, V, lnprob, ncall, nexpand, ncontract, int((phase != DONE).sum())
