"""numpy oracles of the device-side posterior products (smcpp_posterior_columns / _summary / _windows) from a matrix `gamma`
[M x (L + 1)] as `im.gammas[c]` returns it and the span column of the L rows.  Written for clarity, not speed; the window oracle
on purpose does NOT use the kernel's method (bisection in the prefix positions): it expands the rows per base pair with `np.repeat`
(in slabs) and a second formulation builds the explicit overlap matrix."""
import numpy as np

EPS = 2.0 ** -52


def normalized(gamma):
    """p[:, l] = gamma[:, l] / sum_m gamma[m, l] - what `posterior()` returns."""
    gamma = np.asarray(gamma, dtype=np.float64)
    return gamma / gamma.sum(axis=0)


def summary(gamma, weights=None, quantiles=()):
    """dict(colsum, argmax, [mean], qstate, F): F = cumulative p over the states, qstate[k, l] = min{m : F[m, l] >= q_k} (the last
    state if rounding keeps F below q_k)."""
    gamma = np.asarray(gamma, dtype=np.float64)
    M = gamma.shape[0]
    p = normalized(gamma)
    F = np.cumsum(p, axis=0)
    out = {"colsum": gamma.sum(axis=0), "argmax": np.argmax(gamma, axis=0), "F": F}
    if weights is not None:
        out["mean"] = (np.asarray(weights, dtype=np.float64)[:, None] * p).sum(axis=0)
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    qs = np.empty((len(q), gamma.shape[1]), dtype=np.int64)
    for k, level in enumerate(q):
        reached = F >= level
        qs[k] = np.where(reached.any(axis=0), reached.argmax(axis=0), M - 1)
    out["qstate"] = qs
    return out


def quantile_ok(gamma, qstate, level, tol):
    """The acceptance rule for one level: F[m] >= q - tol and (m == 0 or F[m - 1] < q + tol), per column -> bool [ncols]."""
    F = np.cumsum(normalized(gamma), axis=0)
    m = np.asarray(qstate, dtype=np.int64)
    cols = np.arange(F.shape[1])
    at = F[m, cols]
    below = np.where(m > 0, F[np.maximum(m - 1, 0), cols], -np.inf)
    return (at >= level - tol) & (below < level + tol)


def windows_repeat(gamma, spans, W, slab_cells=1 << 24):
    """[M x ceil(P / W)]: expand p per base pair (row l >= 1 repeated s_l times; column 0 takes no part), average each run of W
    base pairs (the last run over what is left).  The per-base-pair matrix is formed `slab_cells` entries at a time; a window that
    straddles two slabs is added up from its two parts."""
    p = normalized(gamma)[:, 1:]
    spans = np.asarray(spans, dtype=np.int64)
    M, L = p.shape
    assert len(spans) == L and W >= 1
    total = int(spans.sum())
    nwin = -(-total // W)
    row_of_bp = np.repeat(np.arange(L, dtype=np.int32), spans)      # base pair -> row
    out = np.zeros((M, nwin))
    step = max(1, slab_cells // M)
    for b0 in range(0, total, step):
        b1 = min(total, b0 + step)
        per_bp = p[:, row_of_bp[b0:b1]]                                 # [M x base pairs of the slab]
        w_first, w_last = b0 // W, (b1 - 1) // W
        starts = np.maximum(np.arange(w_first, w_last + 1, dtype=np.int64) * W, b0) - b0
        out[:, w_first:w_last + 1] += np.add.reduceat(per_bp, starts, axis=1)
    lo = np.arange(nwin, dtype=np.int64) * W
    return out / (np.minimum(lo + W, total) - lo)


def windows_overlap_matrix(gamma, spans, W):
    """The same product from the explicit overlap matrix O[l, w] = |[P_{l-1}, P_l) n [w W, (w + 1) W)| (dense: small cases only)."""
    p = normalized(gamma)[:, 1:]
    spans = np.asarray(spans, dtype=np.int64)
    P1 = np.cumsum(spans)
    P0 = P1 - spans
    total = int(P1[-1])
    nwin = -(-total // W)
    lo = np.arange(nwin, dtype=np.int64) * W
    hi = np.minimum(lo + W, total)
    O = np.clip(np.minimum(P1[:, None], hi[None, :]) - np.maximum(P0[:, None], lo[None, :]), 0, None).astype(np.float64)
    return (p @ O) / (hi - lo)
