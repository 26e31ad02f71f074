"""numpy oracle of the score track (smcpp_score_rows / _windows): a position-level forward-backward pass in float64 over the PURE
hidden Markov model - initial distribution pi, transition matrix T [M x M], one emission vector per key - and the Jacobians of the
three tables with respect to nder directions.  It forms the dense xi_p(i, j) of every position, adds it up over a row's positions and
contracts the row's sum with dT / T; gamma_p is xi_p's column sum and meets dE[k] / E[k]; gamma_0 meets dpi / pi.

It is built from what a manager's getters hand out (`pi`, `transition`, `emission_probs`, `keys` and the three `_jac` getters, arrays
of shapes [M, nder], [M, M, nder], [K, M, nder]) and the rows the manager was given.  On purpose it shares nothing with the kernel: no
generators of T, no blocks, no float vectors, no floor; vectors are renormalised at every position (xi_p is scale free).  Where a table
entry is not positive its ratio is taken as zero, as the engine does (a floored entry has a zero Jacobian anyway).

`loglik` is the log-likelihood of the same model (pi, T, E need not be normalised), whose finite differences the score has to match;
`score_windows` is the second product from the explicit overlap matrix of rows and windows."""
import numpy as np

from transref import row_key_ids

EPS = 2.0 ** -52


def _ratio(d, x):
    x = np.asarray(x, dtype=np.float64)[..., None]
    return np.where(x > 0.0, np.asarray(d, dtype=np.float64) / np.where(x > 0.0, x, 1.0), 0.0)


def loglik(pi, T, keys, E, obs):
    """log of pi^T prod_p (T diag e_p) 1 over the positions of `obs` (rows of span, key...)."""
    pi, T, E = (np.asarray(x, dtype=np.float64) for x in (pi, T, E))
    obs = np.asarray(obs)
    kid = row_key_ids(obs, keys)
    Tt = np.ascontiguousarray(T.T)
    a = pi
    ll = np.log(a.sum())
    a = a / a.sum()
    for l in range(len(obs)):
        e = E[kid[l]]
        for _ in range(int(obs[l, 0])):
            a = e * (Tt @ a)
            s = a.sum()
            ll += np.log(s)
            a /= s
    return float(ll)


def score_rows(pi, T, keys, E, dpi, dT, dE, obs, cells=1 << 22):
    """-> [3 x nder x (L + 1)]: the initial, emission and transition part; column l >= 1 belongs to row l of `obs`, column 0 holds the
    initial part (its other two parts are zero, and so is the initial part of every other column).

    a_0 = pi, a_p = e_p o (T^T a_{p-1}); b_N = 1, b_{p-1} = T (e_p o b_p); xi_p(i, j) = a_{p-1}(i) T(i, j) e_p(j) b_p(j) / (its sum)."""
    pi = np.asarray(pi, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    obs = np.asarray(obs)
    M, L = len(pi), len(obs)
    Gpi, GT, GE = _ratio(dpi, pi), _ratio(dT, T), _ratio(dE, E)
    nder = Gpi.shape[1]
    assert Gpi.shape == (M, nder) and GT.shape == (M, M, nder) and GE.shape == (len(E), M, nder)
    spans = obs[:, 0].astype(np.int64)
    kid = row_key_ids(obs, keys)
    A = np.empty((L + 1, M))                               # forward vectors at the row boundaries
    a = pi / pi.sum()
    A[0] = a
    Tt = np.ascontiguousarray(T.T)
    for l in range(L):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            a /= a.sum()
        A[l + 1] = a
    out = np.zeros((3, nder, L + 1))
    b = np.ones(M) / M                                     # after the last position
    blk = max(1, cells // (M * M))
    for l in range(L - 1, -1, -1):
        e, s = E[kid[l]], int(spans[l])
        X = np.empty((s, M))                               # X[t] = a before position t of the row
        a = A[l]
        for t in range(s):
            X[t] = a
            a = e * (Tt @ a)
            a /= a.sum()
        W = np.empty((s, M))                               # W[t] = e o b after position t
        for t in range(s - 1, -1, -1):
            W[t] = e * b
            b = T @ W[t]
            b /= b.sum()
        xs = np.zeros((M, M))
        for t0 in range(0, s, blk):
            xi = X[t0:t0 + blk, :, None] * T[None, :, :] * W[t0:t0 + blk, None, :]          # dense, per position
            xi /= xi.sum(axis=(1, 2), keepdims=True)
            xs += xi.sum(axis=0)
        out[2, :, l + 1] = np.einsum("ij,ijd->d", xs, GT)
        out[1, :, l + 1] = xs.sum(axis=0) @ GE[kid[l]]
    g0 = A[0] * b
    out[0, :, 0] = (g0 / g0.sum()) @ Gpi
    return out


def score_windows(v, spans, W):
    """[nder x ceil(P / W)] from per-row values v [nder x (L + 1)]: out[d, w] = sum_l O[l, w] / s_l * v[d, l] over the rows l >= 1 with
    the explicit overlap matrix O[l, w] = |[P_{l-1}, P_l) n [w W, (w + 1) W)|, and column 0 added to window 0.
    -> (out, the same sums over the absolute values of the terms)."""
    v = np.asarray(v, dtype=np.float64)
    spans = np.asarray(spans, dtype=np.int64)
    assert v.ndim == 2 and v.shape[1] == len(spans) + 1 and W >= 1
    P1 = np.cumsum(spans)
    P0 = P1 - spans
    total = int(P1[-1])
    nwin = -(-total // W)
    lo = np.arange(nwin, dtype=np.int64) * W
    hi = np.minimum(lo + W, total)
    per_bp = v[:, 1:] / spans
    out, mag = np.zeros((v.shape[0], nwin)), np.zeros((v.shape[0], nwin))
    block = 2048
    for w0 in range(0, nwin, block):
        w1 = min(nwin, w0 + block)
        l0 = int(np.searchsorted(P1, lo[w0], side="right"))               # first row that ends behind the block's start
        l1 = int(np.searchsorted(P0, hi[w1 - 1], side="left"))            # first row that starts at or behind its end
        O = np.clip(np.minimum(P1[l0:l1, None], hi[None, w0:w1]) - np.maximum(P0[l0:l1, None], lo[None, w0:w1]), 0, None).astype(np.float64)
        out[:, w0:w1] = per_bp[:, l0:l1] @ O
        mag[:, w0:w1] = np.abs(per_bp[:, l0:l1]) @ O
    out[:, 0] += v[:, 0]
    mag[:, 0] += np.abs(v[:, 0])
    return out, mag
