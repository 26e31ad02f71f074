"""numpy oracle of the per-position posterior products (smcpp_posterior_positions / _position_summary / _windows_exact): a
position-level forward-backward pass in float64 over the PURE hidden Markov model - initial distribution pi, transition matrix T
[M x M], one emission vector per key -, renormalised at every position:

    a_0 = pi, a_p = e_p o (T^T a_{p-1});   b_N = 1, b_{p-1} = T (e_p o b_p);   gamma_p = a_p o b_p / sum(a_p o b_p).

Positions run 0 .. N (N = the sum of the spans); position 0 is column 0, row l covers positions P_{l-1} + 1 .. P_l.  Like
tests/transref.py (whose `row_key_ids` / `emission_table` it reuses) it is built from what a manager's getters hand out and shares
nothing with the kernel: no generators of T, no float vectors, no floor, no blocks or checkpoints.  Written for clarity, not speed:
two Python loops over the positions (about 10 s per million positions at M = 64).  Memory is one vector per row boundary plus one
SLAB of gamma: `slabs` hands the marginals out row by row, from the last row to the first, and everything else is built on it."""
import numpy as np

from transref import emission_table, row_key_ids  # noqa: F401  (re-exported for the tests)

EPS = 2.0 ** -52


def slabs(pi, T, keys, E, obs):
    """Generator of (first position, G [n x M]) with G[t] = gamma at position first + t: one slab per row of `obs` (span, key...),
    from the LAST row to the first, then (0, [1 x M]) for position 0."""
    pi = np.asarray(pi, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    obs = np.asarray(obs)
    M, L = len(pi), len(obs)
    spans = obs[:, 0].astype(np.int64)
    kid = row_key_ids(obs, keys)
    Tt = np.ascontiguousarray(T.T)
    A = np.empty((L + 1, M))                               # forward vectors at the row boundaries
    a = pi / pi.sum()
    A[0] = a
    for l in range(L):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            a /= a.sum()
        A[l + 1] = a
    P = np.concatenate([[0], np.cumsum(spans)])
    b = np.ones(M) / M                                     # b at the last position
    for l in range(L - 1, -1, -1):
        e, s = E[kid[l]], int(spans[l])
        G = np.empty((s, M))
        a = A[l]
        for t in range(s):                                 # G[t] = a at position P[l] + 1 + t
            a = e * (Tt @ a)
            a /= a.sum()
            G[t] = a
        for t in range(s - 1, -1, -1):
            G[t] *= b
            G[t] /= G[t].sum()
            b = T @ (e * b)
            b /= b.sum()
        yield int(P[l]) + 1, G
    g = A[0] * b
    yield 0, (g / g.sum())[None, :]


def positions(pi, T, keys, E, obs, pos0=0, pos1=None, step=1):
    """[M x npos]: gamma on the grid range(pos0, pos1, step) (default: every position)."""
    N = int(np.asarray(obs)[:, 0].sum())
    pos1 = N + 1 if pos1 is None else pos1
    grid = np.arange(pos0, pos1, step, dtype=np.int64)
    out = np.empty((len(pi), len(grid)))
    for first, G in slabs(pi, T, keys, E, obs):
        j0, j1 = np.searchsorted(grid, [first, first + len(G)])
        if j1 > j0:
            out[:, j0:j1] = G[grid[j0:j1] - first].T
    return out


def window_sums(first, G, W, nwin, out):
    """Adds the slab's positions to their windows: position p >= 1 is base pair p - 1, window (p - 1) // W.  out [M x nwin]."""
    if first == 0:
        return
    w = (np.arange(first, first + len(G), dtype=np.int64) - 1) // W
    cuts = np.concatenate([[0], np.nonzero(np.diff(w))[0] + 1])
    out[:, w[cuts]] += np.add.reduceat(G, cuts, axis=0).T


def windows_exact(pi, T, keys, E, obs, W):
    """[M x ceil(N / W)]: the average of gamma_p over the positions p with p - 1 in [w W, min((w + 1) W, N))."""
    N = int(np.asarray(obs)[:, 0].sum())
    nwin = -(-N // W)
    out = np.zeros((len(pi), nwin))
    for first, G in slabs(pi, T, keys, E, obs):
        window_sums(first, G, W, nwin, out)
    lo = np.arange(nwin, dtype=np.int64) * W
    return out / (np.minimum(lo + W, N) - lo)


def row_sums(pi, T, keys, E, obs):
    """[M x (L + 1)]: sum of gamma_p over the positions of every row (column 0: gamma_0) - s_l times the per-row posterior."""
    L = len(obs)
    out = np.empty((len(pi), L + 1))
    l = L
    for first, G in slabs(pi, T, keys, E, obs):
        out[:, l] = G.sum(axis=0)
        l -= 1
    assert l == -1
    return out
