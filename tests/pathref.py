"""numpy oracle of the posterior path sampler (smcpp_posterior_sample_rows / _sample_positions): forward filtering and backward
sampling over the PURE hidden Markov model - initial distribution pi, transition matrix T [M x M], one emission vector per key - in
float64, with its own Philox4x32-10.

Contract (include/smcpp_engine.h): positions 0 .. N, a_0 = pi, a_p = e_p o (T^T a_{p-1}); x_N is drawn with weights a_N(i), x_q given
x_{q+1} = j with weights a_q(i) T(i, j); every draw is an inverse CDF in ascending state order, C_i = w_0 + .. + w_i,
x = min{i : C_i > u C_{M-1}} clamped to M - 1; u of the draw of x_q of path k of contig c comes from Philox with key = the seed's two
words and counter = (q lo, q hi, k, c).

Like tests/transref.py it is built from what a manager's getters hand out and shares nothing with the kernel: dense a_q at every
position, no generators of T, no floats, no blocks.  Memory is one vector per row boundary plus one row's interior."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))


def philox4x32(counter, key):
    """Philox4x32-10.  counter [..., 4], key [..., 2] (broadcast against each other), 32-bit words -> [..., 4] uint64 holding 32-bit words."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] & M32 for i in range(4))
    k0, k1 = key[..., 0] & M32, key[..., 1] & M32
    for _ in range(10):
        p0 = PHILOX_M[0] * c0                              # (32 x 32 bits: fits 64)
        p1 = PHILOX_M[1] * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + PHILOX_W[0]) & M32
        k1 = (k1 + PHILOX_W[1]) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def words_to_uniform(w0, w1):
    """u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 in [0, 1)."""
    w0 = np.asarray(w0, dtype=np.uint64)
    w1 = np.asarray(w1, dtype=np.uint64)
    return (((w0 >> np.uint64(5)) << np.uint64(26)) + (w1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def uniforms(seed, c, k, q):
    """The uniform of the draw of x_q of path k of contig c under `seed`; k and q broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k, q = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(q, dtype=np.uint64))
    ctr = np.stack([q & M32, q >> np.uint64(32), k & M32, np.full(q.shape, int(c), dtype=np.uint64)], axis=-1)
    out = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return words_to_uniform(out[..., 0], out[..., 1])


def _row_key_ids(obs, keys):
    lut = {tuple(int(x) for x in k): i for i, k in enumerate(np.asarray(keys))}
    return np.array([lut[tuple(int(x) for x in r[1:])] for r in np.asarray(obs)], dtype=np.int64)


def _setup(pi, T, keys, E, obs):
    pi = np.asarray(pi, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    obs = np.asarray(obs)
    spans = obs[:, 0].astype(np.int64)
    return pi / pi.sum(), T, np.ascontiguousarray(T.T), E, spans, _row_key_ids(obs, keys)


def _boundaries(pi, Tt, E, spans, kid):
    """a at position 0 and at the last position of every row: [L + 1][M]."""
    A = np.empty((len(spans) + 1, len(pi)))
    a = pi
    A[0] = a
    for l in range(len(spans)):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            a /= a.sum()
        A[l + 1] = a
    return A


def _interior(a, Tt, e, s):
    """a at the s positions of a row that starts behind vector `a`: [s][M]."""
    X = np.empty((s, len(a)))
    for t in range(s):
        a = e * (Tt @ a)
        a /= a.sum()
        X[t] = a
    return X


def _draw(W, u):
    """Inverse CDF in ascending state order on every line of W [.., M] -> states."""
    C = np.cumsum(W, axis=-1)
    hit = C > (u * C[..., -1])[..., None]
    return np.where(hit.any(axis=-1), hit.argmax(axis=-1), W.shape[-1] - 1).astype(np.int32)


def _path_ids(paths):
    return np.arange(paths, dtype=np.int64) if np.isscalar(paths) else np.asarray(paths, dtype=np.int64)


def sample(pi, T, keys, E, obs, seed, c, paths):
    """The oracle's own sampler, vectorised over the paths: paths = a count (paths 0 .. count - 1) or the path indices.
    -> int32 [n paths][N + 1]."""
    pi, T, Tt, E, spans, kid = _setup(pi, T, keys, E, obs)
    ks = _path_ids(paths)
    A = _boundaries(pi, Tt, E, spans, kid)
    N = int(spans.sum())
    out = np.empty((len(ks), N + 1), dtype=np.int32)
    j = None
    q = N
    for l in range(len(spans) - 1, -1, -1):
        X = _interior(A[l], Tt, E[kid[l]], int(spans[l]))
        for t in range(int(spans[l]) - 1, -1, -1):
            W = np.broadcast_to(X[t], (len(ks), len(pi))) if j is None else X[t][None, :] * Tt[j]
            j = _draw(W, uniforms(seed, c, ks, q))
            out[:, q] = j
            q -= 1
    assert q == 0
    W = np.broadcast_to(A[0], (len(ks), len(pi))) if j is None else A[0][None, :] * Tt[j]
    out[:, 0] = _draw(W, uniforms(seed, c, ks, 0))
    return out


def draw_margins(pi, T, keys, E, obs, seed, c, k0, paths, cells=1 << 22):
    """For every draw of every given path (paths [n][N + 1]: path k0 + i in line i) the distance by which u lies outside
    [C_{x-1}, C_x) / C_{M-1}, the CDF conditioned on the path's OWN next state; 0 when u is inside (a clamped x = M - 1 has no upper
    end).  One row's interior in memory at a time.  -> float64 [n][N + 1]."""
    pi, T, Tt, E, spans, kid = _setup(pi, T, keys, E, obs)
    paths = np.asarray(paths)
    n, M = len(paths), len(pi)
    N = int(spans.sum())
    assert paths.shape == (n, N + 1), (paths.shape, N)
    assert paths.min() >= 0 and paths.max() < M
    ks = k0 + np.arange(n, dtype=np.int64)
    A = _boundaries(pi, Tt, E, spans, kid)
    out = np.empty((n, N + 1))

    def margins(X, q0):
        # X [s][M]: a at positions q0 .. q0 + s - 1
        s = len(X)
        qs = q0 + np.arange(s, dtype=np.int64)
        for i in range(n):
            x = paths[i, q0:q0 + s].astype(np.int64)
            nxt = paths[i, q0 + 1:q0 + s + 1]                            # (position N, the last of its slice, has no successor)
            W = X.copy()
            W[:len(nxt)] *= Tt[nxt]
            C = np.cumsum(W, axis=1)
            tot = C[:, -1]
            thr = uniforms(seed, c, ks[i], qs) * tot
            at = np.arange(s)
            lo = np.where(x > 0, C[at, np.maximum(x - 1, 0)], 0.0)
            hi = np.where(x < M - 1, C[at, x], np.inf)
            out[i, q0:q0 + s] = np.maximum(np.maximum(lo - thr, thr - hi), 0.0) / tot

    blk = max(1, cells // M)
    margins(A[0][None, :], 0)
    P = 0
    for l in range(len(spans)):
        s = int(spans[l])
        X = _interior(A[l], Tt, E[kid[l]], s)
        for t0 in range(0, s, blk):
            margins(X[t0:t0 + blk], P + 1 + t0)
        P += s
    return out


def marginals(pi, T, keys, E, obs):
    """Float64 forward-backward: the posterior marginal of every position, [N + 1][M]."""
    pi, T, Tt, E, spans, kid = _setup(pi, T, keys, E, obs)
    N, M = int(spans.sum()), len(pi)
    ev = np.repeat(kid, spans)
    F = np.empty((N + 1, M))
    a = pi
    F[0] = a
    for p in range(1, N + 1):
        a = E[ev[p - 1]] * (Tt @ a)
        a /= a.sum()
        F[p] = a
    b = np.ones(M) / M
    for p in range(N, -1, -1):
        F[p] *= b
        F[p] /= F[p].sum()
        if p > 0:
            b = T @ (E[ev[p - 1]] * b)
            b /= b.sum()
    return F


def rows_from_positions(path, spans):
    """Per row of spans `spans` from the states at positions 0 .. N (path [.., N + 1]): (state, up, down), each int32 [.., L + 1] -
    the state at the row's last position and the number of positions p of the row with x_{p-1} < x_p / x_{p-1} > x_p; column 0:
    the state at position 0 and zeros."""
    path = np.asarray(path)
    spans = np.asarray(spans, dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(spans)])
    assert path.shape[-1] == P[-1] + 1
    d = np.diff(path.astype(np.int64), axis=-1)                            # d[.., p - 1]: the transition into position p
    shape = path.shape[:-1] + (len(spans) + 1,)
    state = path[..., P].astype(np.int32)
    up, down = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    up[..., 1:] = np.add.reduceat((d > 0).astype(np.int32), P[:-1], axis=-1)
    down[..., 1:] = np.add.reduceat((d < 0).astype(np.int32), P[:-1], axis=-1)
    return state, up, down


def frequency_bound(g, K, tol):
    """Bar on |frequency over K independent draws - probability g| per cell: sqrt(60 g (1 - g) / K) + 10 / K is Bernstein's
    inequality at t = 30 (an exact sampler misses it with probability 2 e^-30 = 2e-13 per cell); `tol` is the bar on g itself."""
    g = np.asarray(g, dtype=np.float64)
    return np.sqrt(60.0 * g * (1.0 - g) / K) + 10.0 / K + tol


def state_frequencies(paths, M):
    """[N + 1][M]: the share of the paths (paths [K][N + 1]) in every state at every position."""
    paths = np.asarray(paths)
    K, P = paths.shape
    f = np.zeros((P, M))
    np.add.at(f, (np.broadcast_to(np.arange(P), (K, P)).ravel(), paths.ravel()), 1.0)
    return f / K
