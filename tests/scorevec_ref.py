"""numpy restatement of the VECTOR form of the score track's transition part (smcpp_amd/csrc/score_vec_dev.hpp), on top of the dense
oracle tests/scoreref.py.  No GPU, no engine: tables in, numbers out.

The Jacobian of the model's transition matrix is semiseparable.  With c0 = 1e-5 / (M + 1) and four coefficient planes per direction
(smcpp_host_score_planes), entry by entry

    dT_d(i, j) = cL_d(j) T(i, j)  (i > j),     (cP_d(i) + cW_d(j)) (T(i, j) - c0)  (i < j),     cD_d(j) T(j, j)  (i == j),

so a row's  sum_ij O(i, j) dT_d(i, j) / T(i, j)  over its dense xi sum O needs four vectors that do not depend on d:

    D(j) = O(j, j),   L(j) = sum_{i>j} O(i, j),   U1(j) = sum_{i<j} O(i, j) phi(i, j),   U2(i) = sum_{j>i} O(i, j) phi(i, j),

phi = (T - c0) / T the share of an upper entry that is not the uniform mix.  `xi_sums` forms O exactly as scoreref.score_rows does
(the same operations in the same order; tests/test_score_planes.py holds its contraction with dT / T to scoreref's transition part),
`shares` takes the four vectors, `contract` meets the planes."""
import numpy as np

from transref import row_key_ids

EPS = 2.0 ** -52


def dense_from_planes(T, cD, cL, cW, cP):
    """dT [M, M, nder] rebuilt entry by entry from the planes [nder, M].  -> (dT, the sum of the absolute terms of every entry)."""
    T = np.asarray(T, dtype=np.float64)
    M = len(T)
    c0 = 1e-5 / (M + 1)
    i, j = np.indices((M, M))
    Tn = T[None]
    val = np.where(i > j, cL[:, None, :] * Tn, np.where(i < j, (cP[:, :, None] + cW[:, None, :]) * (Tn - c0), cD[:, None, :] * Tn))
    mag = np.where(i > j, np.abs(cL[:, None, :]) * Tn,
                   np.where(i < j, (np.abs(cP[:, :, None]) + np.abs(cW[:, None, :])) * (Tn + c0), np.abs(cD[:, None, :]) * Tn))
    return np.moveaxis(val, 0, 2), np.moveaxis(mag, 0, 2)


def xi_sums(pi, T, keys, E, obs, cells=1 << 22):
    """-> O [L, M, M]: the dense xi_p(i, j) of scoreref.score_rows added up over the positions of every row."""
    pi, T, E = (np.asarray(x, dtype=np.float64) for x in (pi, T, E))
    obs = np.asarray(obs)
    M, L = len(pi), len(obs)
    spans = obs[:, 0].astype(np.int64)
    kid = row_key_ids(obs, keys)
    A = np.empty((L + 1, M))
    a = pi / pi.sum()
    A[0] = a
    Tt = np.ascontiguousarray(T.T)
    for l in range(L):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            a /= a.sum()
        A[l + 1] = a
    out = np.zeros((L, M, M))
    b = np.ones(M) / M
    blk = max(1, cells // (M * M))
    for l in range(L - 1, -1, -1):
        e, s = E[kid[l]], int(spans[l])
        X = np.empty((s, M))
        a = A[l]
        for t in range(s):
            X[t] = a
            a = e * (Tt @ a)
            a /= a.sum()
        W = np.empty((s, M))
        for t in range(s - 1, -1, -1):
            W[t] = e * b
            b = T @ W[t]
            b /= b.sum()
        for t0 in range(0, s, blk):
            xi = X[t0:t0 + blk, :, None] * T[None, :, :] * W[t0:t0 + blk, None, :]
            xi /= xi.sum(axis=(1, 2), keepdims=True)
            out[l] += xi.sum(axis=0)
    return out


def shares(O, T, absolute=False):
    """The four vectors of every row from its xi sum: -> D, L, U1, U2, each [rows, M].  absolute: with (T + c0) / T for phi - the sum
    of the absolute terms of T - c0, the scale of what the difference's rounding leaves in an upper entry."""
    T = np.asarray(T, dtype=np.float64)
    M = len(T)
    c0 = 1e-5 / (M + 1)
    phi = np.triu((T + c0 if absolute else T - c0) / T, 1)
    up = O * phi[None]
    return (np.einsum("ljj->lj", O), np.tril(O, -1).sum(axis=1), up.sum(axis=1), up.sum(axis=2))


def contract(D, L, U1, U2, cD, cL, cW, cP):
    """-> transition part [nder, rows]."""
    return (D @ cD.T + L @ cL.T + U1 @ cW.T + U2 @ cP.T).T
