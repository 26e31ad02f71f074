"""tests/posref.py, the oracle of the per-position posterior products, against brute force (CPU only): every path of a 3-state
hidden Markov model over 6 positions enumerated, the sums over the rows against the dense xi of tests/transref.py's formula, the
window oracle at one base pair per window and at one window."""
import itertools

import numpy as np

import posref


def small_hmm(M, K, seed):
    rng = np.random.default_rng(seed)
    pi = rng.random(M) + 0.1
    pi /= pi.sum()
    T = rng.random((M, M)) + 0.05 + 2.0 * np.eye(M)
    T /= T.sum(axis=1, keepdims=True)
    E = rng.random((K, M)) + 0.01
    keys = np.arange(K, dtype=np.int32)[:, None] * np.array([[1, 2]], dtype=np.int32)
    return pi, T, keys, E


def rows_of(spans, kids, keys):
    return np.array([[s, *keys[k]] for s, k in zip(spans, kids)], dtype=np.int32)


def brute_force(pi, T, E, kid_of_pos):
    """gamma [M x (N + 1)] from the enumeration of every path x_0 .. x_N: weight pi(x_0) prod_p T(x_{p-1}, x_p) e_p(x_p)."""
    M, N = len(pi), len(kid_of_pos)
    out = np.zeros((M, N + 1))
    for path in itertools.product(range(M), repeat=N + 1):
        w = pi[path[0]]
        for p in range(1, N + 1):
            w *= T[path[p - 1], path[p]] * E[kid_of_pos[p - 1], path[p]]
        for p, x in enumerate(path):
            out[x, p] += w
    return out / out.sum(axis=0)


def test_every_path_of_a_small_model():
    pi, T, keys, E = small_hmm(3, 3, 1)
    spans, kids = [1, 3, 2], [0, 2, 1]
    obs = rows_of(spans, kids, keys)
    want = brute_force(pi, T, E, np.repeat(kids, spans))
    got = posref.positions(pi, T, keys, E, obs)
    assert got.shape == want.shape == (3, 7)
    assert np.max(np.abs(got - want)) <= 16 * posref.EPS, np.max(np.abs(got - want))
    assert np.max(np.abs(got.sum(axis=0) - 1.0)) <= 4 * posref.EPS
    # grids are taken from the same columns
    for pos0, pos1, step in ((0, 7, 1), (0, 7, 2), (1, 7, 3), (2, 5, 1), (6, 7, 1), (3, 4, 5)):
        assert np.array_equal(posref.positions(pi, T, keys, E, obs, pos0, pos1, step), got[:, pos0:pos1:step])


def dense_marginals(pi, T, E, kid_of_pos):
    """gamma_p(j) = sum_i xi_p(i, j), xi_p(i, j) = a_{p-1}(i) T(i, j) e_p(j) b_p(j): tests/transref.py's formula, all vectors kept."""
    M, N = len(pi), len(kid_of_pos)
    a = np.empty((N + 1, M))
    a[0] = pi
    for p in range(1, N + 1):
        a[p] = E[kid_of_pos[p - 1]] * (T.T @ a[p - 1])
        a[p] /= a[p].sum()
    b = np.empty((N + 1, M))
    b[N] = 1.0
    for p in range(N, 0, -1):
        b[p - 1] = T @ (E[kid_of_pos[p - 1]] * b[p])
        b[p - 1] /= b[p - 1].sum()
    out = np.empty((M, N + 1))
    out[:, 0] = a[0] * b[0] / (a[0] * b[0]).sum()
    for p in range(1, N + 1):
        xi = a[p - 1][:, None] * T * (E[kid_of_pos[p - 1]] * b[p])[None, :]
        out[:, p] = xi.sum(axis=0) / xi.sum()
    return out


def test_row_sums_against_the_dense_xi():
    pi, T, keys, E = small_hmm(7, 4, 2)
    rng = np.random.default_rng(3)
    spans = [1, 64, 65, 1, 1, 130, 2, 7]
    kids = rng.integers(0, 4, len(spans))
    obs = rows_of(spans, kids, keys)
    dense = dense_marginals(pi, T, E, np.repeat(kids, spans))
    got = posref.positions(pi, T, keys, E, obs)
    assert np.max(np.abs(got - dense)) <= 64 * posref.EPS, np.max(np.abs(got - dense))
    sums = posref.row_sums(pi, T, keys, E, obs)
    P = np.concatenate([[0], np.cumsum(spans)])
    assert sums.shape == (7, len(spans) + 1)
    assert np.max(np.abs(sums[:, 0] - dense[:, 0])) <= 64 * posref.EPS
    for l, s in enumerate(spans):
        want = dense[:, P[l] + 1:P[l + 1] + 1].sum(axis=1)
        assert np.max(np.abs(sums[:, l + 1] - want)) <= (s + 64) * posref.EPS, (l, s)
        assert abs(sums[:, l + 1].sum() - s) <= (s + 64) * posref.EPS * s


def test_windows_at_one_base_pair_and_at_one_window():
    pi, T, keys, E = small_hmm(5, 3, 4)
    spans, kids = [3, 1, 70, 1, 12], [0, 1, 2, 0, 1]
    obs = rows_of(spans, kids, keys)
    N = sum(spans)
    g = posref.positions(pi, T, keys, E, obs)
    w1 = posref.windows_exact(pi, T, keys, E, obs, 1)
    assert w1.shape == (5, N) and np.array_equal(w1, g[:, 1:])
    for W in (N, N + 5):
        wn = posref.windows_exact(pi, T, keys, E, obs, W)
        assert wn.shape == (5, 1)
        assert np.max(np.abs(wn[:, 0] - g[:, 1:].mean(axis=1))) <= (N + 8) * posref.EPS
    W = 10
    ww = posref.windows_exact(pi, T, keys, E, obs, W)
    assert ww.shape == (5, -(-N // W))
    for w in range(ww.shape[1]):
        want = g[:, 1 + w * W:1 + min((w + 1) * W, N)].mean(axis=1)
        assert np.max(np.abs(ww[:, w] - want)) <= (W + 8) * posref.EPS
    assert np.max(np.abs(ww.sum(axis=0) - 1.0)) <= (W + 8) * posref.EPS
