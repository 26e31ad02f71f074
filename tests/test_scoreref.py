"""The score oracle (tests/scoreref.py) against finite differences of its own log-likelihood, and smcpp_amd.evidence.information /
covariance on hand-made tracks against explicit loops.  No GPU.

The model is a synthetic hidden Markov model whose tables are smooth positive functions of three parameters, each direction with
basis functions of its own:
    pi(i) = exp(c_i + sum_d theta_d f_d(i)),   T(i, j) = exp(-|i - j| / 2 + sum_d theta_d g_d(i, j)),   E[k](i) = exp(-u_k(i) + sum_d theta_d h_d(k, i)),
so the Jacobians are exact (d pi_d = pi f_d, ...) and the tables are NOT normalised - Fisher's identity does not need them to be, and
the oracle must not rely on it.  The bar: the oracle's sum over the rows within 1e-8 of sum_l |row score| of the central difference
(h = 1e-5) of the log-likelihood; the measured distance is 2e-10 .. 3e-10 (the difference's own rounding: |loglik| 2^-52 / h)."""
import numpy as np
import pytest

import scoreref

NDER = 3
H = 1e-5
BAR = 1e-8
CASES = [(2, 3, 40, 0), (5, 4, 50, 1), (16, 6, 60, 2)]          # M, K, rows, seed


def tables(theta, M, K, which=(True, True, True)):
    """-> pi, T, E, dpi [M, 3], dT [M, M, 3], dE [K, M, 3]; `which`: the tables that follow theta (the others stay at theta = 0)."""
    th = np.asarray(theta, dtype=np.float64)
    i = np.arange(M, dtype=np.float64)
    k = np.arange(K, dtype=np.float64)
    I, J = np.meshgrid(i, i, indexing="ij")
    KK, II = np.meshgrid(k, i, indexing="ij")
    f = np.stack([np.sin(i + 1.0), np.cos(2.0 * i + 0.3), ((i + 0.5) / M) ** 2], axis=-1)
    g = np.stack([np.sin(I + 2.0 * J), np.cos(0.7 * I * J + 1.0), np.tanh((I - J) / 3.0)], axis=-1)
    h = np.stack([np.cos(KK + 0.5 * II), np.sin(1.3 * KK * (II + 1.0)), 1.0 / (1.0 + KK + II)], axis=-1)
    tp, tt, te = (th if w else np.zeros(NDER) for w in which)
    pi = np.exp(-0.3 * np.abs(i - M / 3.0) + f @ tp)
    T = np.exp(-0.5 * np.abs(I - J) + g @ tt)
    E = np.exp(-(0.5 + 0.4 * np.cos(KK * 1.7 + II * 0.9) ** 2 + 0.2 * KK) + h @ te)
    on = [float(w) for w in which]
    return pi, T, E, pi[:, None] * f * on[0], T[:, :, None] * g * on[1], E[:, :, None] * h * on[2]


def rows(M, K, L, seed):
    rng = np.random.default_rng(seed)
    spans = rng.choice([1, 1, 1, 2, 3, 7, 20], size=L)
    spans[[3, 11, 17, 29]] = (65, 2, 7, 1)                         # every span the issue names is there, 65 crosses a block of 64
    keys = np.stack([np.arange(K), np.zeros(K, dtype=np.int64), np.arange(K) % 2], axis=1)
    kid = rng.integers(0, K, size=L)
    kid[:K] = np.arange(K)
    obs = np.concatenate([spans[:, None], keys[kid]], axis=1)
    return keys, obs


def fd(theta, M, K, keys, obs, which):
    """Central difference of the log-likelihood in every direction, the tables of `which` following theta."""
    def ll(th):
        pi, T, E = tables(th, M, K, which)[:3]
        return scoreref.loglik(pi, T, keys, E, obs)
    out = np.empty(NDER)
    for d in range(NDER):
        e = np.zeros(NDER)
        e[d] = H
        out[d] = (ll(theta + e) - ll(theta - e)) / (2 * H)
    return out


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"M{c[0]}-K{c[1]}")
def case(request):
    M, K, L, seed = request.param
    theta = np.array([0.11, -0.07, 0.05])
    keys, obs = rows(M, K, L, seed)
    pi, T, E, dpi, dT, dE = tables(theta, M, K)
    parts = scoreref.score_rows(pi, T, keys, E, dpi, dT, dE, obs)
    return M, K, theta, keys, obs, parts


def test_total_matches_the_finite_difference_of_the_loglik(case):
    M, K, theta, keys, obs, parts = case
    assert parts.shape == (3, NDER, len(obs) + 1) and set(obs[:, 0]) >= {1, 2, 7, 65}
    total = parts.sum(axis=0)
    scale = np.abs(total).sum(axis=1)
    num = fd(theta, M, K, keys, obs, (True, True, True))
    worst = float(np.max(np.abs(total.sum(axis=1) - num) / scale))
    print(f"M = {M}: |sum of row scores - central difference| / sum |row score| = {worst:.3g}")
    assert worst <= BAR, worst


def test_each_part_matches_the_finite_difference_of_its_table(case):
    M, K, theta, keys, obs, parts = case
    scale = np.abs(parts.sum(axis=0)).sum(axis=1)
    for x, which in enumerate(((True, False, False), (False, False, True), (False, True, False))):     # initial, emission, transition
        # (the other tables at theta = 0 are another model: the part is taken on THAT model's oracle run)
        pi, T, E, dpi, dT, dE = tables(theta, M, K, which)
        p = scoreref.score_rows(pi, T, keys, E, dpi, dT, dE, obs)
        others = [y for y in range(3) if y != x]
        assert not p[others].any()
        num = fd(theta, M, K, keys, obs, which)
        worst = float(np.max(np.abs(p[x].sum(axis=1) - num) / scale))
        print(f"M = {M}, part {x}: {worst:.3g}")
        assert worst <= BAR, (x, worst)
    # where the parts live: the initial part in column 0 alone, the others in the rows alone
    assert not parts[0, :, 1:].any() and not parts[1:, :, 0].any() and parts[0, :, 0].any()


def test_windows_oracle():
    rng = np.random.default_rng(5)
    spans = rng.choice([1, 2, 7, 65], size=30)
    v = rng.standard_normal((NDER, 31))
    total = int(spans.sum())
    for W in (1, 10, 100, total):
        out, mag = scoreref.score_windows(v, spans, W)
        assert out.shape == (NDER, -(-total // W)) and np.all(mag >= np.abs(out) - 1e-12)
        assert np.allclose(out.sum(axis=1), v.sum(axis=1), rtol=0, atol=1e-12 * np.abs(v).sum())
        # by hand, base pair by base pair
        bp = np.repeat(v[:, 1:] / spans, spans, axis=1)
        hand = np.stack([bp[:, w * W:(w + 1) * W].sum(axis=1) for w in range(out.shape[1])], axis=1)
        hand[:, 0] += v[:, 0]
        assert np.allclose(out, hand, rtol=0, atol=1e-12 * np.abs(v).sum())


# ---- smcpp_amd.evidence on hand-made tracks ----
def test_information_and_covariance_against_loops():
    from smcpp_amd.evidence import covariance, information
    rng = np.random.default_rng(2)
    tracks = [rng.standard_normal((NDER, 11)), rng.standard_normal((NDER, 4)), rng.standard_normal((NDER, 7))]
    for block in (1, 3, 5):
        blocks = []
        for t in tracks:                                             # as compare_tracks forms them: per contig, the last may hold fewer
            for w0 in range(0, t.shape[1], block):
                blocks.append([sum(t[d, w] for w in range(w0, min(w0 + block, t.shape[1]))) for d in range(NDER)])
        B = len(blocks)
        mean = [sum(b[d] for b in blocks) / B for d in range(NDER)]
        J = [[B / (B - 1.0) * sum((b[d] - mean[d]) * (b[e] - mean[e]) for b in blocks) for e in range(NDER)] for d in range(NDER)]
        info = information(tracks, block)
        assert info["blocks"].shape == (B, NDER)
        assert np.max(np.abs(info["blocks"] - np.array(blocks))) <= 1e-12
        assert np.max(np.abs(info["score"] - np.array([sum(b[d] for b in blocks) for d in range(NDER)]))) <= 1e-12
        assert np.max(np.abs(info["J"] - np.array(J))) <= 1e-12 * max(1.0, np.max(np.abs(J)))
        cov = covariance(info)
        assert np.max(np.abs(cov["cov"] - np.linalg.inv(np.array(J)))) <= 1e-12 * np.max(np.abs(np.linalg.inv(np.array(J)))) * np.linalg.cond(np.array(J))
        assert np.max(np.abs(cov["se"] - np.sqrt(np.diag(np.linalg.inv(np.array(J)))))) <= 1e-12 * np.linalg.cond(np.array(J))
    # a direction the data say nothing about: dropped by rcond, variance 0
    flat = [np.concatenate([t[:2], np.zeros((1, t.shape[1]))]) for t in tracks]
    cov = covariance(information(flat, 1))
    assert cov["se"][2] == 0.0 and np.all(cov["se"][:2] > 0.0)


def test_information_refuses_fewer_than_two_blocks():
    from smcpp_amd.evidence import compare_tracks, information
    one = [np.ones((NDER, 4))]
    with pytest.raises(ValueError, match="at least two"):
        information(one, 4)
    with pytest.raises(ValueError, match="at least two"):            # the same refusal as compare_tracks'
        compare_tracks([np.ones(4)], [np.zeros(4)], 4)
    with pytest.raises(ValueError, match="block < 1"):
        information(one, 0)
    with pytest.raises(ValueError, match="shape"):
        information([np.ones(4)], 1)
    assert information(one, 2)["blocks"].shape == (2, NDER)
