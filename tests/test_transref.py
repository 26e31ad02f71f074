"""The numpy oracle of the posterior transition products (tests/transref.py) pinned on the CPU: hand-worked values, a brute-force
enumeration of every state path, and the reference-pinned statistic - summed over the rows of a contig, stay / up / down are the
trace and the strict upper / lower triangle sums of the contig's xisum, which the goldens hold as the compiled reference computed it.

Bound of the golden check: STAT_TOL = 5e-6 relative, the project's bar for xisum (tests/test_gpu_parity.py).  Measured here: worst over
G1, G3 and G4 1.8e-7 (G4: 1.7e-9, 1.1e-7, 9.4e-8 for stay, up, down) - the float alpha of the reference's algorithm."""
import itertools

import numpy as np
import pytest

import transref
from conftest import load_golden

STAT_TOL = 5e-6


def test_hand_worked_two_states_three_rows():
    """T = [[0.9, 0.1], [0.2, 0.8]] has the stationary distribution (2/3, 1/3).  With pi stationary and an emission that tells nothing,
    every position holds xi = diag(pi) T: stay = 2/3 0.9 + 1/3 0.8 = 13/15, up = 2/3 0.1 = 1/15, down = 1/3 0.2 = 1/15.  Rows of spans
    1, 2, 1 hold that once, twice, once."""
    T = np.array([[0.9, 0.1], [0.2, 0.8]])
    pi = np.array([2.0, 1.0]) / 3.0
    keys = np.array([[0, 0, 0], [1, 0, 0]])
    E = np.ones((2, 2))
    obs = np.array([[1, 0, 0, 0], [2, 1, 0, 0], [1, 0, 0, 0]])
    v = transref.transitions(pi, T, keys, E, obs)
    want = np.array([[0.0, 13 / 15, 26 / 15, 13 / 15], [0.0, 1 / 15, 2 / 15, 1 / 15], [0.0, 1 / 15, 2 / 15, 1 / 15]])
    assert v.shape == (3, 4) and np.allclose(v, want, rtol=0, atol=4 * transref.EPS)
    assert np.all(v[:, 0] == 0.0)
    # one row of span 1 from pi = (0.5, 0.5): xi = diag(pi) T
    v1 = transref.transitions(np.array([0.5, 0.5]), T, keys, E, obs[:1])
    assert np.allclose(v1[:, 1], [0.85, 0.05, 0.1], rtol=0, atol=4 * transref.EPS)


def test_against_every_state_path():
    """Emissions that tell something: the expectation over all 2^5 state paths of a contig of spans 1, 2, 1 (four positions)."""
    T = np.array([[0.9, 0.1], [0.2, 0.8]])
    pi = np.array([0.3, 0.7])
    keys = np.array([[0, 0, 0], [1, 0, 0]])
    E = np.array([[0.5, 0.1], [0.05, 0.4]])
    obs = np.array([[1, 0, 0, 0], [2, 1, 0, 0], [1, 0, 0, 0]])
    em = [E[0], E[1], E[1], E[0]]                          # per position
    row_of = [1, 2, 2, 3]
    want = np.zeros((3, 4))
    total = 0.0
    for path in itertools.product((0, 1), repeat=5):
        p = pi[path[0]]
        for t in range(4):
            p *= T[path[t], path[t + 1]] * em[t][path[t + 1]]
        total += p
        for t in range(4):
            kind = 0 if path[t + 1] == path[t] else 1 if path[t + 1] > path[t] else 2
            want[kind, row_of[t]] += p
    want /= total
    v = transref.transitions(pi, T, keys, E, obs)
    assert np.allclose(v, want, rtol=0, atol=8 * transref.EPS)
    assert np.allclose(v.sum(axis=0), [0, 1, 2, 1], rtol=0, atol=8 * transref.EPS)


def test_window_oracle_small():
    """Rows of spans 3, 1, 4 in windows of 2: by hand, and against the per-base-pair expansion; block size 1 gives the same."""
    v = np.array([[0.0, 3.0, 0.5, 2.0], [0.0, 0.0, 0.25, 1.0], [0.0, 0.0, 0.25, 1.0]])
    spans = [3, 1, 4]
    out, cov = transref.transition_windows(v, spans, 2)
    per_bp = np.repeat(v[:, 1:] / np.array(spans), spans, axis=1)
    assert np.array_equal(cov, [2, 2, 2, 2])
    assert np.allclose(out, per_bp.reshape(3, 4, 2).sum(axis=2), rtol=0, atol=4 * transref.EPS)
    assert np.allclose(out[0], [2.0, 1.5, 1.0, 1.0])
    out1, _ = transref.transition_windows(v, spans, 2, block=1)
    assert np.allclose(out1, out, rtol=0, atol=4 * transref.EPS)
    out3, cov3 = transref.transition_windows(v, spans, 3)
    assert np.array_equal(cov3, [3, 3, 2]) and np.allclose(out3.sum(axis=0), cov3)


@pytest.mark.parametrize("name", ["G1_M16_n4", "G3_M32_n10_2Mbp", "G4_M64_n20_2Mbp"])
def test_row_sums_are_the_triangles_of_the_golden_xisum(name):
    g = load_golden(name)
    v = transref.transitions(g["pi"], g["T"], g["keys"], g["E"], g["obs"])
    L = len(g["obs"])
    assert v.shape == (3, L + 1) and np.all(v[:, 0] == 0.0) and np.all(v >= 0.0)
    spans = g["obs"][:, 0].astype(float)
    assert np.max(np.abs(v[:, 1:].sum(axis=0) - spans) / spans) <= 1e-12
    X = np.asarray(g["xisum"], dtype=np.float64)
    want = np.array([np.trace(X), np.triu(X, 1).sum(), np.tril(X, -1).sum()])
    got = v.sum(axis=1)
    rel = np.abs(got - want) / want
    print(f"{name}: sum over rows stay / up / down {got}, golden xisum {want}, relative {rel}")
    assert np.all(rel <= STAT_TOL), (name, rel)
