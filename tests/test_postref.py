"""The numpy oracles of the posterior products (tests/postref.py) on a case worked by hand and on a random case against a second,
independent formulation.  No device needed."""
from fractions import Fraction as Fr

import numpy as np

import postref


def _hand_case():
    """Three rows with spans 2, 3, 1 (prefix positions 0, 2, 5, 6), M = 2.  gamma is un-normalised on purpose; the normalised columns
    are (1/2, 1/2), (1/4, 3/4), (1/2, 1/2), (3/4, 1/4): quarters, exact in binary."""
    gamma = np.array([[3.0, 0.5, 5.0, 0.75],
                      [3.0, 1.5, 5.0, 0.25]])
    spans = np.array([2, 3, 1])
    return gamma, spans


def test_hand_worked_columns_and_summary():
    gamma, _ = _hand_case()
    p = postref.normalized(gamma)
    want = [[Fr(1, 2), Fr(1, 4), Fr(1, 2), Fr(3, 4)],
            [Fr(1, 2), Fr(3, 4), Fr(1, 2), Fr(1, 4)]]
    assert np.array_equal(p, np.array([[float(x) for x in r] for r in want]))
    s = postref.summary(gamma, weights=[1.0, 3.0], quantiles=(0.3, 0.5, 0.8))
    assert np.array_equal(s["colsum"], [6.0, 2.0, 10.0, 1.0])
    assert np.array_equal(s["argmax"], [0, 1, 0, 0])                      # ties: the first maximum
    # mean = 1 * p0 + 3 * p1
    assert np.array_equal(s["mean"], [float(Fr(1, 2) + 3 * Fr(1, 2)), float(Fr(1, 4) + 3 * Fr(3, 4)), 2.0, float(Fr(3, 4) + 3 * Fr(1, 4))])
    # F[0] = 1/2, 1/4, 1/2, 3/4; F[1] = 1
    assert np.array_equal(s["qstate"], [[0, 1, 0, 0],        # q = 0.3
                                        [0, 1, 0, 0],        # q = 0.5 (reached exactly at state 0 where F[0] = 1/2)
                                        [1, 1, 1, 1]])       # q = 0.8
    for k, q in enumerate((0.3, 0.5, 0.8)):
        assert postref.quantile_ok(gamma, s["qstate"][k], q, 0.0).all()
    assert not postref.quantile_ok(gamma, np.array([1, 1, 1, 1]), 0.3, 0.0).all()      # one state too late is rejected


def test_hand_worked_windows():
    """W = 4: window 0 = base pairs [0, 4) = row 1 (2 bp) + row 2 (2 bp); window 1 = [4, 6) = row 2 (1 bp) + row 3 (1 bp), 2 bp covered."""
    gamma, spans = _hand_case()
    want = np.array([[float((2 * Fr(1, 4) + 2 * Fr(1, 2)) / 4), float((Fr(1, 2) + Fr(3, 4)) / 2)],
                     [float((2 * Fr(3, 4) + 2 * Fr(1, 2)) / 4), float((Fr(1, 2) + Fr(1, 4)) / 2)]])
    assert want.tolist() == [[0.375, 0.625], [0.625, 0.375]]
    for f in (postref.windows_repeat, postref.windows_overlap_matrix):
        got = f(gamma, spans, 4)
        assert got.shape == (2, 2)
        assert np.array_equal(got, want), f.__name__
    # W = 1: one column per base pair; a window wider than the contig: the span-weighted average of the rows
    per_bp = postref.windows_repeat(gamma, spans, 1)
    assert np.array_equal(per_bp[0], [0.25, 0.25, 0.5, 0.5, 0.5, 0.75])
    wide = postref.windows_overlap_matrix(gamma, spans, 100)
    assert wide.shape == (2, 1) and wide[0, 0] == float((2 * Fr(1, 4) + 3 * Fr(1, 2) + Fr(3, 4)) / 6)
    # slabs smaller than a window: the parts of a straddling window are added up
    assert np.array_equal(postref.windows_repeat(gamma, spans, 4, slab_cells=6), want)


def test_random_case_two_formulations():
    rng = np.random.default_rng(7)
    M, L = 13, 400
    gamma = rng.random((M, L + 1)) * rng.integers(1, 50, L + 1)
    gamma[rng.random((M, L + 1)) < 0.1] = 0.0
    spans = rng.integers(1, 40, L)
    spans[5] = 700
    for W in (1, 7, 100, 1000, int(spans.sum()) + 5):
        a = postref.windows_repeat(gamma, spans, W, slab_cells=M * 1000)
        b = postref.windows_overlap_matrix(gamma, spans, W)
        assert a.shape == b.shape == (M, -(-int(spans.sum()) // W))
        tol = (W + 2 * M + 8) * postref.EPS
        assert np.all(np.abs(a - b) <= tol * np.abs(b)), W
        assert np.all(np.abs(a.sum(axis=0) - 1.0) <= tol), W
    # quantile states against a plain loop
    q = (0.025, 0.5, 0.975)
    s = postref.summary(gamma, weights=rng.random(M) + 0.1, quantiles=q)
    p = postref.normalized(gamma)
    for l in range(L + 1):
        run = 0.0
        loop = []
        for level in q:
            run, found = 0.0, M - 1
            for m in range(M):
                run += p[m, l]
                if run >= level:
                    found = m
                    break
            loop.append(found)
        assert list(s["qstate"][:, l]) == loop
    for k, level in enumerate(q):
        assert postref.quantile_ok(gamma, s["qstate"][k], level, 0.0).all()
