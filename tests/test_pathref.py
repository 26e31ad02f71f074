"""tests/pathref.py, the numpy oracle of the posterior path sampler, on the CPU: its Philox4x32-10 against the known answers of
include/smcpp_engine.h, its sampler against the float64 marginals and the expected number of state changes of a small fixed HMM
(M = 16, 401 positions, 4096 paths), and `draw_margins` - the measure the device is held to in tests/test_gpu_posterior_paths.py -
on the oracle's own paths (exactly 0) and on perturbed paths (non-zero at the perturbed draw and at the one before it).

Measured here: worst frequency deviation 0.30 of its bound, mean number of changes 0.69 standard errors off the expectation."""
import numpy as np
import pytest

import pathref
import transref

GAMMA_TOL = 2e-5                                            # (tests/test_gpu_parity.py; that module needs the engine)
SEED, CONTIG, K = 0x5EED0123456789AB, 3, 4096

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = pathref.philox4x32(ctr, key)
        assert tuple(int(x) for x in got) == want, ([hex(int(x)) for x in got], [hex(x) for x in want])
    w = pathref.philox4x32(KNOWN[0][0], KNOWN[0][1])
    assert float(pathref.words_to_uniform(w[0], w[1])) == 0.39904647231489565
    assert float(pathref.uniforms(0, 0, 0, 0)) == 0.39904647231489565
    # vectorised: the same words one by one; the high word of q and of the seed reach the counter and the key
    q = np.array([0, 1, 2 ** 32, 2 ** 40 + 7])
    u = pathref.uniforms(SEED, 2, 5, q)
    assert u.shape == (4,) and len(set(u.tolist())) == 4 and np.all((u >= 0) & (u < 1))
    for i, qq in enumerate(q.tolist()):
        w = pathref.philox4x32((qq & 0xffffffff, qq >> 32, 5, 2), (SEED & 0xffffffff, SEED >> 32))
        assert float(pathref.words_to_uniform(w[0], w[1])) == u[i]
    assert pathref.uniforms(SEED ^ (1 << 40), 2, 5, 0) != pathref.uniforms(SEED, 2, 5, 0)
    assert pathref.uniforms(SEED, 3, 5, 0) != pathref.uniforms(SEED, 2, 5, 0)
    assert pathref.uniforms(SEED, 2, 6, 0) != pathref.uniforms(SEED, 2, 5, 0)


@pytest.fixture(scope="module")
def hmm():
    rng = np.random.default_rng(20240611)
    M = 16
    pi = rng.random(M) + 0.1
    pi /= pi.sum()
    T = 0.92 * np.eye(M) + 0.08 * rng.dirichlet(np.ones(M), size=M)
    keys = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 2]])
    E = 0.05 + rng.random((3, M))
    spans = np.array([1, 64, 1, 1, 65, 7, 1, 128, 30, 1, 2, 99])
    obs = np.column_stack([spans, keys[rng.integers(0, 3, len(spans))]])
    assert spans.sum() == 400
    args = (pi, T, keys, E, obs)
    return {"args": args, "M": M, "spans": spans, "paths": pathref.sample(*args, SEED, CONTIG, K)}


def test_oracle_sampler_against_marginals_and_expected_changes(hmm):
    args, M, paths = hmm["args"], hmm["M"], hmm["paths"]
    assert paths.shape == (K, 401) and paths.dtype == np.int32 and paths.min() >= 0 and paths.max() < M
    g = pathref.marginals(*args)
    assert np.allclose(g.sum(axis=1), 1.0, atol=1e-12)
    f = pathref.state_frequencies(paths, M)
    ratio = np.abs(f - g) / pathref.frequency_bound(g, K, GAMMA_TOL)
    print(f"worst frequency deviation {ratio.max():.2f} of the bound")
    assert ratio.max() <= 1.0
    # the number of state changes per path against the expectation from the dense xi
    tr = transref.transitions(*args)
    want = tr[1:].sum()
    changes = (np.diff(paths, axis=1) != 0).sum(axis=1)
    se = changes.std(ddof=1) / np.sqrt(K)
    print(f"mean changes {changes.mean():.3f}, expected {want:.3f}, {abs(changes.mean() - want) / se:.2f} standard errors")
    assert se > 0 and abs(changes.mean() - want) <= 6 * se
    # rows_from_positions: the counts add up to the changes, the states are the positions'
    state, up, down = pathref.rows_from_positions(paths, hmm["spans"])
    assert state.shape == up.shape == down.shape == (K, len(hmm["spans"]) + 1) and state.dtype == up.dtype == down.dtype == np.int32
    assert np.array_equal(up.sum(axis=1) + down.sum(axis=1), changes)
    assert np.all(up[:, 0] == 0) and np.all(down[:, 0] == 0) and np.array_equal(state[:, 0], paths[:, 0])
    assert np.array_equal(state[:, -1], paths[:, -1]) and np.array_equal(state[:, 2], paths[:, 65])
    one = pathref.rows_from_positions(paths[7], hmm["spans"])
    assert all(np.array_equal(a, b[7]) for a, b in zip(one, (state, up, down)))
    assert np.array_equal(up[:, 2], (np.diff(paths[:, 0:66], axis=1)[:, 1:] > 0).sum(axis=1))   # row 2: positions 2 .. 65


def test_paths_do_not_depend_on_what_is_asked_for(hmm):
    args, paths = hmm["args"], hmm["paths"]
    assert np.array_equal(pathref.sample(*args, SEED, CONTIG, [5, 4000, 17]), paths[[5, 4000, 17]])
    assert not np.array_equal(pathref.sample(*args, SEED + 1, CONTIG, 4), paths[:4])
    assert not np.array_equal(pathref.sample(*args, SEED, CONTIG + 1, 4), paths[:4])


def test_draw_margins(hmm):
    args, paths = hmm["args"], hmm["paths"]
    m = pathref.draw_margins(*args, SEED, CONTIG, 0, paths[:64])
    assert m.shape == (64, 401) and np.all(m == 0.0)
    assert np.all(pathref.draw_margins(*args, SEED, CONTIG, 100, paths[100:104], cells=16 * 50) == 0.0)   # (blocks of 50 positions)
    # one state of one path changed: u is outside at that draw whatever the other state is (the intervals of the states are
    # disjoint), and at the draw before it (in time: position q - 1), which was conditioned on it - there for the other states that
    # move the conditional CDF past u, of which there is at least one; every other draw is untouched
    for q in (0, 1, 65, 66, 200, 399, 400):
        before = 0
        for other in range(1, hmm["M"]):
            bad = paths[:3].copy()
            bad[1, q] = (bad[1, q] + other) % hmm["M"]
            mb = pathref.draw_margins(*args, SEED, CONTIG, 0, bad)
            assert mb[1, q] > 0.0, (q, other)
            before += q > 0 and mb[1, q - 1] > 0.0
            mb[1, max(q - 1, 0):q + 1] = 0.0
            assert np.all(mb == 0.0), (q, other)
        assert q == 0 or before >= 1, q
        print(f"position {q}: the draw before it is off for {before} of {hmm['M'] - 1} other states")
    # the wrong path index, seed or contig: draws are off (not most of them: a sticky chain's "stay" interval holds most u)
    assert (pathref.draw_margins(*args, SEED, CONTIG, 1, paths[:2]) > 0).sum() >= 10
    assert (pathref.draw_margins(*args, SEED + 1, CONTIG, 0, paths[:2]) > 0).sum() >= 10
    assert (pathref.draw_margins(*args, SEED, CONTIG + 1, 0, paths[:2]) > 0).sum() >= 10
