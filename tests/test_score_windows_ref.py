"""The oracle of the score track's exact windows (tests/scorewin_ref.py) against itself and against the row oracle it is built on,
and the inputs of tests/test_gpu_score_windows_exact.py against the question they are there to answer.  No GPU.

Parameters: the host preparation of the synthetic model with one direction per piece (smcpp_host_prep_onepop_jac) at M = 8.

  1. a handful of rows with spans 1, 2, 64, 65, 200: the windows of every W sum (math.fsum) to the rows' sum; W >= N is the one-window
     total; W = 1 gives the per-position values; a row that no boundary cuts gives its window what the row oracle gives the row.
     Bars: the two sides add the same numbers in different orders - (terms + 8) 2^-52 of sum |term|, the window bar of
     tests/test_gpu_score_track.py.
  2. the inputs discriminate: on the un-binned input of the GPU test the row oracle APPORTIONED (scoreref.score_windows) and the
     exact windows differ by more than 10 GAMMA_TOL B_w in at least one window - otherwise a device that apportions would pass.
  3. both bindings declare smcpp_score_windows_exact (tests/test_host.py's staleness check covers the rest)."""
import math

import numpy as np
import pytest

import scoreref
import scorewin_ref
from test_gpu_parity import GAMMA_TOL

EPS = scoreref.EPS
M = 8
N_HAP = 8
SPANS = (1, 2, 64, 65, 200)
GAP_W = 100


def host_tables(keys, theta, rho):
    from smcpp_amd import _engine, synth
    a, s = synth.model_pieces()
    return _engine.host_prep_onepop_jac(N_HAP, synth.hidden_states(M), 0.5, a, np.eye(len(a)), s, theta, rho, 1.0, keys)


def unbinned_input():
    """Contig 0 of the GPU test's un-binned input (scorewin_ref.unbinned_input), the keys of all its contigs, theta and rho."""
    contigs, theta, rho = scorewin_ref.unbinned_input()
    keys = np.unique(np.vstack([c[:, 1:] for c in contigs]), axis=0).astype(np.int32)
    return contigs[0], keys, theta, rho


@pytest.fixture(scope="module")
def handful():
    import test_gpu_gamma as tg
    n = N_HAP
    obs = np.array([[1, 1, 2, n], [64, 0, 0, n], [2, 0, 1, n], [200, 0, 0, n], [1, 1, 0, n], [65, -1, 0, 0], [1, 0, 3, n], [2, 0, 0, n],
                    [200, 0, 0, n], [1, 1, 1, n]], dtype=np.int32)
    assert set(obs[:, 0]) == set(SPANS)
    keys = np.unique(obs[:, 1:], axis=0).astype(np.int32)
    tabs = host_tables(keys, tg.TH_U, tg.RH_U)
    rows = scoreref.score_rows(tabs[0], tabs[1], keys, tabs[2], tabs[3], tabs[4], tabs[5], obs)
    u, b = scorewin_ref.positions(tabs[0], tabs[1], keys, tabs[2], tabs[3], tabs[4], tabs[5], obs)
    return obs, keys, tabs, (rows[0] + rows[1]) + rows[2], u, b


def test_expand():
    obs = np.array([[3, 0, 0, 8], [1, 1, 2, 8], [2, -1, 0, 0]], dtype=np.int32)
    ex = scorewin_ref.expand(obs)
    assert ex.dtype == obs.dtype and ex.tolist() == [[1, 0, 0, 8]] * 3 + [[1, 1, 2, 8]] + [[1, -1, 0, 0]] * 2
    assert obs[0, 0] == 3                                                  # (the input is left alone)


def test_windows_sum_to_the_rows(handful):
    obs, keys, tabs, rows, u, b = handful
    N = int(obs[:, 0].sum())
    assert u.shape == b.shape == (rows.shape[0], N + 1) and np.all(b > 0.0)
    # the rows' sum contracts the SUM of a row's xi_p with G (M^2 signed terms), the positions contract every xi_p: both are within
    # (terms) 2^-52 of sum_p max |G|, the scale b
    mag = (M * M + 8) / (N + 8) * np.array([math.fsum(r) for r in b])
    want = np.array([math.fsum(r) for r in rows])
    for W in (1, 7, 64, 65, 100, N - 1, N, N + 5):
        got, B = scorewin_ref.exact_windows(*tabs[:2], keys, *tabs[2:], obs, W)
        assert got.shape == B.shape == (rows.shape[0], -(-N // W))
        sums = np.array([math.fsum(r) for r in got])
        # (the positions of a row against the row's own dense sum: the oracle's two groupings of the same xi_p)
        assert np.all(np.abs(sums - want) <= (N + 8) * EPS * mag), (W, np.max(np.abs(sums - want) / mag) / EPS)
        assert np.allclose(np.array([math.fsum(r) for r in B]), np.array([math.fsum(r) for r in b]), rtol=1e-13, atol=0)
        if W >= N:
            assert got.shape[1] == 1 and np.all(np.abs(got[:, 0] - want) <= (N + 8) * EPS * mag)
        if W == 1:
            first = u[:, 0] + u[:, 1]
            assert np.array_equal(got[:, 1:], u[:, 2:]) and np.all(np.abs(got[:, 0] - first) <= 4 * EPS * (np.abs(u[:, 0]) + np.abs(u[:, 1])))


def test_uncut_rows_are_the_row_oracles(handful):
    obs, keys, tabs, rows, u, b = handful
    P = np.concatenate([[0], np.cumsum(obs[:, 0])])
    for l in range(len(obs)):
        seg = u[:, 1 + P[l]:1 + P[l + 1]]
        got = np.array([math.fsum(r) for r in seg])
        mag = np.array([math.fsum(r) for r in b[:, 1 + P[l]:1 + P[l + 1]]])
        assert np.all(np.abs(got - rows[:, l + 1]) <= (obs[l, 0] + M * M + 8) * EPS * mag), l


def test_the_gpu_input_discriminates():
    obs, keys, theta, rho = unbinned_input()
    assert int(obs[:, 0].max()) > GAP_W                                   # rows that several boundaries cut
    tabs = host_tables(keys, theta, rho)
    rows = scoreref.score_rows(tabs[0], tabs[1], keys, tabs[2], tabs[3], tabs[4], tabs[5], obs)
    apportioned, _ = scoreref.score_windows((rows[0] + rows[1]) + rows[2], obs[:, 0], GAP_W)
    exact, B = scorewin_ref.exact_windows(tabs[0], tabs[1], keys, tabs[2], tabs[3], tabs[4], tabs[5], obs, GAP_W)
    ratio = np.abs(apportioned - exact) / (GAMMA_TOL * B)
    print(f"apportioned against exact windows at W = {GAP_W}: worst {ratio.max():.3g} of GAMMA_TOL B_w, "
          f"{int((ratio > 10.0).any(axis=0).sum())} of {ratio.shape[1]} windows beyond 10")
    assert ratio.max() > 10.0, ratio.max()


def test_bindings_declare_the_entry():
    from smcpp_amd import _cabi
    decl = {name: (ret, args) for name, ret, args in _cabi.declarations()}
    assert "smcpp_score_windows_exact" in decl
    ret, args = decl["smcpp_score_windows_exact"]
    assert ret == "int" and [t for t, _ in args] == [t for t, _ in decl["smcpp_score_windows"][1]]
    assert "smcpp_score_windows_exact(" in _cabi.pyx_extern_block() and _cabi.pyx_block_is_current()
    from smcpp_amd import _smcpp
    assert hasattr(_smcpp.PyOnePopInferenceManager, "score_windows_exact")
