"""tests/llref.py, the float64 reference of the log-likelihood track, pinned on the CPU: against the enumeration of every path of a
small model, against oracle/oracle.py's restatement of the reference (per-row log_c and loglik) on the goldens G1, G2 (long spans)
and G4 - the differences found there are the reference's own float noise, printed and quoted in llref's docstring -, and
smcpp_amd.evidence.compare_tracks / surprisal on hand-made tracks with the jackknife in closed form.

Bounds against the oracle.  The oracle (like the reference) carries alpha as FLOAT from row to row, so the vector a row starts
from is off by up to 2^-24 relative per entry (more on entries at the 1e-10 floor, which hold no mass worth speaking of).  A
perturbation d of the start vector moves the row's log c by at most |d|_1 times the spread of the row's log-evidence over the start
states, which log c itself bounds for a row of many positions and 1 bounds for a short one: FLOAT_EPS (1 + |log c_l|) per row with
a factor 64 for the rows in front whose perturbations have not yet been forgotten, and the same per unit of |loglik| for the total."""
import itertools

import numpy as np
import pytest

import llref
from conftest import load_golden

FLOAT_EPS = 2.0 ** -24
WIDTHS = (100, 10_000)


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


def test_every_path_of_a_small_model():
    """l(p) = log of the summed weight of every path x_0 .. x_p."""
    pi, T, keys, E = small_hmm(3, 3, 1)
    spans, kids = [1, 3, 2], [0, 2, 1]
    obs = rows_of(spans, kids, keys)
    kid_of_pos = np.repeat(kids, spans)
    N = len(kid_of_pos)
    want = np.zeros(N + 1)
    for p in range(1, N + 1):
        tot = 0.0
        for path in itertools.product(range(3), repeat=p + 1):
            w = pi[path[0]]
            for t in range(1, p + 1):
                w *= T[path[t - 1], path[t]] * E[kid_of_pos[t - 1], path[t]]
            tot += w
        want[p] = np.log(tot)
    ell = llref.track(pi, T, keys, E, obs)
    assert ell.shape == (N + 1,) and ell[0] == 0.0
    assert np.max(np.abs(ell - want)) <= 16 * N * llref.EPS * np.abs(want).max()
    # rows, grids and windows are read off l
    r = llref.rows(ell, obs)
    assert r[0] == 0.0 and np.array_equal(r[1:], [ell[1], ell[4] - ell[1], ell[6] - ell[4]])
    for pos0, pos1, step in ((0, 7, 1), (0, 7, 2), (1, 7, 3), (2, 5, 1), (6, 7, 1)):
        assert np.array_equal(llref.grid(ell, pos0, pos1, step), ell[pos0:pos1:step])
    assert np.array_equal(llref.windows(ell, 1), np.diff(ell))
    assert np.array_equal(llref.windows(ell, 4), [ell[4], ell[6] - ell[4]])
    for W in (6, 7, 100):
        assert np.array_equal(llref.windows(ell, W), [ell[6]])
    # a split in l's own proportions with l's own row values gives l back
    back = llref.split_rows(ell, obs, r)
    assert np.max(np.abs(back - ell)) <= 8 * llref.EPS * np.abs(ell).max()


@pytest.mark.parametrize("name", ["G1_M16_n4", "G2_M51_n6_longspans", "G4_M64_n20_2Mbp"])
def test_rows_and_total_against_the_oracle(name):
    g = load_golden(name)
    obs = np.ascontiguousarray(g["obs"], dtype=np.int32)
    ell, d_row, d_win, d_tot = llref.noise(g["pi"], g["T"], g["keys"], g["E"], obs, WIDTHS)
    print(f"{name}: NOISE d_row {d_row:.2e} " + " ".join(f"d_win({W}) {d_win[W]:.2e}" for W in WIDTHS) + f" total rel {d_tot:.2e}")
    from oracle import oracle
    o = oracle.estep(g["pi"], g["T"], g["keys"], g["E"], obs)
    r = llref.rows(ell, obs)
    assert r.shape == o["log_c"].shape
    bar = 64 * FLOAT_EPS * (1.0 + np.abs(o["log_c"][1:]))
    miss = np.abs(r[1:] - o["log_c"][1:]) / bar
    assert miss.max() <= 1.0, f"{name}: row {int(miss.argmax()) + 1} off by {miss.max():.2f} of its bar"
    assert d_tot <= 64 * FLOAT_EPS, (name, d_tot)
    # the golden's own recorded values (the compiled reference) say the same
    assert abs(ell[-1] - float(g["loglik"])) <= 64 * FLOAT_EPS * abs(float(g["loglik"]))
    # windows are differences of l: they add up to the total, and one window is the total
    for W in WIDTHS:
        w = llref.windows(ell, W)
        assert len(w) == -(-(len(ell) - 1) // W)
        assert abs(w.sum() - ell[-1]) <= len(w) * llref.EPS * np.abs(w).sum()
    assert llref.windows(ell, len(ell) + 5)[0] == ell[-1]


# ---- smcpp_amd.evidence on hand-made tracks ----
def test_compare_tracks_closed_form():
    from smcpp_amd.evidence import compare_tracks
    a = [np.array([-1.0, -2.0, -3.0, -4.0]), np.array([-5.0, -6.0])]
    b = [np.array([-1.5, -1.0, -3.0, -6.0]), np.array([-4.0, -6.5])]
    r = compare_tracks(a, b)                              # d = .5, -1, 0, 2, -1, .5: D = 1, mean 1/6
    d = np.array([0.5, -1.0, 0.0, 2.0, -1.0, 0.5])
    assert np.array_equal(r["blocks"], d) and r["delta"] == 1.0
    se = np.sqrt(6.0 / 5.0 * np.sum((d - 1.0 / 6.0) ** 2))
    assert abs(r["se"] - se) <= 4 * llref.EPS * se and abs(r["z"] - 1.0 / se) <= 8 * llref.EPS / se
    # the delete-one-block jackknife of a sum, literally: theta_(b) = (B / (B - 1)) (D - d_b) estimates D without block b
    B = len(d)
    th = B / (B - 1.0) * (d.sum() - d)
    lit = np.sqrt((B - 1.0) / B * np.sum((th - th.mean()) ** 2))
    assert abs(r["se"] - lit) <= 16 * llref.EPS * lit
    # blocks of two windows never straddle contigs; the last block of a contig may be short
    r2 = compare_tracks(a, b, block=2)
    assert np.array_equal(r2["blocks"], [-0.5, 2.0, -0.5]) and r2["delta"] == 1.0
    assert abs(r2["se"] - np.sqrt(3.0 / 2.0 * np.sum((r2["blocks"] - 1.0 / 3.0) ** 2))) <= 4 * llref.EPS * r2["se"]
    r3 = compare_tracks(a, b, block=3)
    assert np.array_equal(r3["blocks"], [-0.5, 2.0, -0.5])
    # identical tracks: no difference, no spread
    same = compare_tracks(a, a)
    assert same["delta"] == 0.0 and same["se"] == 0.0 and same["z"] == 0.0


def test_compare_tracks_refusals():
    from smcpp_amd.evidence import compare_tracks
    a = [np.array([-1.0, -2.0, -3.0])]
    with pytest.raises(ValueError, match="at least two"):
        compare_tracks(a, a, block=3)
    with pytest.raises(ValueError, match="at least two"):
        compare_tracks([np.array([-1.0])], [np.array([-2.0])])
    with pytest.raises(ValueError, match="shapes"):
        compare_tracks(a, [np.array([-1.0, -2.0])])
    with pytest.raises(ValueError, match="contigs"):
        compare_tracks(a, a + a)
    with pytest.raises(ValueError, match="block < 1"):
        compare_tracks(a, a, block=0)


def test_surprisal_divides_the_last_window_by_its_true_width():
    from smcpp_amd.evidence import surprisal
    s = surprisal([np.array([-10.0, -20.0, -3.0]), np.array([-4.0])], 10, [23, 8])
    assert np.array_equal(s[0], [1.0, 2.0, 1.0]) and np.array_equal(s[1], [0.5])
    full = surprisal([np.array([-10.0, -20.0])], 10, [20])
    assert np.array_equal(full[0], [1.0, 2.0])
    with pytest.raises(ValueError, match="do not cover"):
        surprisal([np.array([-1.0, -2.0])], 10, [25])
