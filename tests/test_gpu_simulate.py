"""The simulator - `im.simulate` / `smcpp_simulate` (smcpp_amd/csrc/simulate_dev.hpp) and smcpp_amd/simulate.py - on the device.

The truth is tests/simref.py: EVERY draw of every event of every replicate is held to the oracle's float64 CDF interval, widened only
by the tolerances its docstring derives from the arithmetic (TAU_CDF, TAU_G); no draw is exempt.  The shapes are the smallest at
which each part of the kernel can go wrong: M = 1 (no transitions), 2, 64 (a full wavefront), 65 (the first ragged second state per
lane), 150 (three per lane), 300 (eight per lane); alphabets of 14 keys (n = 4), 77 keys (n = 25: the second lane chunk) and 59
two-population keys; one `set_raw` manager with an unstructured T.  theta = 2.5e-2 and rho = 6e-3 per position, so that 5000 positions
hold hundreds of events.  Repetition, a split of the replicates into calls, every capacity (resumed runs), an E-step or a posterior
product in between and the Cython binding give the same bits; contig ends (N = 1, no event at all, a last event exactly on N) and a
wavefront's second unit of work are reached on purpose and asserted from `describe()`.  Frequencies of 4096 replicates are held to
pi T^p and (pi T^p) Ebar by Bernstein's bound at t = 30; the calibration test feeds simulated data back through a save_gamma E-step
under the generating parameters and holds sum_p (gamma_p(x_p) - sum_i gamma_p(i)^2), whose mean is zero for a correct generator AND a
correct posterior, to six of its own standard errors.

Measured on one MI355X (events in 8 replicates of 5000 positions / worst distance of a u from its CDF interval / quiet runs that are
not the floor of the oracle's own quotient):  M1 3706 / 0 / 0,  M2 3712 / 0 / 0,  M64 3648 / 0 / 0,  M65 3645 / 0 / 0,  M150 3646 / 0 / 0,
M300 3653 / 0 / 0,  M64:n25 6123 / 0 / 0,  twopop:M24 5432 / 0 / 0,  raw:M40 6008 / 0 / 0 (946 of them change the state; with the
model's T about 90 of 3650 do, and none at M = 2, whose first state is [0, 0.01)).  Frequencies: worst state / key deviation 0.02 /
0.39 of the bound at M = 2, 0.28 / 0.37 at M = 65.  Calibration: mean D = -1.13, standard error 1.30.  Every test below 2 s (the
bootstrap: two fits in 1.15 s, both calls 1.55 s)."""
import functools
import time
import types

import numpy as np
import pytest

import pathref
import simref

pytestmark = pytest.mark.gpu

SEED = 0x5EED51D0AB12CD34
THETA, RHO = 2.5e-2, 6e-3
CASES = ["M1", "M2", "M64", "M65", "M150", "M300", "M64:n25", "twopop:M24", "raw:M40"]


# ---------------------------------------------------------------------------------------------------------------------------------
# managers (one per case and module run; a simulation does not change them)
# ---------------------------------------------------------------------------------------------------------------------------------
def _onepop_model():
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    a, s = synth.model_pieces()
    return PiecewiseModel(a, s, 1e4, "pop1")


def _case(name, cython=False):
    from smcpp_amd import _engine, _smcpp, simulate, synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    parts = name.split(":")
    if parts[0] == "twopop":
        M = int(parts[1][1:])
        a, s = synth.model_pieces()
        model = TwoPopulationModel(PiecewiseModel(a, s, 1e4, pid="pop1"),
                                   PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(8)), s[:8], 1e4, pid="pop2"), 0.3)
        sim = simulate.Simulator(model, (4, 3), synth.hidden_states(M), THETA, RHO, a=(2, 0))
    elif parts[0] == "raw":
        # set_raw with a reversible T of no structure; pi and the emission table from the host preparation of the synthetic model
        M, n = int(parts[1][1:]), 4
        keys, q = simulate.full_alphabet(n)
        a, s = synth.model_pieces()
        hs = synth.hidden_states(M)
        pi, _, E = _engine.host_prep_onepop(n, hs, 0.5, a, s, THETA, RHO, 1.0, keys)
        rng = np.random.default_rng(M)
        S = rng.random((M, M)); S = S + S.T + 40.0 * M * np.eye(M)
        T = S / S.sum(axis=1, keepdims=True)
        listing = np.ascontiguousarray(np.hstack([np.ones((len(keys), 1), dtype=np.int32), keys]))
        im = _smcpp.PyOnePopInferenceManager(n, [listing], hs, ("pop1",), 0.5)
        im.theta = THETA; im.rho = RHO
        im.set_raw(pi, T, keys, E)
        lut = {tuple(int(x) for x in k): i for i, k in enumerate(im.keys)}
        alphabet = np.array([lut[tuple(int(x) for x in k)] for k in keys], dtype=np.int32)
        sim = types.SimpleNamespace(im=im, alphabet=alphabet, quiet=int(alphabet[q]), quiet_entry=q, key_rows=keys)
    else:
        M = int(parts[0][1:])
        n = int(parts[1][1:]) if len(parts) > 1 else 4
        sim = simulate.Simulator(_onepop_model(), n, synth.hidden_states(M), THETA, RHO, cython=cython)
    sim.im._simulate_call([1], sim.alphabet, sim.quiet, 0, 0, 0, 1, 1, None)              # (prepares the parameters)
    pi, T, E = sim.im._hmm_tables()
    sim.tb = simref.Tables(pi, T, E[sim.alphabet], sim.quiet_entry)
    return sim


case = functools.lru_cache(maxsize=None)(_case)


def draw(sim, lengths, R, seed=SEED, **kw):
    return sim.im.simulate(lengths, R, seed, sim.alphabet, sim.quiet, **kw)


def check_all(sim, lengths, ev, seed=SEED, first_replicate=0, first_contig=0, reps=None):
    """check_events on every (or the given) replicate of every contig; -> (events, worst CDF distance, worst run distance)."""
    n, wc, wg = 0, 0.0, 0.0
    for c, N in enumerate(np.atleast_1d(lengths)):
        for k in (range(len(ev["pos"][c])) if reps is None else reps):
            r = simref.check_events(sim.tb, None, None, None, int(N), seed, first_contig + c, first_replicate + k, ev["x0"][c, k],
                                    ev["pos"][c][k], ev["state"][c][k], ev["key"][c][k])
            n, wc, wg = n + r["events"], max(wc, r["worst_cdf"]), max(wg, r["worst_run"])
    return n, wc, wg


def same_bits(a, b, ra=None, rb=None):
    """The replicates ra of result a are the replicates rb of result b, bit for bit."""
    nc = len(a["pos"])
    assert len(b["pos"]) == nc
    ra = list(range(len(a["pos"][0]))) if ra is None else list(ra)
    rb = list(range(len(b["pos"][0]))) if rb is None else list(rb)
    assert len(ra) == len(rb)
    for c in range(nc):
        for i, j in zip(ra, rb):
            assert a["x0"][c, i] == b["x0"][c, j], (c, i, j)
            for f in ("pos", "state", "key"):
                assert a[f][c][i].dtype == b[f][c][j].dtype and np.array_equal(a[f][c][i], b[f][c][j]), (f, c, i, j)


# ---------------------------------------------------------------------------------------------------------------------------------
# every draw
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_every_draw_against_the_oracle(name):
    """8 replicates of 5000 positions: every quiet run, successor state and key of every event inside the oracle's interval."""
    sim = case(name)
    N, R = 5000, 8
    t0 = time.time()
    ev = draw(sim, [N], R)
    t1 = time.time()
    assert ev["x0"].shape == (1, R) and ev["x0"].dtype == np.int32
    assert ev["pos"][0][0].dtype == np.int64 and ev["state"][0][0].dtype == np.int32 and ev["key"][0][0].dtype == np.int32
    n, wc, wg = check_all(sim, [N], ev)
    stays = sum(int((np.concatenate([[ev["x0"][0, k]], ev["state"][0][k][:-1]]) == ev["state"][0][k]).sum()) for k in range(R))
    print(f"{name}: M = {sim.tb.M}, |A| = {sim.tb.A}: {n} events in {R} replicates of {N} positions ({stays} keep the state), "
          f"{ev['calls']} device calls in {t1 - t0:.3f} s; worst CDF distance {wc:.2e} (bar {simref.tau_cdf(sim.tb.M, sim.tb.A):.2e}), "
          f"worst run distance {wg:.2e}; describe: {({k: v for k, v in sim.im.describe().items() if k.startswith('simulate')})}")
    assert n > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["M65", "M64:n25"])
def test_same_bits_across_calls_splits_and_capacities(name):
    sim = case(name)
    L = [1500, 1500, 700]
    full = draw(sim, L, 8)
    same_bits(full, draw(sim, L, 8))                                       # a repeated call
    same_bits(full, draw(sim, L, 3), range(3))                             # replicates [0, 8) = [0, 3) + [3, 8)
    same_bits(full, draw(sim, L, 5, first_replicate=3), range(3, 8))
    for cap in (1, 7, 4000):                                               # resumed runs: every capacity gives the bits of an uncapped one
        r = draw(sim, L[2:], 2, first_contig=2, cap=cap)
        one = {k: (full[k][2:] if k != "calls" else 0) for k in full}
        same_bits(one, r, range(2))
        assert (r["calls"] == 1) == (cap == 4000), (cap, r["calls"])
    # two contigs of equal length in one call get different draws
    assert not np.array_equal(full["pos"][0][0], full["pos"][1][0])
    # ... and a contig is named by first_contig + its index, whatever call it is in
    same_bits({k: (full[k][1:2] if k != "calls" else 0) for k in full}, draw(sim, L[1:2], 8, first_contig=1))


def test_same_bits_around_an_estep_and_a_posterior_product():
    sim = case("M64")
    L = [2000]
    before = draw(sim, L, 4)
    sim.im.save_gamma = True
    sim.im.E_step()
    ll = sim.im.loglik()
    same_bits(before, draw(sim, L, 4))
    cols = sim.im.posterior_columns(0)
    paths = sim.im.posterior_sample_positions(0, 4, SEED)
    same_bits(before, draw(sim, L, 4))
    # ... and the simulation disturbs neither: the products of the stored E-step are what they were, a fresh E-step gives the same
    assert np.array_equal(cols, sim.im.posterior_columns(0))
    assert np.array_equal(paths, sim.im.posterior_sample_positions(0, 4, SEED))
    sim.im.E_step()
    assert sim.im.loglik() == ll
    # a seed shared with the path sampler does not share its uniforms
    assert simref.uniforms(SEED, 0, 0, 0, 0) != pathref.uniforms(SEED, 0, 0, 0)


def test_the_cython_manager_gives_the_same_bits():
    a, b = case("M65"), _case("M65", cython=True)
    assert type(a.im).__module__.endswith("_smcpp") and type(b.im).__module__.endswith("_smcpp_cy")
    L = [1200, 300]
    same_bits(draw(a, L, 4), draw(b, L, 4))
    same_bits(draw(a, L, 4), draw(b, L, 4, cap=5))


# ---------------------------------------------------------------------------------------------------------------------------------
# ends
# ---------------------------------------------------------------------------------------------------------------------------------
def test_contig_ends():
    sim = case("M64")
    # N = 1
    ev = draw(sim, [1], 64)
    n1, _, _ = check_all(sim, [1], ev)
    assert all(len(p) <= 1 for p in ev["pos"][0]) and all(np.all(p == 1) for p in ev["pos"][0])
    # N shorter than the first quiet run: no event at all (found with the oracle's sampler)
    N = 5
    ref = simref.sample(sim.tb, None, None, None, N, SEED, 0, 16)
    empty = [k for k, r in enumerate(ref) if len(r[1]) == 0]
    assert len(empty) >= 4
    ev = draw(sim, [N], 16)
    check_all(sim, [N], ev)
    assert all(len(ev["pos"][0][k]) == 0 for k in empty)
    assert all(ev["x0"][0, k] == ref[k][0] for k in range(16))
    # a last event exactly on N: N = the position of the third event of the oracle's replicate 0 of a longer contig
    long_ = simref.sample(sim.tb, None, None, None, 2000, SEED, 0, 1)[0]
    N = int(long_[1][2])
    ev = draw(sim, [N], 1)
    check_all(sim, [N], ev)
    assert len(ev["pos"][0][0]) == 3 and ev["pos"][0][0][-1] == N
    assert np.array_equal(ev["pos"][0][0], long_[1][:3]) and np.array_equal(ev["state"][0][0], long_[2][:3])
    assert np.array_equal(ev["key"][0][0], long_[3][:3])
    print(f"N = 1: {n1} events in 64 replicates; N = 5: {len(empty)} of 16 replicates without an event; a last event on N = {N}")


def test_a_wavefronts_second_unit_of_work():
    """2 contigs x 2100 replicates = 4200 (contig, replicate) pairs on 4096 wavefronts: the pairs 4096 .. 4199 are second units.
    They are held to the oracle and are, bit for bit, what calls of at most 64 replicates give, in which no wavefront takes two."""
    sim = case("M64")
    L, R = [64, 64], 2100
    ev = draw(sim, L, R, cap=64)
    d = sim.im.describe()
    assert d["simulate_units"] == 4200 and d["simulate_waves"] == 4096, d
    second = range(4096 - R, R)                                            # replicates of contig 1 on a wavefront's second unit
    tail = {k: (ev[k][1:] if k != "calls" else 0) for k in ev}
    n, wc, wg = check_all(sim, L[1:], tail, first_contig=1, reps=list(second)[:48] + list(second)[-16:])
    n0, _, _ = check_all(sim, L[:1], ev, reps=range(32))
    small = draw(sim, L[1:], 64, first_contig=1, first_replicate=R - 64, cap=64)
    assert sim.im.describe()["simulate_units"] == sim.im.describe()["simulate_waves"] == 64
    same_bits(tail, small, range(R - 64, R), range(64))
    print(f"second units: {n} events held in 64 replicates (first units: {n0} in 32), worst CDF distance {wc:.2e}")
    assert n > 0 and n0 > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# frequencies
# ---------------------------------------------------------------------------------------------------------------------------------
def test_frequencies_against_the_marginals():
    """4096 replicates of 64 positions at M = 2 and M = 65: the state frequencies at every position against pi T^p, the key
    frequencies against (pi T^p) Ebar, by Bernstein's bound at t = 30 (2e-13 per cell for an exact sampler)."""
    for name in ("M2", "M65"):
        sim = case(name)
        N, R = 64, 4096
        ev = draw(sim, [N], R)
        XO = [simref.expand(N, sim.quiet_entry, ev["x0"][0, k], ev["pos"][0][k], ev["state"][0][k], ev["key"][0][k]) for k in range(R)]
        X, O = np.array([x for x, _ in XO]), np.array([o for _, o in XO])
        S, Kd = simref.marginals(sim.tb.pi, sim.tb.T, sim.tb.EA, N)
        ds = np.abs(simref.frequencies(X, sim.tb.M) - S) / pathref.frequency_bound(S, R, 0.0)
        dk = np.abs(simref.frequencies(O[:, 1:], sim.tb.A) - Kd[1:]) / pathref.frequency_bound(Kd[1:], R, 0.0)
        print(f"{name}: worst state deviation {ds.max():.2f} of the bound, worst key deviation {dk.max():.2f} of the bound")
        assert ds.max() <= 1.0, name
        assert dk.max() <= 1.0, name


# ---------------------------------------------------------------------------------------------------------------------------------
# calibration against the E-step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_calibration_against_the_estep():
    """256 replicates of 500 positions at M = 64 through `events_to_rows` into ONE manager, a save_gamma E-step under the generating
    parameters: D_r = sum_p (gamma_p(x_p) - sum_i gamma_p(i)^2) over the positions 0 .. N with the simulated path x has mean zero."""
    from smcpp_amd import _smcpp, simulate, synth
    sim = case("M64")
    N, R, M = 500, 256, 64
    ev = draw(sim, [N], R)
    rows = [simulate.events_to_rows(N, ev["pos"][0][k], ev["key"][0][k], sim.key_rows, sim.quiet_entry) for k in range(R)]
    paths = [simulate.segments_to_path(simulate.events_to_segments(N, ev["x0"][0, k], ev["pos"][0][k], ev["state"][0][k])) for k in range(R)]
    assert all(int(r[:, 0].sum()) == N for r in rows) and all(len(p) == N + 1 for p in paths)
    im = _smcpp.PyOnePopInferenceManager(4, rows, synth.hidden_states(M), ("pop1",), 0.5)
    im.model = _onepop_model()
    im.theta = THETA; im.rho = RHO; im.alpha = 1.0
    im.save_gamma = True
    im.E_step()
    D = np.empty(R)
    at = np.arange(N + 1)
    for k in range(R):
        g = im.posterior_positions(k)
        assert g.shape == (M, N + 1)
        D[k] = float((g[paths[k], at] - (g * g).sum(axis=0)).sum())
    se = D.std(ddof=1) / np.sqrt(R)
    print(f"calibration: mean D = {D.mean():.4f}, standard error {se:.4f} ({D.mean() / se:+.2f} s.e.), sd of D {D.std(ddof=1):.3f}")
    assert se > 0 and abs(D.mean()) <= 6.0 * se


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_manager_usable():
    from smcpp_amd import _smcpp, simulate, synth
    sim = case("M65")
    ok = draw(sim, [300], 2)
    A, q = sim.alphabet, sim.quiet
    call = sim.im.simulate
    K = len(sim.im.keys)
    bad = [
        (lambda: call([0], 1, SEED, A, q), "N < 1"),
        (lambda: call([300, -5], 1, SEED, A, q), "N < 1"),
        (lambda: call([300], 0, SEED, A, q), "n_replicates < 1"),
        (lambda: call([300], 1, SEED, A, q, cap=0), "cap < 1"),
        (lambda: call([300], 1, SEED, list(A[:-1]) + [K], q), "out of range"),
        (lambda: call([300], 1, SEED, list(A[:-1]) + [-1], q), "out of range"),
        (lambda: call([300], 1, SEED, list(A) + [int(A[3])], q), "given twice"),
        (lambda: call([300], 1, SEED, [k for k in A if k != q], q), "not in the alphabet"),
        (lambda: call([300], 2, SEED, A, q, first_replicate=2 ** 31 - 1), r"2\^31"),
        (lambda: call([300], 1, SEED, A, q, first_replicate=-1), "first_replicate < 0"),
        (lambda: call([300], 2 ** 20, SEED, A, q, cap=2 ** 12), "exceed the cap of 2.31 - 1 elements"),
    ]
    for f, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            f()
        same_bits(ok, draw(sim, [300], 2))
    # parameters not set
    keys, _ = simulate.full_alphabet(4)
    listing = np.ascontiguousarray(np.hstack([np.ones((len(keys), 1), dtype=np.int32), keys]))
    im = _smcpp.PyOnePopInferenceManager(4, [listing], synth.hidden_states(8), ("pop1",), 0.5)
    with pytest.raises(RuntimeError, match="parameters are not set"):
        im.simulate([100], 1, SEED, quiet=0)
    # a state whose alphabet mass is 0
    pi, T, E = sim.im._hmm_tables()
    M = len(pi)
    im2 = _smcpp.PyOnePopInferenceManager(4, [listing], synth.hidden_states(M), ("pop1",), 0.5)
    E0 = E.copy(); E0[:, 7] = 0.0
    im2.set_raw(pi, T, im2.keys, E0)
    with pytest.raises(RuntimeError, match="state 7 gives the alphabet no mass"):
        im2.simulate([100], 1, SEED, quiet=0)
    im2.set_raw(pi, T, im2.keys, E)                                         # the manager still works afterwards
    same_bits(ok, im2.simulate([300], 2, SEED, sim.alphabet, sim.quiet))
    im.model = _onepop_model()
    im.theta = THETA; im.rho = RHO
    assert len(im.simulate([300], 1, SEED, quiet=0)["pos"][0][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# bootstrap plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_parametric_bootstrap_plumbing():
    """B = 2 data sets from a tiny fitted model, one EM iteration each: two models, the same seed gives the same models, the band
    of N(t) has the right shape."""
    from smcpp_amd import simulate, synth
    from smcpp_amd.analysis import EstimateArgs, SMCModel
    m = SMCModel([0.05, 0.3, 2.0], 4000.0, "pop1")
    m[:] = np.log([0.6, 1.5, 1.0])
    final = {"theta": 1e-4, "rho": 1e-4, "alpha": 100, "model": m.to_dict(),
             "hidden_states": {"pop1": [float(x) for x in synth.hidden_states(8)]}}
    args = EstimateArgs(knots=4, em_iterations=1, multi=True, r=1.25e-8)
    t0 = time.time()
    a = simulate.parametric_bootstrap(final, 4, [150_000, 120_000], 2, seed=11, estimate_args=args)
    t1 = time.time()
    b = simulate.parametric_bootstrap(final, 4, [150_000, 120_000], 2, seed=11, estimate_args=args)
    assert len(a) == 2 and len(b) == 2
    for x, y in zip(a, b):
        assert np.array_equal(x.knots, y.knots) and np.array_equal(x[:], y[:])
    assert not np.array_equal(a[0][:], a[1][:])
    t = np.logspace(1, 5, 9)
    band = simulate.size_history_band(a, t, (0.025, 0.5, 0.975))
    assert band.shape == (3, 9) and np.all(np.isfinite(band)) and np.all(band > 0) and np.all(np.diff(band, axis=0) >= 0)
    print(f"bootstrap: two fits in {t1 - t0:.2f} s; median N(t) {band[1].round(0).tolist()}")
