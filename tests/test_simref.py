"""The simulator's oracle (tests/simref.py) and the host side of smcpp_amd/simulate.py, without a device: `check_events` accepts the
oracle's own event-driven sampler and rejects tampered event lists; the event-driven sampler and the naive position-by-position walk
agree in distribution; the alphabet of `full_alphabet` carries all of the emission mass but the 1e-10 floors; `events_to_rows` and
`events_to_segments` on hand-written event lists.  The model is the synthetic one, prepared on the host (smcpp_host_prep_onepop)."""
import numpy as np
import pytest

import pathref
import simref

SEED = 0x51D0C0FFEE123457
THETA, RHO = 2.5e-2, 6e-3


def host_model(M=8, n=4):
    from smcpp_amd import _engine, simulate, synth
    keys, q = simulate.full_alphabet(n)
    a, s = synth.model_pieces()
    pi, T, E = _engine.host_prep_onepop(n, synth.hidden_states(M), 0.5, a, s, THETA, RHO, 1.0, keys)
    return pi, T, E, q, keys


@pytest.fixture(scope="module")
def model():
    return host_model()


@pytest.fixture(scope="module")
def sampled(model):
    pi, T, E, q, _ = model
    N = 3000
    return N, simref.sample(pi, T, E, q, N, SEED, 3, 12)


def test_check_events_accepts_the_oracles_sampler(model, sampled):
    pi, T, E, q, _ = model
    N, reps = sampled
    total = 0
    for k, (x0, pos, st, key) in enumerate(reps):
        r = simref.check_events(pi, T, E, q, N, SEED, 3, k, x0, pos, st, key)
        assert r["worst_cdf"] == 0.0 and r["worst_run"] == 0.0, r
        total += r["events"]
    print(f"{total} events in {len(reps)} replicates of {N} positions")
    assert total > 100 * len(reps) // 2
    stay = sum(int((np.concatenate([[x0], st[:-1]]) == st).sum()) for x0, _, st, _ in reps)
    quiet_moves = sum(int((key == q).sum()) for _, _, _, key in reps)
    assert stay > 0 and quiet_moves > 0                                    # both kinds of loud position occur


def _pick(reps, cond):
    for k, (x0, pos, st, key) in enumerate(reps):
        prev = np.concatenate([[x0], st[:-1]])
        for e in range(len(pos)):
            if cond(prev, pos, st, key, e):
                return k, e
    raise AssertionError("no such event in the sample")


def test_check_events_rejects_a_shifted_position(model, sampled):
    pi, T, E, q, _ = model
    N, reps = sampled
    k, e = _pick(reps, lambda prev, pos, st, key, e: 0 < e < len(pos) - 1 and pos[e + 1] - pos[e] > 1)
    x0, pos, st, key = reps[k]
    pos = pos.copy(); pos[e] += 1
    with pytest.raises(AssertionError, match="quiet run"):
        simref.check_events(pi, T, E, q, N, SEED, 3, k, x0, pos, st, key)


def test_check_events_rejects_a_swapped_state(model, sampled):
    pi, T, E, q, _ = model
    N, reps = sampled
    k, e = _pick(reps, lambda prev, pos, st, key, e: e > 0)
    x0, pos, st, key = reps[k]
    st = st.copy(); st[e] = (st[e] + 1) % len(pi)
    with pytest.raises(AssertionError):
        simref.check_events(pi, T, E, q, N, SEED, 3, k, x0, pos, st, key)


def test_check_events_rejects_the_quiet_key_on_a_stay_event(model, sampled):
    pi, T, E, q, _ = model
    N, reps = sampled
    k, e = _pick(reps, lambda prev, pos, st, key, e: prev[e] == st[e])
    x0, pos, st, key = reps[k]
    assert key[e] != q
    key = key.copy(); key[e] = q
    with pytest.raises(AssertionError, match="key"):
        simref.check_events(pi, T, E, q, N, SEED, 3, k, x0, pos, st, key)


def test_check_events_rejects_an_event_past_N(model, sampled):
    pi, T, E, q, _ = model
    N, reps = sampled
    x0, pos, st, key = reps[0]
    with pytest.raises(AssertionError, match="past N"):
        simref.check_events(pi, T, E, q, N, SEED, 3, 0, x0, np.append(pos, N + 1), np.append(st, st[-1]), np.append(key, 1))
    # ... and a list cut short misses a loud position
    with pytest.raises(AssertionError, match="missing"):
        simref.check_events(pi, T, E, q, N, SEED, 3, 0, x0, pos[:-1], st[:-1], key[:-1])


def test_the_two_samplers_agree_in_distribution(model):
    """4096 replicates of 24 positions: the per-position state and key frequencies of the event-driven sampler and of the naive
    walk both lie within Bernstein's bound at t = 30 (2e-13 per cell for an exact sampler) of pi T^p and (pi T^p) Ebar, and so
    within the sum of the two bounds of each other."""
    pi, T, E, q, _ = model
    N, R = 24, 4096
    S, Kd = simref.marginals(pi, T, E, N)
    reps = simref.sample(pi, T, E, q, N, SEED, 0, R)
    XO = [simref.expand(N, q, *r) for r in reps]
    Xe, Oe = np.array([x for x, _ in XO]), np.array([o for _, o in XO])
    Xn, On = simref.sample_positionwise(pi, T, E, N, np.random.default_rng(7), R)
    bs, bk = pathref.frequency_bound(S, R, 0.0), pathref.frequency_bound(Kd[1:], R, 0.0)
    for name, X, O in (("events", Xe, Oe), ("positions", Xn, On)):
        ds = np.abs(simref.frequencies(X, len(pi)) - S) / bs
        dk = np.abs(simref.frequencies(O[:, 1:], len(E)) - Kd[1:]) / bk
        print(f"{name}: worst state deviation {ds.max():.2f} of the bound, worst key deviation {dk.max():.2f}")
        assert ds.max() <= 1.0 and dk.max() <= 1.0, name
    assert np.all(np.abs(simref.frequencies(Xe, len(pi)) - simref.frequencies(Xn, len(pi))) <= 2 * bs)
    assert np.all(np.abs(simref.frequencies(Oe[:, 1:], len(E)) - simref.frequencies(On[:, 1:], len(E))) <= 2 * bk)


@pytest.mark.parametrize("n", [4, 25])
def test_alphabet_mass(n):
    """sum_{k in A} E[k][m] = 1 up to the 1e-10 floors of incorporate_theta (|A| of them at most) and the rounding of |A| terms."""
    pi, T, E, q, keys = host_model(M=16, n=n)
    assert len(keys) == 3 * (n + 1) - 1 and tuple(keys[q]) == (0, 0, n) and not any(tuple(k) == (2, n, n) for k in keys)
    dev = np.abs(E.sum(axis=0) - 1.0)
    print(f"n = {n}: {len(keys)} keys, worst |mass - 1| = {dev.max():.3e}")
    assert dev.max() <= len(keys) * 1e-10 + len(keys) * 2.0 ** -52


def test_full_alphabet_twopop():
    from smcpp_amd import simulate
    keys, q = simulate.full_alphabet_twopop(3, 2, 2, 0)
    assert len(keys) == 3 * 4 * 1 * 3 - 1 and tuple(keys[q]) == (0, 0, 3, 0, 0, 2)
    assert [tuple(k) for k in keys] == sorted(tuple(k) for k in keys) and (2, 3, 3, 0, 2, 2) not in [tuple(k) for k in keys]
    keys, q = simulate.full_alphabet_twopop(2, 2, 1, 1)
    assert len(keys) == 2 * 3 * 2 * 3 - 1 and (1, 2, 2, 1, 2, 2) not in [tuple(k) for k in keys]


def test_events_to_rows_and_segments():
    from smcpp_amd import simulate
    keys, q = simulate.full_alphabet(4)
    het, der = 6, 2                                                        # (1, 1, 4) and (0, 2, 4)
    assert tuple(keys[het]) == (1, 1, 4) and tuple(keys[der]) == (0, 2, 4)
    Q = [0, 0, 4]
    # a contig with no event
    assert simulate.events_to_rows(10, [], [], keys, q).tolist() == [[10] + Q]
    assert simulate.events_to_segments(10, 3, [], []).tolist() == [[3, 0, 10]]
    # an event at position N, one at position 1
    assert simulate.events_to_rows(10, [1, 10], [het, der], keys, q).tolist() == [[1, 1, 1, 4], [8] + Q, [1, 0, 2, 4]]
    assert simulate.events_to_segments(10, 3, [1, 10], [3, 5]).tolist() == [[3, 0, 9], [5, 10, 10]]
    # a state change that emits the quiet key leaves no row, but a segment
    assert simulate.events_to_rows(10, [4, 7], [q, het], keys, q).tolist() == [[6] + Q, [1, 1, 1, 4], [3] + Q]
    assert simulate.events_to_segments(10, 0, [4, 7], [2, 2]).tolist() == [[0, 0, 3], [2, 4, 10]]
    # two equal loud rows in a row are merged; different ones are not
    assert simulate.events_to_rows(10, [4, 5, 6], [het, het, der], keys, q).tolist() == [[3] + Q, [2, 1, 1, 4], [1, 0, 2, 4], [4] + Q]
    seg = simulate.events_to_segments(10, 1, [4, 5, 6], [0, 0, 1])
    assert seg.tolist() == [[1, 0, 3], [0, 4, 5], [1, 6, 10]]
    assert simulate.segments_to_path(seg).tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1]
    rows = simulate.events_to_rows(10, [4, 5, 6], [het, het, der], keys, q)
    assert rows.dtype == np.int32 and int(rows[:, 0].sum()) == 10


def test_size_history_band():
    from smcpp_amd import simulate
    from smcpp_amd.analysis import SMCModel
    ms = []
    for y in (0.0, 1.0, 2.0):
        m = SMCModel([0.1, 1.0, 10.0], 1e4, "pop1")
        m[:] = y
        ms.append(m)
    band = simulate.size_history_band(ms, [100.0, 1e4, 1e6], (0.0, 0.5, 1.0))
    assert band.shape == (3, 3)
    assert np.allclose(band[:, 0], 1e4 * np.exp([0.0, 1.0, 2.0]))


class _MockManager:
    """`_simulate_call` / `_hmm_tables` / `keys` served from the oracle's sampler: what `simulate.drive` needs of a manager."""

    def __init__(self, model, N):
        self.pi, self.T, self.E, self.q, self.keys = model
        self.calls = []

    def _hmm_tables(self):
        return self.pi, self.T, self.E

    def _simulate_call(self, lengths, alphabet, quiet, seed, contig0, rep0, nreps, cap, resume):
        assert quiet == self.q and list(alphabet) == list(range(len(self.E)))
        nc = len(lengths)
        self.calls.append(int(cap))
        x0 = np.full((nc, nreps), -1, dtype=np.int32)
        nev = np.zeros((nc, nreps), dtype=np.int64)
        pos = np.full((nc, nreps, cap), -7, dtype=np.int64)
        st = np.full((nc, nreps, cap), -7, dtype=np.int32)
        key = np.full((nc, nreps, cap), -7, dtype=np.int32)
        rout = np.zeros((nc, nreps, 3), dtype=np.int64)
        for c in range(nc):
            full = simref.sample(self.pi, self.T, self.E, self.q, int(lengths[c]), seed, contig0 + c, rep0 + np.arange(nreps))
            for k, (x, P, S, K) in enumerate(full):
                N = int(lengths[c])
                e0, p0, i0 = (0, 0, -1) if resume is None else (int(v) for v in np.asarray(resume).reshape(nc, nreps, 3)[c, k])
                if i0 < 0:
                    x0[c, k] = i0 = x
                if p0 >= N:
                    rout[c, k] = (e0, p0, i0)
                    continue
                m = min(cap, len(P) - e0)
                nev[c, k] = m
                pos[c, k, :m], st[c, k, :m], key[c, k, :m] = P[e0:e0 + m], S[e0:e0 + m], K[e0:e0 + m]
                e1 = e0 + m
                p1, i1 = (int(P[e1 - 1]), int(S[e1 - 1])) if e1 else (0, i0)
                if e1 == len(P) and p1 < N and m < cap:                    # the event that ends the contig is drawn as well
                    e1, p1 = e1 + 1, N
                rout[c, k] = (e1, p1, i1)
        return x0, nev, pos, st, key, rout


def test_drive_continues_every_replicate_to_N_whatever_the_capacity(model):
    from smcpp_amd import simulate
    L = [900, 400]
    want = [simref.sample(model[0], model[1], model[2], model[3], N, SEED, 5 + c, 2 + np.arange(3)) for c, N in enumerate(L)]
    for cap in (None, 1, 7, 1000):
        im = _MockManager(model, L)
        ev = simulate.drive(im, L, 3, SEED, None, model[3], first_replicate=2, first_contig=5, cap=cap)
        assert ev["calls"] == len(im.calls) and (cap is None or set(im.calls) == {cap})
        if cap is None:
            assert im.calls[0] == 16 and len(im.calls) == 2 and im.calls[1] > 64       # sized from N max (1 - s) plus a margin
        for c in range(2):
            for k in range(3):
                x, P, S, K = want[c][k]
                assert ev["x0"][c, k] == x and np.array_equal(ev["pos"][c][k], P) and np.array_equal(ev["state"][c][k], S)
                assert np.array_equal(ev["key"][c][k], K) and ev["pos"][c][k].dtype == np.int64
