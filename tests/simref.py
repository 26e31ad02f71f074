"""numpy oracle of the simulator (smcpp_simulate, smcpp_amd/csrc/simulate_dev.hpp): a float64 restatement of the contract of
include/smcpp_engine.h from what a manager's getters hand out - pi [M], T [M x M], the emission vectors of the alphabet EA [|A| x M] -
and `pathref.philox4x32`.  It shares nothing with the kernel: sequential cumulative sums, no lanes, no chunks.

The process: positions 0 .. N, x_0 ~ pi, x_p ~ T(x_{p-1}, .), o_p ~ Ebar(. | x_p), Ebar(k | m) = EA[k][m] / sum_k' EA[k'][m].  Walked by
events: from (p, i), s_i = T(i, i) Ebar(q | i), u_0 gives the quiet run G = floor(log(1 - u_0) / log s_i) clamped to N - p (finished when
p + G >= N), u_1 the state at the loud position p + G + 1 (weights T(i, j), j != i, and T(i, i)(1 - Ebar(q | i)) for j = i), u_2 its key
(weights EA[k][j], the quiet key's 0 when j = i); x_0 takes u_3 of event 0.  Every draw: x = min{ j : C_j > u C_last }, clamped.  u_t of
event e of replicate k of contig c: Philox4x32-10, counter (q lo, q hi, k, c) with q = 4 e + t, key (seed lo, seed hi ^ 0x53494D55).

`check_events` follows the DEVICE's own event list (a draw one ulp from a boundary would otherwise make every later event differ) and
holds each of the three draws of each event to the oracle's CDF interval, widened by a tolerance that comes from the arithmetic alone,
with u = 2^-53 and gamma_n = n u (Higham: a sum of n + 1 non-negative terms in ANY order has relative error at most gamma_n):

  state / key / x_0 draws.  The normalised C_x / C_last of either side differs from the exact one by the two sums (gamma_{n-1} each,
  n = M or |A| terms), by the weight T(i, i) (loud / mass) - two sums over the alphabet, a division, a product: 2 gamma_{|A|-1} + 2 u -
  and by the product u_t C_last (u); all other weights are inputs.  Per side 2 gamma_{n-1} + 2 gamma_{|A|-1} + 3 u, device and oracle
  together:            TAU_CDF = (4 max(M, |A|) + 4 |A| + 8) 2^-53          (1.5e-13 at M = 300, |A| = 14), on the [0, 1] scale.

  quiet run.  r = log(1 - u_0) / log s_i: 1 - u_0 is exact; the device's log is documented to 1 ulp = 2 u, the host's log of s_i (both
  sides) likewise; s_i = T(i, i) (EA[q][i] / mass) carries gamma_{|A|-1} + 2 u, which the logarithm turns into that over |ln s_i|
  RELATIVE to log s_i; the division adds u.  Per side 5 u + (|A| + 1) u / |ln s_i|, together
                       TAU_G(i) = (10 + (2 |A| + 2) / |ln s_i|) 2^-53,
  and G must lie in [floor(r (1 - TAU_G)), floor(r (1 + TAU_G))]: the integers a quotient within TAU_G of r can floor to.

No draw is excluded.  The tolerances are not fitted to device output; tests/test_gpu_simulate.py prints the worst distance it meets."""
import numpy as np

import pathref

U = 2.0 ** -53
SIM_KEY_XOR = 0x53494D55


def tau_cdf(M, A):
    return (4 * max(M, A) + 4 * A + 8) * U


def tau_g(A, ls):
    return (10.0 + (2 * A + 2) / np.abs(ls)) * U


def uniforms(seed, c, k, e, t):
    """u_t of event e of replicate k of contig c under `seed`; k, e broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = 4 * np.asarray(e, dtype=np.uint64) + np.uint64(t)
    k, q = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), q)
    ctr = np.stack([q & pathref.M32, q >> np.uint64(32), k & pathref.M32, np.full(q.shape, int(c), dtype=np.uint64)], axis=-1)
    out = pathref.philox4x32(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) ^ SIM_KEY_XOR], dtype=np.uint64))
    return pathref.words_to_uniform(out[..., 0], out[..., 1])


class Tables:
    """What depends on the state alone, in float64, by the formulas of the contract (the stay-loud weight without cancellation)."""

    def __init__(self, pi, T, EA, q):
        self.pi = np.asarray(pi, dtype=np.float64)
        self.T = np.asarray(T, dtype=np.float64)
        self.EA = np.asarray(EA, dtype=np.float64)                        # [|A|][M]
        self.q = int(q)
        self.M, self.A = len(self.pi), len(self.EA)
        assert self.T.shape == (self.M, self.M) and self.EA.shape == (self.A, self.M) and 0 <= self.q < self.A
        self.mass = self.EA.sum(axis=0)
        loud = np.delete(self.EA, self.q, axis=0).sum(axis=0) if self.A > 1 else np.zeros(self.M)
        d = np.diag(self.T)
        self.s = d * (self.EA[self.q] / self.mass)
        with np.errstate(divide="ignore"):
            self.ls = np.log(self.s)
        self.wst = d * (loud / self.mass)
        self.Ebar = self.EA / self.mass

    def state_weights(self, i):
        """[len(i)][M]: the weights of the successor of states i."""
        i = np.atleast_1d(i)
        W = self.T[i].copy()
        W[np.arange(len(i)), i] = self.wst[i]
        return W

    def key_weights(self, i, j):
        """[len(j)][|A|]: the weights of the key in states j entered from states i."""
        i, j = np.atleast_1d(i), np.atleast_1d(j)
        W = self.EA[:, j].T.copy()
        W[i == j, self.q] = 0.0
        return W


def _margin(W, u, x):
    """Distance by which u lies outside [C_{x-1}, C_x) / C_last on every line of W (a clamped x = last has no upper end)."""
    C = np.cumsum(W, axis=-1)
    tot = C[..., -1]
    at = np.arange(len(x))
    lo = np.where(x > 0, C[at, np.maximum(x - 1, 0)], 0.0) / tot
    hi = np.where(x < W.shape[-1] - 1, C[at, x] / tot, np.inf)
    return np.maximum(np.maximum(lo - u, u - hi), 0.0)


def check_events(pi, T, EA, q, N, seed, c, k, x0, pos, state, key):
    """Hold the event list of replicate k of contig c (x0; pos, state, key of the loud positions) to the oracle: raises
    AssertionError naming the first draw that lies outside its widened interval; -> dict of the worst distances met (CDF draws: on
    the [0, 1] scale; quiet runs: the relative distance of G's nearest admissible quotient from r) and the number of events."""
    tb = pi if isinstance(pi, Tables) else Tables(pi, T, EA, q)
    M, A = tb.M, tb.A
    pos = np.asarray(pos, dtype=np.int64)
    state = np.asarray(state, dtype=np.int64)
    key = np.asarray(key, dtype=np.int64)
    n = len(pos)
    assert state.shape == (n,) and key.shape == (n,), "event arrays differ in length"
    assert 0 <= int(x0) < M, f"x0 = {x0} is no state"
    assert n == 0 or (state.min() >= 0 and state.max() < M), "an event's state is out of range"
    assert n == 0 or (key.min() >= 0 and key.max() < A), "an event's key is out of range"
    assert n == 0 or (pos[0] >= 1 and np.all(np.diff(pos) >= 1)), "event positions do not ascend from 1"
    assert n == 0 or pos[-1] <= N, f"an event lies past N = {N}: position {int(pos[-1])}"
    tc = tau_cdf(M, A)
    # ---- x_0 ----
    m0 = float(_margin(tb.pi[None, :], uniforms(seed, c, k, 0, 3)[None], np.array([int(x0)]))[0])
    assert m0 <= tc, f"x0 = {x0}: u_3 of event 0 lies {m0:.3e} outside its CDF interval (bar {tc:.3e})"
    prev_s = np.concatenate([[int(x0)], state[:-1]])                      # the state every event starts from
    prev_p = np.concatenate([[0], pos[:-1]])
    ev = np.arange(n, dtype=np.int64)
    worst_g = 0.0
    # ---- quiet runs (the n recorded events, then the one that ends the contig) ----
    G = pos - prev_p - 1
    u0 = uniforms(seed, c, k, np.arange(n + 1, dtype=np.int64), 0)
    l1 = np.log(1.0 - u0)
    if n:
        ls = tb.ls[prev_s]
        assert np.all(ls < 0.0), "a loud position behind a state whose quiet run never ends (s >= 1)"
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(np.isinf(ls), 0.0, l1[:n] / ls)
            tg = np.where(np.isinf(ls), 0.0, tau_g(A, ls))
        lo, hi = np.floor(r * (1.0 - tg)), np.floor(r * (1.0 + tg))
        bad = np.nonzero((G < lo) | (G > hi))[0]
        assert len(bad) == 0, (f"event {int(bad[0])}: quiet run G = {int(G[bad[0]])} from position {int(prev_p[bad[0]])}, the oracle's "
                               f"quotient is {r[bad[0]]:.17g} (admissible {lo[bad[0]]:.0f} .. {hi[bad[0]]:.0f})")
        off = G != np.floor(r)
        if off.any():
            worst_g = float(np.max(np.abs(np.where(G[off] > r[off], G[off], G[off] + 1) - r[off]) / np.maximum(r[off], 1e-300)))
    pN, iN = (int(pos[-1]), int(state[-1])) if n else (0, int(x0))
    if pN < N:
        lsN = tb.ls[iN]
        if lsN < 0.0:
            rN = 0.0 if np.isinf(lsN) else l1[n] / lsN
            tgN = 0.0 if np.isinf(lsN) else float(tau_g(A, lsN))
            assert np.floor(rN * (1.0 + tgN)) >= N - pN, (f"the list ends at position {pN} < N = {N}, but the quiet run of event {n} "
                                                           f"is {rN:.17g} positions: a loud position is missing")
    # ---- successor states and keys ----
    worst_c = m0
    if n:
        ms = _margin(tb.state_weights(prev_s), uniforms(seed, c, k, ev, 1), state)
        bad = np.nonzero(ms > tc)[0]
        assert len(bad) == 0, (f"event {int(bad[0])} at position {int(pos[bad[0]])}: state {int(state[bad[0]])} from "
                               f"{int(prev_s[bad[0]])}: u_1 lies {ms[bad[0]]:.3e} outside its CDF interval (bar {tc:.3e})")
        mk = _margin(tb.key_weights(prev_s, state), uniforms(seed, c, k, ev, 2), key)
        bad = np.nonzero(mk > tc)[0]
        assert len(bad) == 0, (f"event {int(bad[0])} at position {int(pos[bad[0]])}: key {int(key[bad[0]])} in state "
                               f"{int(state[bad[0]])}: u_2 lies {mk[bad[0]]:.3e} outside its CDF interval (bar {tc:.3e})")
        worst_c = max(worst_c, float(ms.max()), float(mk.max()))
    return {"events": n, "worst_cdf": worst_c, "worst_run": worst_g}


def _draw(W, u):
    return pathref._draw(W, u).astype(np.int64)


def sample(pi, T, EA, q, N, seed, c, replicates):
    """The oracle's own event-driven sampler, vectorised over the replicates (a count, or the replicate indices).
    -> list of (x0, pos int64, state int32, key int32) per replicate."""
    tb = pi if isinstance(pi, Tables) else Tables(pi, T, EA, q)
    ks = pathref._path_ids(replicates)
    R = len(ks)
    i = _draw(np.broadcast_to(tb.pi, (R, tb.M)), uniforms(seed, c, ks, 0, 3))
    x0 = i.copy()
    p = np.zeros(R, dtype=np.int64)
    out = [([], [], []) for _ in range(R)]
    act = np.arange(R)
    e = 0
    while len(act):
        ia, pa = i[act], p[act]
        ls = tb.ls[ia]
        room = N - pa
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.floor(np.log(1.0 - uniforms(seed, c, ks[act], e, 0)) / ls)
        r = np.where(np.isinf(ls), 0.0, r)
        G = np.where(ls >= 0.0, room, np.where(r >= room, room, r)).astype(np.int64)
        go = G < room
        p[act[~go]] = N
        act, ia, pa, G = act[go], ia[go], pa[go], G[go]
        if len(act) == 0:
            break
        pn = pa + G + 1
        j = _draw(tb.state_weights(ia), uniforms(seed, c, ks[act], e, 1))
        kx = _draw(tb.key_weights(ia, j), uniforms(seed, c, ks[act], e, 2))
        for a, P, J, K in zip(act, pn, j, kx):
            out[a][0].append(P); out[a][1].append(J); out[a][2].append(K)
        p[act], i[act] = pn, j
        act = act[pn < N]
        e += 1
    return [(int(x0[a]), np.array(out[a][0], dtype=np.int64), np.array(out[a][1], dtype=np.int32), np.array(out[a][2], dtype=np.int32))
            for a in range(R)]


def expand(N, q, x0, pos, state, key):
    """Events -> the state at positions 0 .. N and the key at positions 1 .. N (entry 0 of the keys: -1)."""
    pos = np.asarray(pos, dtype=np.int64)
    st = np.concatenate([[int(x0)], np.asarray(state, dtype=np.int64)])
    first = np.concatenate([[0], pos, [N + 1]])
    x = np.repeat(st, np.diff(first))
    o = np.full(N + 1, q, dtype=np.int64)
    o[0] = -1
    o[pos] = key
    return x.astype(np.int32), o.astype(np.int32)


def sample_positionwise(pi, T, EA, N, rng, R):
    """The naive walk p = 1 .. N with numpy's generator `rng`: -> states [R][N + 1], keys [R][N + 1] (entry 0: -1)."""
    tb = Tables(pi, T, EA, 0)
    pi_ = tb.pi / tb.pi.sum()
    Tn = tb.T / tb.T.sum(axis=1, keepdims=True)
    X = np.empty((R, N + 1), dtype=np.int32)
    O = np.full((R, N + 1), -1, dtype=np.int32)
    x = _draw(np.broadcast_to(pi_, (R, tb.M)), rng.random(R))
    X[:, 0] = x
    for p in range(1, N + 1):
        x = _draw(Tn[x], rng.random(R))
        X[:, p] = x
        O[:, p] = _draw(tb.Ebar[:, x].T, rng.random(R))
    return X, O


def marginals(pi, T, EA, N):
    """-> (state marginals pi T^p [N + 1][M], key marginals (pi T^p) Ebar [N + 1][|A|]; line 0 of the keys is unused)."""
    tb = Tables(pi, T, EA, 0)
    a = tb.pi / tb.pi.sum()
    Tn = tb.T / tb.T.sum(axis=1, keepdims=True)
    S = np.empty((N + 1, tb.M))
    for p in range(N + 1):
        S[p] = a
        a = a @ Tn
    return S, S @ tb.Ebar.T


def frequencies(X, n):
    """[P][n]: the share of the lines of X [K][P] that hold each value 0 .. n - 1 at every column."""
    return pathref.state_frequencies(X, n)
