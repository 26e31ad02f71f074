"""Run the model forwards: data sets and hidden paths drawn from pi, T and the emission table a manager holds, on the device
(`smcpp_simulate`, smcpp_amd/csrc/simulate_dev.hpp; include/smcpp_engine.h states the process and the random stream).

    alphabet, quiet = full_alphabet(n)                       the complete observations of n undistinguished lineages
    sim = Simulator(model, n, hidden_states, theta, rho)     one manager over a listing of the alphabet
    contigs, paths = sim.contigs(lengths, replicates, seed)  `Contig`s that Analysis / vcf2smc.write_smc accept + the hidden paths
    models = parametric_bootstrap("model.final.json", n, lengths, B, seed, EstimateArgs(...))
    band = size_history_band(models, t, (0.025, 0.5, 0.975))

The device returns EVENTS - the loud positions of a contig, with the state and the key drawn there; `events_to_rows` turns them into
`.smc` rows, `events_to_segments` into the hidden path as runs of equal state.  Out of scope: missing data (a = -1) in simulated
contigs, thinning / binning (the output is bp-level rows; the existing pipeline shapes them)."""
from __future__ import annotations

import numpy as np

from . import data as D

CELL_BUDGET = 1 << 24            # events per device call over all (contig, replicate) pairs (16 bytes each on either side)


# ---------------------------------------------------------------------------------------------------------------------------------
# alphabets
# ---------------------------------------------------------------------------------------------------------------------------------
def full_alphabet(n, a=2):
    """Every complete observation (a', b, nb = n) of `a` distinguished and `n` undistinguished lineages, lexicographic (the order
    a manager keeps its keys in), WITHOUT the derived-monomorphic twin (a, n, n): `recode_monomorphic` maps it onto (0, 0, n), and
    the emission table gives both the same vector.  -> (keys int32 [K, 3], index of the quiet entry (0, 0, n)); K = (a + 1)(n + 1) - 1."""
    keys = [(x, b, n) for x in range(a + 1) for b in range(n + 1) if not (x == a and b == n)]
    return np.array(keys, dtype=np.int32), keys.index((0, 0, n))


def full_alphabet_twopop(n1, n2, a1=2, a2=0):
    """The two-population form: (a1', b1, n1, a2', b2, n2) without the twin (a1, n1, n1, a2, n2, n2).  -> (keys int32 [K, 6], index
    of the quiet entry (0, 0, n1, 0, 0, n2))."""
    keys = [(x1, b1, n1, x2, b2, n2) for x1 in range(a1 + 1) for b1 in range(n1 + 1) for x2 in range(a2 + 1) for b2 in range(n2 + 1)
            if not (x1 == a1 and b1 == n1 and x2 == a2 and b2 == n2)]
    return np.array(keys, dtype=np.int32), keys.index((0, 0, n1, 0, 0, n2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the device calls: continue every replicate until its position reaches N
# ---------------------------------------------------------------------------------------------------------------------------------
def _default_quiet(keys, alphabet):
    """The alphabet's key with a = b = 0 in every population and the most observed lineages."""
    best, best_nb = None, -1
    for k in alphabet:
        r = keys[k]
        if np.all(r[0::3] == 0) and np.all(r[1::3] == 0) and int(r[2::3].sum()) > best_nb:
            best, best_nb = int(k), int(r[2::3].sum())
    if best is None:
        raise RuntimeError("simulate: the alphabet holds no monomorphic key (a = b = 0): name the quiet key")
    return best


def _im_keys(im):
    return np.asarray(im._keys() if hasattr(im, "_keys") else im.keys)


def event_rate(T, E, alphabet, quiet):
    """max_i (1 - s_i), s_i = T(i, i) Ebar(q | i): the largest chance of a position to be loud."""
    EA = np.asarray(E)[np.asarray(alphabet)]
    s = np.diag(T) * EA[list(alphabet).index(quiet)] / EA.sum(axis=0)
    return float(np.max(1.0 - s))


def drive(im, lengths, n_replicates=1, seed=0, alphabet=None, quiet=None, first_replicate=0, first_contig=0, cap=None):
    """`im.simulate` of both bindings (which provide `_simulate_call` and `_hmm_tables`)."""
    lengths = np.ascontiguousarray(np.atleast_1d(np.asarray(lengths, dtype=np.int64)).reshape(-1))
    keys = _im_keys(im)
    alphabet = np.arange(len(keys), dtype=np.int32) if alphabet is None else np.ascontiguousarray(alphabet, dtype=np.int32).reshape(-1)
    if quiet is None:
        quiet = _default_quiet(keys, [k for k in alphabet if 0 <= k < len(keys)])
    nc, R = len(lengths), int(n_replicates)
    fixed = cap is not None

    def call(cap_, resume):
        return im._simulate_call(lengths, alphabet, quiet, seed, first_contig, first_replicate, R, cap_, resume)

    if fixed:
        cap_ = int(cap)
    else:
        # the first call checks the arguments and prepares the parameters with a token capacity; the capacity of the calls behind it
        # comes from the model: N max_i (1 - s_i) events are expected at most, plus six standard deviations and a constant
        cap_ = 16
    x0, pieces, resume, ncalls, rate = None, [], None, 0, None
    while True:
        r = call(cap_, resume)
        ncalls += 1
        if x0 is None:
            x0 = r[0].copy()
        # (only what a call has written is kept: the events of all pairs behind each other, and where each pair's begin)
        nev = r[1].reshape(-1)
        live = np.arange(r[2].shape[2])[None, :] < nev[:, None]
        off = np.concatenate([[0], np.cumsum(nev)])
        pieces.append((off, r[2].reshape(len(nev), -1)[live], r[3].reshape(len(nev), -1)[live], r[4].reshape(len(nev), -1)[live]))
        resume = r[5]
        left = lengths[:, None] - resume[:, :, 1]
        del r
        if not np.any(left > 0):
            break
        if not fixed:
            if rate is None:
                _, T, E = im._hmm_tables()
                rate = event_rate(T, E, alphabet, quiet)
            mean = float(left.max()) * rate
            want = int(mean + 6.0 * np.sqrt(mean) + 64)
            cap_ = max(16, min(want, CELL_BUDGET // max(1, nc * R)))
    out = {"x0": x0, "pos": [], "state": [], "key": [], "calls": ncalls}
    for c in range(nc):
        P, S, K = [], [], []
        for k in range(R):
            u = c * R + k
            P.append(np.concatenate([p[1][p[0][u]:p[0][u + 1]] for p in pieces]))
            S.append(np.concatenate([p[2][p[0][u]:p[0][u + 1]] for p in pieces]))
            K.append(np.concatenate([p[3][p[0][u]:p[0][u + 1]] for p in pieces]))
        out["pos"].append(P); out["state"].append(S); out["key"].append(K)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# events -> rows, events -> the hidden path
# ---------------------------------------------------------------------------------------------------------------------------------
def events_to_rows(N, pos, key, key_rows, quiet):
    """`.smc` rows (span, a, b, nb[, ...]) int32 of a contig of N positions whose loud positions `pos` (ascending, 1 .. N) carry the
    alphabet entries `key`; `key_rows[k]` is the observation of entry k, `quiet` the quiet entry's index.  Quiet runs, span-1 loud
    rows, adjacent equal rows merged as `compress_repeated_obs` does; an event that emits the quiet key leaves no row."""
    pos = np.asarray(pos, dtype=np.int64)
    key = np.asarray(key, dtype=np.int64)
    key_rows = np.asarray(key_rows, dtype=np.int32)
    assert pos.shape == key.shape and (len(pos) == 0 or (pos[0] >= 1 and pos[-1] <= N and np.all(np.diff(pos) > 0)))
    loud = key != quiet
    pos, key = pos[loud], key[loud]
    m = len(pos)
    gaps = np.diff(np.concatenate([[0], pos, [N + 1]])) - 1                # quiet positions in front of every loud one, and behind the last
    rows = np.empty((2 * m + 1, 1 + key_rows.shape[1]), dtype=np.int32)
    assert gaps.max() < 2 ** 31
    rows[0::2, 0] = gaps
    rows[0::2, 1:] = key_rows[quiet]
    rows[1::2, 0] = 1
    rows[1::2, 1:] = key_rows[key]
    rows = rows[rows[:, 0] > 0]
    return np.ascontiguousarray(D.compress_repeated_obs(rows), dtype=np.int32)


def events_to_segments(N, x0, pos, state):
    """The hidden path over positions 0 .. N as runs of equal state: int64 [S, 3] rows (state, first position, last position)."""
    pos = np.asarray(pos, dtype=np.int64)
    st = np.concatenate([[int(x0)], np.asarray(state, dtype=np.int64)])
    first = np.concatenate([[0], pos])
    keep = np.ones(len(st), dtype=bool)
    keep[1:] = st[1:] != st[:-1]
    st, first = st[keep], first[keep]
    last = np.concatenate([first[1:] - 1, [N]])
    return np.stack([st, first, last], axis=1).astype(np.int64)


def segments_to_path(seg):
    """The states at positions 0 .. N from `events_to_segments`' rows."""
    seg = np.asarray(seg, dtype=np.int64)
    return np.repeat(seg[:, 0], seg[:, 2] - seg[:, 1] + 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the simulator
# ---------------------------------------------------------------------------------------------------------------------------------
class Simulator:
    """One manager over a one-contig listing of the alphabet (so that its emission table holds exactly these keys: nothing of the
    emission assembly is restated), with `model`, theta, rho and alpha set.  `n`: the undistinguished sample size, or (n1, n2) with
    a two-population model and `a` = (a1, a2)."""

    def __init__(self, model, n, hidden_states, theta, rho, alpha=1.0, polarization_error=0.5, a=None, device=-1, cython=False):
        if cython:
            from . import _smcpp_cy as B
        else:
            from . import _smcpp as B
        self.hidden_states = np.asarray(hidden_states, dtype=np.float64)
        if np.isscalar(n):
            self.n, self.a = [int(n)], [2]
            keys, q = full_alphabet(int(n), 2)
            pid = (getattr(model, "pid", None) or "pop1",)
            listing = np.ascontiguousarray(np.hstack([np.ones((len(keys), 1), dtype=np.int32), keys]))
            self.im = B.PyOnePopInferenceManager(int(n), [listing], self.hidden_states, pid, polarization_error, device)
        else:
            self.n, self.a = [int(x) for x in n], [int(x) for x in (a or (2, 0))]
            keys, q = full_alphabet_twopop(self.n[0], self.n[1], self.a[0], self.a[1])
            pid = tuple(model.pids)
            listing = np.ascontiguousarray(np.hstack([np.ones((len(keys), 1), dtype=np.int32), keys]))
            self.im = B.PyTwoPopInferenceManager(self.n[0], self.n[1], self.a[0], self.a[1], [listing], self.hidden_states, pid,
                                                 polarization_error, device)
        self.pid = pid
        self.im.model = model
        self.im.theta = theta; self.im.rho = rho; self.im.alpha = alpha
        # the manager sorts its keys; the alphabet is the list of their indices, in the alphabet's own (the same) order
        lut = {tuple(int(x) for x in k): i for i, k in enumerate(_im_keys(self.im))}
        self.key_rows = keys
        self.alphabet = np.array([lut[tuple(int(x) for x in k)] for k in keys], dtype=np.int32)
        self.quiet_entry = q
        self.quiet = int(self.alphabet[q])

    def tables(self):
        """(pi, T, E restricted to the alphabet [|A|, M]) in float64, as the manager's getters hand them out."""
        self.im._simulate_call([1], self.alphabet, self.quiet, 0, 0, 0, 1, 1, None)         # (prepares the parameters if need be)
        pi, T, E = self.im._hmm_tables()
        return pi, T, E[self.alphabet]

    def alphabet_mass(self):
        """sum_{k in A} E[k][m] per state: 1 up to the 1e-10 floors of incorporate_theta, |A| 1e-10 at most, and rounding."""
        return self.tables()[2].sum(axis=0)

    def events(self, lengths, replicates=1, seed=0, first_replicate=0, first_contig=0, cap=None):
        """`im.simulate` over this simulator's alphabet (keys come back as indices into `key_rows`)."""
        return self.im.simulate(lengths, replicates, seed, self.alphabet, self.quiet, first_replicate, first_contig, cap)

    def contigs(self, lengths, replicates=1, seed=0, first_replicate=0):
        """-> (contigs, paths), each `[replicate][contig]`: `Contig`s of bp-level rows and `events_to_segments` arrays."""
        lengths = [int(x) for x in np.atleast_1d(lengths)]
        ev = self.events(lengths, replicates, seed, first_replicate)
        contigs, paths = [], []
        for r in range(int(replicates)):
            cs, ps = [], []
            for c, N in enumerate(lengths):
                rows = events_to_rows(N, ev["pos"][c][r], ev["key"][c][r], self.key_rows, self.quiet_entry)
                cs.append(D.Contig(data=rows, pid=self.pid, n=list(self.n), a=list(self.a), fn="simulated:%d:%d" % (first_replicate + r, c)))
                ps.append(events_to_segments(N, ev["x0"][c, r], ev["pos"][c][r], ev["state"][c][r]))
            contigs.append(cs); paths.append(ps)
        return contigs, paths


# ---------------------------------------------------------------------------------------------------------------------------------
# the parametric bootstrap
# ---------------------------------------------------------------------------------------------------------------------------------
def parametric_bootstrap(final_json, n, lengths, B, seed=0, estimate_args=None, device=-1):
    """Draw B data sets of contigs of `lengths` base pairs from the one-population model of a `model.final.json` (a path or the
    loaded dict; theta and rho per base pair as it states them, its hidden states), refit each with `Analysis(estimate_args)` and
    return the B fitted models.  The same seed gives the same data sets and - numpy's generator is seeded per replicate for the
    initial jitter and the hidden-state mixture of `Analysis` - the same fits."""
    from . import analysis as A
    d = A._load_final(final_json)
    model = A.model_from_dict(d["model"])
    if getattr(model, "NPOP", 1) != 1:
        raise RuntimeError("parametric_bootstrap: one-population models only")
    args = estimate_args or A.EstimateArgs()
    hs = d["hidden_states"][model.pid] if isinstance(d["hidden_states"], dict) else d["hidden_states"]
    pol = 0.0 if args.unfold else args.polarization_error
    sim = Simulator(model, n, hs, d["theta"], d["rho"], 1.0, pol, device=device)
    contigs, _ = sim.contigs(lengths, B, seed)
    fitted = []
    state = np.random.get_state()
    try:
        for r in range(int(B)):
            np.random.seed((int(seed) * 1000003 + r) % (2 ** 32))
            an = A.Analysis(contigs[r], args)
            an.run()
            fitted.append(an.model)
    finally:
        np.random.set_state(state)
    return fitted


def size_history_band(models, t, quantiles=(0.025, 0.5, 0.975)):
    """Pointwise quantiles of N(t) over fitted models: t in generations, N(t) = N0 model(t / (2 N0)).  -> [len(quantiles), len(t)]."""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    curves = np.array([m.N0 * np.asarray(m(t / (2.0 * m.N0)), dtype=np.float64) for m in models])
    return np.quantile(curves, np.asarray(quantiles, dtype=np.float64), axis=0)
