"""Host-side mirror of the reference's ``smcpp._smcpp`` module surface for the E-step path.

Same class names, constructor signatures, properties and error behaviour as ``smcpp/_smcpp.pyx``
(``_PyInferenceManager`` 122-308, ``PyOnePopInferenceManager`` 310-332, ``PyTwoPopInferenceManager`` 334-368),
implemented over the C ABI of ``include/smcpp_engine.h``.  The compute runs in HIP kernels on the MI355X;
nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _engine as E

aca = np.ascontiguousarray


def set_num_threads(k):
    """``_smcpp.pyx:61-64``."""
    E.lib().smcpp_set_num_threads(int(k))


class _PyInferenceManager:
    def _my_init(self, observations, hidden_states, im_id=None):
        self._im = None
        self._im_id = im_id
        self.seed = 1
        if len(observations) == 0:
            raise RuntimeError("Observations list is empty")
        hidden_states = np.asarray(hidden_states, dtype=np.float64)
        if not np.all(np.sort(hidden_states) == hidden_states):
            raise RuntimeError("Hidden states must be in ascending order")
        self._observations = [aca(ob, dtype=np.int32) for ob in observations]
        self._Ls = np.array([ob.shape[0] for ob in self._observations], dtype=np.int32)
        self._hs = aca(hidden_states)
        self._num_hmms = len(observations)
        self._model = None
        self._theta = self._rho = self._alpha = None

    def _ptrs(self):
        arr = (C.POINTER(C.c_int) * self._num_hmms)()
        for i, ob in enumerate(self._observations):
            arr[i] = ob.ctypes.data_as(C.POINTER(C.c_int))
        return arr

    def __del__(self):
        im = getattr(self, "_im", None)
        if im and E is not None:         # (at interpreter shutdown the module globals may already be gone)
            try:
                E.lib().smcpp_destroy(im)
            except Exception:  # noqa: BLE001
                pass
            self._im = None

    # ---- properties mirrored from _smcpp.pyx:157-183 ----
    @property
    def observations(self):
        return self._observations

    @property
    def theta(self):
        return self._theta

    @theta.setter
    def theta(self, v):
        self._theta = v
        E.check(E.lib().smcpp_set_theta(self._im, float(v)))

    @property
    def rho(self):
        return self._rho

    @rho.setter
    def rho(self, v):
        self._rho = v
        E.check(E.lib().smcpp_set_rho(self._im, float(v)))

    @property
    def alpha(self):
        return self._alpha

    @alpha.setter
    def alpha(self, v):
        self._alpha = v
        E.check(E.lib().smcpp_set_alpha(self._im, float(v)))

    def E_step(self, forward_backward_only=False):
        """``_smcpp.pyx:185-191``."""
        if None in (self.theta, self.rho, self.alpha):
            raise RuntimeError("theta / rho / alpha must be set")
        E.check(E.lib().smcpp_estep(self._im, int(bool(forward_backward_only))))

    @property
    def model(self):
        return self._model

    @model.setter
    def model(self, m):
        self._model = m
        if hasattr(m, "register"):
            m.register(self)
        self.update("model update")

    @property
    def save_gamma(self):
        return bool(E.lib().smcpp_get_save_gamma(self._im))

    @save_gamma.setter
    def save_gamma(self, sg):
        E.check(E.lib().smcpp_set_save_gamma(self._im, int(bool(sg))))

    @property
    def hidden_states(self):
        hs = np.zeros(len(self._hs))
        E.check(E.lib().smcpp_get_hidden_states(self._im, E.dptr(hs)))
        return list(hs)

    @hidden_states.setter
    def hidden_states(self, hs):
        hs = aca(hs, dtype=np.float64)
        if len(hs) != len(self._hs):
            raise RuntimeError("hidden states must be same size")
        E.check(E.lib().smcpp_set_hidden_states(self._im, len(hs), E.dptr(hs)))

    @property
    def M(self):
        return len(self._hs) - 1

    @property
    def keys(self):
        K = E.lib().smcpp_num_keys(self._im)
        kl = E.lib().smcpp_key_len(self._im)
        k = np.zeros((K, kl), dtype=np.int32)
        E.check(E.lib().smcpp_get_keys(self._im, E.iptr(k)))
        return k

    @property
    def emission_probs(self):
        keys = self.keys
        out = np.zeros((len(keys), self.M))
        E.check(E.lib().smcpp_get_emission_probs(self._im, E.dptr(out)))
        return {tuple(int(x) for x in k): out[i].copy() for i, k in enumerate(keys)}

    @property
    def gamma_sums(self):
        keys = self.keys
        ret = []
        for c in range(self._num_hmms):
            vals = np.zeros((len(keys), self.M))
            present = np.zeros(len(keys), dtype=np.uint8)
            E.check(E.lib().smcpp_get_gamma_sums(self._im, c, E.dptr(vals),
                                                 present.ctypes.data_as(C.POINTER(C.c_ubyte))))
            ret.append({tuple(int(x) for x in keys[k]): vals[k].copy() for k in range(len(keys)) if present[k]})
        return ret

    @property
    def gammas(self):
        ret = []
        for c in range(self._num_hmms):
            # sized from what the LAST E-step stored (the save_gamma flag may have been toggled since)
            ncol = int(E.lib().smcpp_gamma_cols(self._im, c))
            g = np.zeros((self.M, ncol))
            E.check(E.lib().smcpp_get_gamma(self._im, c, E.dptr(g)))
            ret.append(g)
        return ret

    def gamma_argmax(self, c=0):
        out = np.zeros(int(self._Ls[c]) + 1, dtype=np.int32)
        E.check(E.lib().smcpp_get_gamma_argmax(self._im, c, E.iptr(out)))
        return out

    # ---- posterior products computed on the device (include/smcpp_engine.h: smcpp_posterior_*; no counterpart in _smcpp.pyx) ----
    def _selection(self, c, start, stop, step):
        c = int(c)
        if stop is None:
            stop = int(self._Ls[c]) + 1 if 0 <= c < self._num_hmms else 1   # (a bad contig index: the engine raises)
        start, stop, step = int(start), int(stop), int(step)
        ncols = max(0, -(-(stop - start) // step)) if step >= 1 else 0      # (bad arguments: the engine raises before ncols is used)
        return start, stop, step, ncols

    def posterior_columns(self, c=0, start=0, stop=None, step=1, dtype=np.float64, normalize=True):
        """Columns `range(start, stop, step)` of the posterior of contig `c` as `[M, ncols]` in `dtype` (float64 or float32):
        normalised to sum to one per column, or (`normalize=False`) the stored values, bit for bit those of `gammas[c]`.  The
        matrix is transposed (and normalised) on the device."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("posterior_columns: dtype must be float64 or float32")
        start, stop, step, ncols = self._selection(c, start, stop, step)
        out = np.empty((self.M, ncols), dtype=dtype)
        E.check(E.lib().smcpp_posterior_columns(self._im, int(c), start, stop, step, int(bool(normalize)),
                                                int(dtype == np.dtype(np.float32)), out.ctypes.data_as(C.c_void_p), None))
        return out

    def posterior_summary(self, c=0, weights=None, quantiles=(), start=0, stop=None, step=1):
        """Per selected column of contig `c`, without fetching the matrix: dict of `colsum` (sum over the states), `argmax` (first
        maximum), `mean` (`sum_m weights[m] p[m, l]`; absent without weights) and `qstate` `[len(quantiles), ncols]`, the first
        state at which the cumulative posterior reaches each level (at most 8 levels, each in (0, 1))."""
        start, stop, step, ncols = self._selection(c, start, stop, step)
        q = aca(np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1))
        w = None if weights is None else aca(weights, dtype=np.float64).reshape(-1)
        if w is not None and len(w) != self.M:
            raise RuntimeError(f"posterior_summary: {len(w)} weights for {self.M} hidden states")
        ret = {"colsum": np.empty(ncols), "argmax": np.empty(ncols, dtype=np.int32), "qstate": np.empty((len(q), ncols), dtype=np.int32)}
        if w is not None:
            ret["mean"] = np.empty(ncols)
        E.check(E.lib().smcpp_posterior_summary(self._im, int(c), start, stop, step, E.dptr(w), len(q), E.dptr(q) if len(q) else None,
                                                E.dptr(ret["colsum"]), E.iptr(ret["argmax"]), E.dptr(ret.get("mean")),
                                                E.iptr(ret["qstate"]) if len(q) else None))
        return ret

    def posterior_windows(self, c=0, window=10_000):
        """`[M, ceil(P_L / window)]`: the posterior of contig `c` averaged over windows of `window` base pairs (row `l >= 1` covers
        the base pairs `[P_{l-1}, P_l)`, `P` the cumulative spans of the rows the manager was given; column 0 takes no part)."""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_posterior_windows(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty((self.M, nw.value))
        E.check(E.lib().smcpp_posterior_windows(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def posterior_transitions(self, c=0, start=0, stop=None, step=1):
        """Where the hidden state changes: dict of `stay`, `up`, `down`, each `[ncols]` over the columns `range(start, stop, step)` of
        contig `c` - the expected number of the row's positions at which the state stays, moves to a higher index (an older state)
        or to a lower one.  They sum to the row's span; column 0 holds zeros.  (include/smcpp_engine.h: smcpp_posterior_transitions.)"""
        start, stop, step, ncols = self._selection(c, start, stop, step)
        ret = {k: np.empty(ncols) for k in ("stay", "up", "down")}
        E.check(E.lib().smcpp_posterior_transitions(self._im, int(c), start, stop, step, E.dptr(ret["stay"]), E.dptr(ret["up"]),
                                                    E.dptr(ret["down"])))
        return ret

    def posterior_transition_windows(self, c=0, window=10_000):
        """`[3, ceil(P_L / window)]`: expected stay / up / down counts of contig `c` per window of `window` base pairs, every row
        apportioned uniformly over its base pairs; the three rows of a window sum to its covered base pairs."""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_posterior_transition_windows(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty((3, nw.value))
        E.check(E.lib().smcpp_posterior_transition_windows(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def posterior_sample_rows(self, c=0, n_paths=1, seed=0, first_path=0, start=0, stop=None, step=1):
        """Joint draws of the hidden-state path of contig `c` from the posterior (forward filtering, backward sampling on the device),
        reduced per row: dict of `state`, `up`, `down`, each int32 `[n_paths, ncols]` over the columns `range(start, stop, step)` -
        the state at the row's last position and the number of the row's positions at which the sampled path moves to a higher /
        lower state; column 0 holds the state at position 0 and zeros.  Path `first_path + k` under `seed` is the same whatever
        else a call asks for (include/smcpp_engine.h: smcpp_posterior_sample_rows states the contract and the random stream)."""
        start, stop, step, ncols = self._selection(c, start, stop, step)
        args = (self._im, int(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_path), int(n_paths), start, stop, step)
        E.check(E.lib().smcpp_posterior_sample_rows(*args, None, None, None))      # (the checks alone: nothing is allocated for a bad call)
        ret = {k: np.empty((int(n_paths), ncols), dtype=np.int32) for k in ("state", "up", "down")}
        E.check(E.lib().smcpp_posterior_sample_rows(*args, E.iptr(ret["state"]), E.iptr(ret["up"]), E.iptr(ret["down"])))
        return ret

    def posterior_sample_positions(self, c=0, n_paths=1, seed=0, first_path=0, pos0=0, pos1=None):
        """int32 `[n_paths, pos1 - pos0]`: the states of the sampled paths `first_path .. first_path + n_paths - 1` of contig `c` at
        positions `pos0 .. pos1 - 1` of `0 .. P_L` (position 0 is column 0, row `l` covers positions `P_{l-1} + 1 .. P_l`;
        default: all of them)."""
        c = int(c)
        if pos1 is None:
            pos1 = int(self._observations[c][:, 0].sum(dtype=np.int64)) + 1 if 0 <= c < self._num_hmms else 1     # (a bad contig index: the engine raises)
        pos0, pos1 = int(pos0), int(pos1)
        args = (self._im, c, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_path), int(n_paths), pos0, pos1)
        E.check(E.lib().smcpp_posterior_sample_positions(*args, None))             # (the checks alone)
        out = np.empty((int(n_paths), pos1 - pos0), dtype=np.int32)
        E.check(E.lib().smcpp_posterior_sample_positions(*args, E.iptr(out)))
        return out

    def _grid(self, c, pos0, pos1, step):
        c = int(c)
        if pos1 is None:
            pos1 = int(self._observations[c][:, 0].sum(dtype=np.int64)) + 1 if 0 <= c < self._num_hmms else 1     # (a bad contig index: the engine raises)
        pos0, pos1, step = int(pos0), int(pos1), int(step)
        npos = max(0, -(-(pos1 - pos0) // step)) if step >= 1 else 0          # (bad arguments: the engine raises before npos is used)
        return c, pos0, pos1, step, npos

    def posterior_positions(self, c=0, pos0=0, pos1=None, step=1):
        """`[M, npos]`: the posterior of the single positions `range(pos0, pos1, step)` of `0 .. P_L` of contig `c` (position 0 is
        column 0, row `l` covers positions `P_{l-1} + 1 .. P_l`; default: all of them), every column summing to one.
        (include/smcpp_engine.h: smcpp_posterior_positions.)"""
        c, pos0, pos1, step, npos = self._grid(c, pos0, pos1, step)
        E.check(E.lib().smcpp_posterior_positions(self._im, c, pos0, pos1, step, None))            # (the checks alone)
        out = np.empty((self.M, npos))
        E.check(E.lib().smcpp_posterior_positions(self._im, c, pos0, pos1, step, E.dptr(out)))
        return out

    def posterior_position_summary(self, c=0, weights=None, quantiles=(), pos0=0, pos1=None, step=1):
        """Per position of the grid `range(pos0, pos1, step)` of contig `c`, without fetching the columns: dict of `argmax` (the
        lowest state of maximal posterior), `mean` (`sum_m weights[m] gamma_p(m)`; absent without weights) and `qstate`
        `[len(quantiles), npos]`, the first state at which the cumulative posterior reaches each level (at most 8, each in (0, 1))."""
        c, pos0, pos1, step, npos = self._grid(c, pos0, pos1, step)
        q = aca(np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).reshape(-1))
        w = None if weights is None else aca(weights, dtype=np.float64).reshape(-1)
        if w is not None and len(w) != self.M:
            raise RuntimeError(f"posterior_position_summary: {len(w)} weights for {self.M} hidden states")
        args = (self._im, c, pos0, pos1, step, E.dptr(w), len(q), E.dptr(q) if len(q) else None)
        E.check(E.lib().smcpp_posterior_position_summary(*args, None, None, None))                 # (the checks alone)
        ret = {"argmax": np.empty(npos, dtype=np.int32), "qstate": np.empty((len(q), npos), dtype=np.int32)}
        if w is not None:
            ret["mean"] = np.empty(npos)
        E.check(E.lib().smcpp_posterior_position_summary(*args, E.iptr(ret["argmax"]), E.dptr(ret.get("mean")),
                                                         E.iptr(ret["qstate"]) if len(q) else None))
        return ret

    def posterior_windows_exact(self, c=0, window=10_000):
        """`[M, ceil(P_L / window)]`: the posterior of contig `c` averaged over windows of `window` base pairs like
        `posterior_windows`, but exact on rows that a window boundary cuts: their interior is walked position by position
        instead of being apportioned uniformly."""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_posterior_windows_exact(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty((self.M, nw.value))
        E.check(E.lib().smcpp_posterior_windows_exact(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def loglik_rows(self, c=0, start=0, stop=None, step=1):
        """`[ncols]`: log c of the caller's rows `range(start, stop, step)` of contig `c` under the last E-step (a plain one is
        enough); row 0 gives 0 and the rows sum to `logliks()[c]`.  (include/smcpp_engine.h: smcpp_loglik_rows.)"""
        start, stop, step, ncols = self._selection(c, start, stop, step)
        E.check(E.lib().smcpp_loglik_rows(self._im, int(c), start, stop, step, None))              # (the checks alone)
        out = np.empty(ncols)
        E.check(E.lib().smcpp_loglik_rows(self._im, int(c), start, stop, step, E.dptr(out)))
        return out

    def loglik_positions(self, c=0, pos0=0, pos1=None, step=1):
        """`[npos]`: `l(p) = log P(o_1 .. o_p)` at the positions `range(pos0, pos1, step)` of `0 .. P_L` of contig `c` (position 0
        carries no observation: `l(0) = 0`; `l(P_L)` is `logliks()[c]`).  Inside a row the engine walks forward from the stored
        vector and splits the row's log c exactly.  (include/smcpp_engine.h: smcpp_loglik_positions.)"""
        c, pos0, pos1, step, npos = self._grid(c, pos0, pos1, step)
        E.check(E.lib().smcpp_loglik_positions(self._im, c, pos0, pos1, step, None))               # (the checks alone)
        out = np.empty(npos)
        E.check(E.lib().smcpp_loglik_positions(self._im, c, pos0, pos1, step, E.dptr(out)))
        return out

    def loglik_windows(self, c=0, window=10_000):
        """`[ceil(P_L / window)]`: the log-likelihood of contig `c` per window of `window` positions,
        `l(min((w + 1) W, P_L)) - l(w W)`; the windows sum to `logliks()[c]`.  (include/smcpp_engine.h: smcpp_loglik_windows.)"""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_loglik_windows(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty(nw.value)
        E.check(E.lib().smcpp_loglik_windows(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def score_rows(self, c=0, start=0, stop=None, step=1, parts=False):
        """`[nder, ncols]`: d loglik / d direction contributed by the caller's rows `range(start, stop, step)` of contig `c` under the
        last `save_gamma` E-step, for the `nder` derivative seeds of the parameters it ran on (a differentiable model); column 0
        holds the initial distribution's share.  `parts=True`: `[3, nder, ncols]`, the initial, emission and transition part; the
        last two sum over all columns and contigs to rows 1 + 2 and 3 of `Q_with_gradient()`'s Jacobian (row 0 weighs the initial
        part by the stored, unnormalised mass of column 0).  At most 64 hidden states; at most 256 with SMCPP_SCORE_FORM=vectors
        (`_engine.set_option`; read at every call; one-population models).
        (include/smcpp_engine.h: smcpp_score_rows.)"""
        start, stop, step, ncols = self._selection(c, start, stop, step)
        parts = 1 if parts else 0
        E.check(E.lib().smcpp_score_rows(self._im, int(c), start, stop, step, parts, None))        # (the checks alone)
        nder = E.lib().smcpp_num_derivatives(self._im)
        out = np.empty((3, nder, ncols) if parts else (nder, ncols))
        E.check(E.lib().smcpp_score_rows(self._im, int(c), start, stop, step, parts, E.dptr(out)))
        return out

    def score_windows(self, c=0, window=10_000):
        """`[nder, ceil(P_L / window)]`: the score of contig `c` per window of `window` base pairs, every row apportioned uniformly
        over its base pairs (windows as in `posterior_transition_windows`); column 0's share goes to window 0, and the windows sum
        to `score_rows(c).sum(1)`.  (include/smcpp_engine.h: smcpp_score_windows.)"""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_score_windows(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty((E.lib().smcpp_num_derivatives(self._im), nw.value))
        E.check(E.lib().smcpp_score_windows(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def score_windows_exact(self, c=0, window=10_000):
        """`[nder, ceil(P_L / window)]`: the score of contig `c` per window like `score_windows`, but exact on rows that a window
        boundary cuts: every window gets the score of the positions that lie in it (position p >= 1 in window `(p - 1) // window`),
        as if every row had been given as rows of span 1.  The vectors form only: SMCPP_SCORE_FORM=vectors (`_engine.set_option`),
        at most 256 hidden states.  (include/smcpp_engine.h: smcpp_score_windows_exact.)"""
        nw = C.c_longlong(0)
        E.check(E.lib().smcpp_score_windows_exact(self._im, int(c), int(window), C.byref(nw), None))
        out = np.empty((E.lib().smcpp_num_derivatives(self._im), nw.value))
        E.check(E.lib().smcpp_score_windows_exact(self._im, int(c), int(window), C.byref(nw), E.dptr(out)))
        return out

    def _hmm_tables(self):
        """(pi [M], T [M, M], E [K, M]) as plain float64 arrays, straight from the C getters."""
        K = E.lib().smcpp_num_keys(self._im)
        pi, T, Et = np.zeros(self.M), np.zeros((self.M, self.M)), np.zeros((K, self.M))
        E.check(E.lib().smcpp_get_pi(self._im, E.dptr(pi)))
        E.check(E.lib().smcpp_get_transition(self._im, E.dptr(T)))
        E.check(E.lib().smcpp_get_emission_probs(self._im, E.dptr(Et)))
        return pi, T, Et

    def _simulate_call(self, lengths, alphabet, quiet, seed, contig0, rep0, nreps, cap, resume):
        """One `smcpp_simulate` call: -> (x0 [nc, R], n_events [nc, R], pos [nc, R, cap], state, key, resume_out [nc, R, 3])."""
        lengths = aca(lengths, dtype=np.int64).reshape(-1)
        alphabet = aca(alphabet, dtype=np.int32).reshape(-1)
        nc, R, cap = len(lengths), int(nreps), int(cap)
        shape = (nc, max(R, 0))
        ll = C.POINTER(C.c_longlong)
        rin = None if resume is None else aca(resume, dtype=np.int64).reshape(-1)
        args = (self._im, nc, lengths.ctypes.data_as(ll), len(alphabet), E.iptr(alphabet), int(quiet), int(seed) & 0xFFFFFFFFFFFFFFFF,
                int(contig0), int(rep0), R, cap, None if rin is None else rin.ctypes.data_as(ll))
        E.check(E.lib().smcpp_simulate(*args, None, None, None, None, None, None))     # (the checks alone: nothing is allocated for a bad call)
        x0 = np.empty(shape, dtype=np.int32)
        nev = np.empty(shape, dtype=np.int64)
        pos = np.empty(shape + (cap,), dtype=np.int64)
        state = np.empty(shape + (cap,), dtype=np.int32)
        key = np.empty(shape + (cap,), dtype=np.int32)
        rout = np.empty(shape + (3,), dtype=np.int64)
        E.check(E.lib().smcpp_simulate(*args, E.iptr(x0), nev.ctypes.data_as(ll), pos.ctypes.data_as(ll), E.iptr(state), E.iptr(key),
                                       rout.ctypes.data_as(ll)))
        return x0, nev, pos, state, key, rout

    def simulate(self, lengths, n_replicates=1, seed=0, alphabet=None, quiet=None, first_replicate=0, first_contig=0, cap=None):
        """Draw `n_replicates` data sets with their hidden paths from the model this manager holds, on the device: one simulated
        contig of `lengths[c]` positions per entry (include/smcpp_engine.h: smcpp_simulate states the process, the event-driven
        walk and the random stream).  `alphabet`: key indices (rows of `keys`; default: all of them), `quiet`: the key index of
        the monomorphic observation (default: the alphabet's key with a = b = 0 and the most observed lineages).  Returns a dict:
        `x0` int32 `[contigs, replicates]`, and `pos` (int64), `state`, `key` (int32; the index INTO the alphabet) as
        `[contig][replicate]` lists of arrays over the loud positions, ascending.  Replicate `first_replicate + r` of contig
        `first_contig + c` under `seed` is the same whatever else a call asks for and whatever `cap` (events per replicate and
        device call; default: sized from the model) is."""
        from .simulate import drive
        return drive(self, lengths, n_replicates, seed, alphabet, quiet, first_replicate, first_contig, cap)

    @property
    def xisums(self):
        ret = []
        for c in range(self._num_hmms):
            x = np.zeros((self.M, self.M))
            E.check(E.lib().smcpp_get_xisum(self._im, c, E.dptr(x)))
            ret.append(x)
        return ret

    @property
    def pi(self):
        out = np.zeros(self.M)
        E.check(E.lib().smcpp_get_pi(self._im, E.dptr(out)))
        return out

    @property
    def transition(self):
        out = np.zeros((self.M, self.M))
        E.check(E.lib().smcpp_get_transition(self._im, E.dptr(out)))
        return out

    def Q(self, separate=False):
        """``_smcpp.pyx:277-301`` (values; derivative seeds are the M-step path, not built yet)."""
        q = np.zeros(4)
        E.check(E.lib().smcpp_q(self._im, E.dptr(q), None))
        if separate:
            return list(q)
        return float(q.sum())

    def Q_with_gradient(self):
        """The four Q terms and their forward-mode Jacobian [4 x nder] with respect to the derivative seeds handed
        to `set_params` (what `Q()` returns inside an ad number in the reference, `_smcpp.pyx:277-301`)."""
        q = np.zeros(4)
        nder = E.lib().smcpp_num_derivatives(self._im)
        jac = np.zeros((4, max(nder, 1)))
        E.check(E.lib().smcpp_q(self._im, E.dptr(q), E.dptr(jac)))
        return q, jac[:, :nder]

    def loglik(self):
        """``_smcpp.pyx:303-308``: sum over contigs."""
        return float(sum(self.logliks()))

    def logliks(self):
        out = np.zeros(self._num_hmms)
        E.check(E.lib().smcpp_loglik(self._im, E.dptr(out)))
        return out

    # ---- engine extensions ----
    def set_raw(self, pi, T, keys, Etab):
        pi = aca(pi, dtype=np.float64); T = aca(T, dtype=np.float64)
        keys = aca(keys, dtype=np.int32); Etab = aca(Etab, dtype=np.float64)
        E.check(E.lib().smcpp_set_raw(self._im, E.dptr(pi), E.dptr(T), len(keys), E.iptr(keys), E.dptr(Etab)))

    def set_chunking(self, rows_per_chunk=0, eps_alpha=0.0, eps_beta=0.0):
        E.check(E.lib().smcpp_set_chunking(self._im, int(rows_per_chunk), float(eps_alpha), float(eps_beta)))

    def set_warm_start(self, on=True):
        """Extension: reuse the previous E-step's converged chunk-boundary vectors as start vectors (see the header)."""
        E.check(E.lib().smcpp_set_warm_start(self._im, int(bool(on))))

    def set_prep_mode(self, host=False):
        """Where the cold preparation runs: device kernels (default) or the host routines (see the header)."""
        E.check(E.lib().smcpp_set_prep_mode(self._im, int(bool(host))))

    def device_index(self):
        """The HIP device this manager lives on."""
        return int(E.lib().smcpp_device(self._im))

    @property
    def debug(self):
        """`InferenceManager::debug` (`_smcpp.pxd:53`): declared by the reference, read by nothing in its C++."""
        return bool(E.lib().smcpp_get_debug(self._im))

    @debug.setter
    def debug(self, on):
        E.check(E.lib().smcpp_set_debug(self._im, int(bool(on))))

    def chain_mode(self):
        """Chain kernel family in use: 0 generic, 1 LDS-resident, 2 cooperative, 3 streamed operands, 4 lock-step (MFMA),
        5 scans over the semiseparable structure of the transition matrix (the other families are its fallback)."""
        return int(E.lib().smcpp_chain_mode(self._im))

    def chunks(self, backward=False):
        """The scan chains' chunk list of one direction as the current plan cut it (`smcpp_debug_chunks`): an int array [n, 5] of
        (contig, r0, r1, h0, h1); the chunk owns the engine's rows r0+1 .. r1, h0 / h1 bound the halo it enters through."""
        n = int(E.lib().smcpp_debug_chunks(self._im, int(bool(backward)), 0, None))
        out = np.zeros((max(n, 0), 5), dtype=np.int32)
        if n > 0:
            E.lib().smcpp_debug_chunks(self._im, int(bool(backward)), n, E.iptr(out))
        return out

    def describe(self):
        """The engine's environment switches and the plan this manager resolved (chain family, chunks, history passes, whether the
        stored passes of the last E-step ran their scans in float): `smcpp_describe`."""
        return E.describe(self._im)

    def last_timing(self):
        t = np.zeros(9)
        E.check(E.lib().smcpp_last_timing(self._im, E.dptr(t)))
        return dict(zip(["host_prep_ms", "chains_wall_ms", "forward_ms", "backward_ms", "stats_ms", "finalize_ms",
                         "device_total_ms", "fwd_passes", "bwd_passes"], t))

    def last_host_timing(self):
        t = np.zeros(4)
        E.check(E.lib().smcpp_last_host_timing(self._im, E.dptr(t)))
        return dict(zip(["cold_prep_ms", "eigensystems_ms", "staging_ms", "host_total_ms"], t))

    def stream(self):
        return E.lib().smcpp_stream(self._im)

    def set_global_keys(self, gkeys):
        gkeys = aca(gkeys, dtype=np.int32)
        E.check(E.lib().smcpp_set_global_keys(self._im, len(gkeys), E.iptr(gkeys)))

    def pack_stats(self):
        n = C.c_long(0)
        E.check(E.lib().smcpp_pack_stats(self._im, None, C.byref(n), 0))
        buf = np.zeros(n.value)
        E.check(E.lib().smcpp_pack_stats(self._im, E.dptr(buf), C.byref(n), 0))
        return buf

    def stats_len(self):
        n = C.c_long(0)
        E.check(E.lib().smcpp_pack_stats(self._im, None, C.byref(n), 0))
        return int(n.value)

    def pack_stats_device(self, device_ptr, sync=True):
        """Write the packed statistics into a device buffer of `stats_len()` doubles (e.g. `tensor.data_ptr()` of the
        fp64 tensor that is all-reduced over RCCL); returns after the kernel has finished, or - `sync=False` - right after
        the enqueue on the engine's stream (`stream()`), for a consumer that is ordered on that stream."""
        n = C.c_long(0)
        E.check(E.lib().smcpp_pack_stats(self._im, C.cast(C.c_void_p(int(device_ptr)), C.POINTER(C.c_double)),
                                         C.byref(n), 1 if sync else 2))
        return int(n.value)

    def unpack_stats_device(self, device_ptr, n):
        E.check(E.lib().smcpp_unpack_stats(self._im, C.cast(C.c_void_p(int(device_ptr)), C.POINTER(C.c_double)),
                                           int(n), 1))

    def unpack_stats(self, buf):
        buf = aca(buf, dtype=np.float64)
        E.check(E.lib().smcpp_unpack_stats(self._im, E.dptr(buf), len(buf), 0))

    # ---- the exchange issued by the engine itself through RCCL's C API (include/smcpp_engine.h: smcpp_rccl_*) ----
    @staticmethod
    def rccl_unique_id(libpath=None):
        out = C.create_string_buffer(128)
        E.check(E.lib().smcpp_rccl_unique_id((libpath or "").encode(), out))
        return out.raw

    def rccl_init(self, unique_id, rank, world, libpath=None):
        E.check(E.lib().smcpp_rccl_init(self._im, (libpath or "").encode(), bytes(unique_id), int(rank), int(world)))

    def rccl_exchange(self):
        """pack -> ncclAllReduce -> the reduced log-likelihood sum, all on the engine's stream; returns that sum"""
        v = np.zeros(1)
        E.check(E.lib().smcpp_rccl_exchange(self._im, E.dptr(v)))
        return float(v[0])

    def rccl_unpack(self):
        E.check(E.lib().smcpp_rccl_unpack(self._im))

    def rccl_fetch(self):
        out = np.zeros(self.stats_len())
        E.check(E.lib().smcpp_rccl_fetch(self._im, E.dptr(out), len(out)))
        return out


class PyOnePopInferenceManager(_PyInferenceManager):
    """``PyOnePopInferenceManager(n, observations, hidden_states, im_id, polarization_error)`` (_smcpp.pyx:310-332)."""

    def __init__(self, n, observations, hidden_states, im_id, polarization_error, device=-1):
        self._my_init(observations, hidden_states, im_id)
        im = C.c_void_p()
        E.check(E.lib().smcpp_create_onepop(int(n), self._num_hmms, E.iptr(self._Ls), self._ptrs(), len(self._hs),
                                            E.dptr(self._hs), C.c_double(polarization_error), int(device),
                                            C.byref(im)))
        self._im = im
        self._n = int(n)
        # sensible defaults (_smcpp.pyx:318-320)
        self.alpha = 1
        self.theta = 1e-4
        self.rho = 1e-4

    @property
    def pid(self):
        assert len(self._im_id) == 1
        return self._im_id[0]

    def update(self, message, *args, **kwargs):
        m = self._model.for_pop(self.pid) if hasattr(self._model, "for_pop") else self._model
        a = aca(np.asarray(m.stepwise_values(), dtype=np.float64))
        s = aca(np.asarray(m.s, dtype=np.float64))
        assert np.all(a > 0) and len(a) > 0
        seeds = m.derivative_seeds() if hasattr(m, "derivative_seeds") else None
        if seeds is None:
            E.check(E.lib().smcpp_set_params(self._im, len(a), E.dptr(a), None, 0, E.dptr(s)))
        else:
            da = aca(np.asarray(seeds, dtype=np.float64))
            E.check(E.lib().smcpp_set_params(self._im, len(a), E.dptr(a), E.dptr(da), da.shape[1], E.dptr(s)))


class PyTwoPopInferenceManager(_PyInferenceManager):
    """``PyTwoPopInferenceManager(n1, n2, a1, a2, observations, hidden_states, im_id, polarization_error)``
    (_smcpp.pyx:334-368).  `im.model = TwoPopulationModel(...)` feeds the distinguished model, both populations and
    the split to the engine's JointCSFS preparation; `set_raw` remains available."""

    def __init__(self, n1, n2, a1, a2, observations, hidden_states, im_id, polarization_error, device=-1):
        assert a1 + a2 == 2
        assert a1 in [1, 2]
        assert a2 in [0, 1]
        self._a1 = a1
        self._my_init(observations, hidden_states, im_id)
        im = C.c_void_p()
        E.check(E.lib().smcpp_create_twopop(int(n1), int(n2), int(a1), int(a2), self._num_hmms, E.iptr(self._Ls),
                                            self._ptrs(), len(self._hs), E.dptr(self._hs),
                                            C.c_double(polarization_error), int(device), C.byref(im)))
        self._im = im
        self.alpha = 1
        self.theta = 1e-4
        self.rho = 1e-4

    def update(self, message, *args, **kwargs):
        m = self._model
        pids = self._im_id
        dist = None if self._a1 == 1 else pids[0]              # both lineages apart -> special distinguished model
        dm = m.for_pop(dist)
        ms = [m.for_pop(p) for p in pids]
        arrs, seeds = [], []
        for q in (dm, ms[0], ms[1]):
            arrs.append((aca(np.asarray(q.stepwise_values(), dtype=np.float64)), aca(np.asarray(q.s, dtype=np.float64))))
            sd = q.derivative_seeds() if hasattr(q, "derivative_seeds") else None
            seeds.append(None if sd is None else aca(np.asarray(sd, dtype=np.float64)))
        nder = max([0] + [x.shape[1] for x in seeds if x is not None])
        ptr = lambda x: None if x is None else E.dptr(x)       # noqa: E731
        (ad, sd_), (a1, s1), (a2, s2) = arrs
        E.check(E.lib().smcpp_set_params_twopop(self._im, len(ad), E.dptr(ad), E.dptr(sd_), ptr(seeds[0]), len(a1),
                                                E.dptr(a1), E.dptr(s1), ptr(seeds[1]), len(a2), E.dptr(a2),
                                                E.dptr(s2), ptr(seeds[2]), C.c_double(float(m.split)), int(nder)))


class PyRateFunction:
    """Mirror of `PyRateFunction` (smcpp/_smcpp.pyx:370-399): cumulative hazard of a piecewise-constant model.
    Values are plain floats; `R_jac` / `average_coal_times_jac` additionally return the Jacobians with respect to the
    model's `derivative_seeds()` (the `.d()` parts of the reference's ad numbers)."""

    def __init__(self, model, hs):
        self._model = model
        self._hs = np.asarray(list(hs), dtype=np.float64)
        self._a = np.asarray([float(x) for x in model.stepwise_values()], dtype=np.float64)
        self._s = np.asarray(model.s, dtype=np.float64)

    def R(self, t):
        assert np.isfinite(t)
        return float(E.host_rate_function(self._a, self._s, [t])[0])

    def average_coal_times(self):
        if len(self._hs) < 2:
            return []
        return list(E.host_rate_function(self._a, self._s, [0.0], self._hs)[1])

    def _seeds(self):
        da = getattr(self._model, "derivative_seeds", lambda: None)()
        return np.eye(len(self._a)) if da is None else da

    def R_jac(self, t):
        R, dR = E.host_rate_function_jac(self._a, self._seeds(), self._s, [t])[:2]
        return float(R[0]), dR[0]

    def average_coal_times_jac(self):
        _, _, ct, dct = E.host_rate_function_jac(self._a, self._seeds(), self._s, [0.0], self._hs)
        return ct, dct

    def random_coal_times(self, t1, t2, K):
        seeds = np.random.randint(0, np.iinfo(np.int64).max, size=K, dtype=np.int64).astype(np.uint64)
        t, R = E.host_random_coal_times(self._a, self._s, t1, t2, seeds)
        return [[float(x), float(y)] for x, y in zip(t, R)]


def raw_sfs(model, n, t1, t2, below_only=False, jac=False):
    """Mirror of `raw_sfs` (smcpp/_smcpp.pyx:401-412): conditioned SFS [3, n+1] of the single hidden state [t1, t2)."""
    a = np.asarray([float(x) for x in model.stepwise_values()], dtype=np.float64)
    s = np.asarray(model.s, dtype=np.float64)
    if not jac:
        return E.host_raw_sfs(n, a, s, t1, t2, below_only)
    da = getattr(model, "derivative_seeds", lambda: None)()
    return E.host_raw_sfs(n, a, s, t1, t2, below_only, da=np.eye(len(a)) if da is None else da)


def joint_csfs(n1, n2, a1, a2, model, hidden_states, K=10):
    """Mirror of `joint_csfs` (smcpp/_smcpp.pyx:416-437, "used for testing purposes only"): list over hidden states of
    the joint conditioned SFS [(a1+1), (n1+1), (a2+1), (n2+1)] of a `TwoPopulationModel`."""
    assert (a1 == 2 and a2 == 0) or (a1 == a2 == 1)
    p1, p2 = model.for_pop(model.pids[0]), model.for_pop(model.pids[1])
    J = E.host_joint_csfs(n1, n2, a1, a2, np.asarray(list(hidden_states), dtype=np.float64),
                          (p1.stepwise_values(), p1.s), (p2.stepwise_values(), p2.s), float(model.split), K)
    return [J[m] for m in range(J.shape[0])]
