"""The `smc++ posterior` product (reference `smcpp/commands/posterior.py:48-111` and
`smcpp/estimation_tools.py:170-197`): balanced hidden states, posterior decoding matrix and its argmax path."""
from __future__ import annotations

import numpy as np
import scipy.optimize

from . import _engine, _smcpp
from .model import PiecewiseModel


def balance_hidden_states(model, M):
    """Break points `[0, b_1, ..., b_{M-1}, inf)` (coalescent units) such that the probability of coalescing in each
    of the M intervals is equal under the model: `exp(-R(b_m)) = (M - m) / M`, root-found with Brent's method exactly
    as `estimation_tools.py:170-197` does (which is called with M+1 and returns generations = 2 N0 x these)."""
    a = np.asarray(model.stepwise_values(), dtype=float)
    s = np.asarray(model.s, dtype=float)
    ret = [0.0]
    for m in range(1, M):
        def f(t):
            return float(np.exp(-_engine.host_rate_function(a, s, t)[0]) - (M - m) / M)
        lo = hi = ret[-1]
        while f(lo) * f(hi) >= 0:
            hi = 2 * (hi + 1)
        ret.append(scipy.optimize.brentq(f, lo, hi))
    ret.append(np.inf)
    return np.array(ret)


def _decode_setup(model, contigs, M, n, theta, rho, alpha, polarization_error, hidden_states, device, a, start, end, thinning,
                  save_gamma=True):
    """What `posterior`, `posterior_products` and `evidence.loglik_track` share: the hidden states, the rows handed to the manager
    (missing row in front, `start` / `end` / `thinning` applied) and a one- or two-population manager after its E-step - a
    `save_gamma` one unless `save_gamma=False`.  -> `(hidden_states, obs, im)`."""
    twopop = not np.isscalar(n) and len(n) == 2
    dist = model.model1 if twopop else model          # `distinguished_model` (smcpp/model.py:70-72,275-277)
    hs = balance_hidden_states(dist, M) if hidden_states is None else np.asarray(hidden_states, dtype=float)
    obs = []
    for c in contigs:
        d = np.asarray(c, dtype=np.int32)
        if start is not None or end is not None:
            pos = np.cumsum(d[:, 0])
            lb = 0 if start is None else start
            ub = pos[-1] if end is None else end
            d = d[(pos >= lb) & (pos <= ub)]
        miss = np.zeros((1, d.shape[1]), dtype=np.int32)
        miss[0, 0] = 1
        miss[0, 1::3] = -1
        obs.append(np.ascontiguousarray(np.vstack([miss, d])))
    if thinning > 1:
        from .data import thin_data
        obs = [np.ascontiguousarray(thin_data(o, thinning, 0)) for o in obs]
    if twopop:
        assert a is not None and len(a) == 2 and all(o.shape[1] == 7 for o in obs)
        pids = tuple(getattr(model, "pids", ("pop1", "pop2")))
        im = _smcpp.PyTwoPopInferenceManager(int(n[0]), int(n[1]), int(a[0]), int(a[1]), obs, hs, pids, polarization_error,
                                             device=device)
    else:
        nn = int(n if np.isscalar(n) else n[0])
        im = _smcpp.PyOnePopInferenceManager(nn, obs, hs, (getattr(model, "pid", "pop1"),), polarization_error, device=device)
    im.model = model
    im.theta = theta
    im.rho = rho
    im.alpha = alpha
    im.save_gamma = bool(save_gamma)
    im.E_step()
    return hs, obs, im


def posterior(model, contigs, M, n, theta, rho, alpha=1.0, polarization_error=0.5, hidden_states=None, device=-1, a=None,
              start=None, end=None, thinning=1, return_manager=False):
    """Posterior decoding of each contig.  Returns `(hidden_states, gammas, sites, paths)`:
    `gammas[c]` is `[M, L+1]` with columns normalised to one (`posterior.py:102-106`), `sites[c]` the span column of the
    rows handed to the manager (missing row included) exactly as the reference stores it under `<file>_sites`
    (`posterior.py:109`: `obs[:, 0]`, one entry per row; cumulative positions are `np.cumsum` of it), `paths[c]` the
    argmax state per column computed on the device.  `return_manager=True` appends the inference manager (its device buffers
    stay allocated for as long as the caller keeps it) - nothing is kept otherwise.
    A missing row is prepended to every contig as the reference does (`posterior.py:83`); `start` / `end` keep the rows whose
    cumulative position lies in [start, end] (`posterior.py:76-82`: "only approximately picked out"), `thinning` > 1 thins every
    contig as `thin_dataset` does (`posterior.py:85-87`).
    TWO populations (`posterior.py:88-100`): `n = (n1, n2)` undistinguished and `a = (a1, a2)` distinguished lineages per
    population, rows of 7 columns, `model` a `TwoPopulationModel`; the hidden states are balanced with respect to the
    DISTINGUISHED lineages' model (`m.distinguished_model`, `posterior.py:60-62`)."""
    hs, obs, im = _decode_setup(model, contigs, M, n, theta, rho, alpha, polarization_error, hidden_states, device, a, start, end,
                                thinning)
    gammas, sites, paths = [], [], []
    for c, g in enumerate(im.gammas):
        g = g / g.sum(axis=0, keepdims=True)
        gammas.append(g)
        sites.append(obs[c][:, 0].copy())
        paths.append(im.gamma_argmax(c))
    if return_manager:
        return hs, gammas, sites, paths, im
    return hs, gammas, sites, paths


def average_coal_times(model, hidden_states):
    """E[T | hs_m <= T < hs_{m+1}] under `model` for every hidden state, coalescent units (`PyRateFunction.average_coal_times`,
    `_smcpp.pyx:370-389`).  Finite in the last, unbounded state as well."""
    a = np.asarray(model.stepwise_values(), dtype=float)
    s = np.asarray(model.s, dtype=float)
    _, ct = _engine.host_rate_function(a, s, [0.0], hs=np.asarray(hidden_states, dtype=float))
    return ct


def posterior_products(model, contigs, M, n, theta, rho, alpha=1.0, polarization_error=0.5, hidden_states=None, device=-1, a=None,
                       start=None, end=None, thinning=1, window=None, quantiles=(0.025, 0.5, 0.975), return_manager=False, transitions=False,
                       paths=0, seed=0, grid=None, exact_windows=False, loglik_windows=False):
    """What a posterior decoding is reduced to, computed on the device without ever fetching the `[M, L+1]` matrix (arguments and
    set-up as `posterior`: hidden states, the prepended missing row, `start` / `end` / `thinning`, one or two populations).
    Returns `(hidden_states, products)`; `products[c]` is a dict for contig c:
      `sites`       the span column of the rows handed to the manager, as `posterior` returns it;
      `path`        argmax state per column, `[L+1]` int32 (`posterior`'s `paths[c]`);
      `mean_tmrca`  posterior mean of the coalescence time per column, `[L+1]`, coalescent units: `sum_m w_m p[m, l]` with `w_m`
                    the average coalescence time of hidden state m under the distinguished model (`average_coal_times`);
      `qstate`      `[len(quantiles), L+1]` int32: the first state at which the cumulative posterior reaches each level (a credible
                    band in units of hidden states; at most 8 levels);
      `windows`     only with `window=W` base pairs: `[M, ceil(P / W)]`, the posterior averaged over windows of W base pairs, P the
                    total span of the rows handed to the manager.  Position 0 of the window axis is the PREPENDED MISSING ROW (span
                    1), not the first base pair of the caller's contig: window w covers the caller's base pairs [w W - 1, (w + 1) W - 1).
    With `transitions=True` (one-population or two-population models alike) each dict gains
      `transitions`         `[3, L+1]`: per column the expected number of the row's positions at which the hidden state stays, moves
                            up (to an older state) or moves down; the three sum to the row's span, column 0 holds zeros
                            (`im.posterior_transitions`);
      `transition_windows`  only with `window=W`: `[3, ceil(P / W)]`, the same counts per window of W base pairs, a row
                            apportioned uniformly over its base pairs (windows as for `windows`).
    With `paths=K > 0` each dict gains joint draws of the hidden-state path from the posterior, reduced per column
    (`im.posterior_sample_rows(c, K, seed)`; path k of contig c under `seed` is the same whatever K is):
      `path_state`  `[K, L+1]` int32: the state of sampled path k at the row's last position (column 0: at position 0);
      `path_up`, `path_down`  `[K, L+1]` int32: the number of the row's positions at which path k moves to a higher (older) / lower
                    state; `(path_up + path_down).sum(axis=1)` is the number of breakpoints of path k.
    With `grid=step` (positions `0 .. P`: position 0 is column 0, row l covers positions `P_{l-1} + 1 .. P_l`) each dict gains the
    posterior of single positions, summarised on the grid `range(0, P + 1, step)` (`im.posterior_position_summary`):
      `grid_positions`   `[npos]` int64, the positions;
      `grid_path`, `grid_mean_tmrca`, `grid_qstate`   as `path`, `mean_tmrca`, `qstate`, per grid position instead of per column.
    With `exact_windows=True` (and `window=W`) `windows` comes from `im.posterior_windows_exact`: rows that a window boundary cuts
    are walked position by position instead of being apportioned uniformly.
    With `loglik_windows=True` (and `window=W`) each dict gains
      `loglik_windows`   `[ceil(P / W)]`: the contig's log-likelihood per window of W positions (`im.loglik_windows`; windows as
                         for `windows`), summing to the contig's log-likelihood.
    `return_manager=True` appends the inference manager."""
    hs, obs, im = _decode_setup(model, contigs, M, n, theta, rho, alpha, polarization_error, hidden_states, device, a, start, end,
                                thinning)
    twopop = not np.isscalar(n) and len(n) == 2
    w = average_coal_times(model.model1 if twopop else model, hs)
    products = []
    for c in range(len(obs)):
        sm = im.posterior_summary(c, weights=w, quantiles=quantiles)
        prod = {"sites": obs[c][:, 0].copy(), "path": sm["argmax"], "mean_tmrca": sm["mean"], "qstate": sm["qstate"]}
        if window is not None:
            prod["windows"] = im.posterior_windows_exact(c, window) if exact_windows else im.posterior_windows(c, window)
            if loglik_windows:
                prod["loglik_windows"] = im.loglik_windows(c, window)
        if transitions:
            tr = im.posterior_transitions(c)
            prod["transitions"] = np.stack([tr["stay"], tr["up"], tr["down"]])
            if window is not None:
                prod["transition_windows"] = im.posterior_transition_windows(c, window)
        if paths > 0:
            pr = im.posterior_sample_rows(c, n_paths=paths, seed=seed)
            prod["path_state"], prod["path_up"], prod["path_down"] = pr["state"], pr["up"], pr["down"]
        if grid is not None:
            total = int(obs[c][:, 0].sum(dtype=np.int64))
            gs = im.posterior_position_summary(c, weights=w, quantiles=quantiles, pos0=0, pos1=total + 1, step=int(grid))
            prod["grid_positions"] = np.arange(0, total + 1, int(grid), dtype=np.int64)
            prod["grid_path"], prod["grid_mean_tmrca"], prod["grid_qstate"] = gs["argmax"], gs["mean"], gs["qstate"]
        products.append(prod)
    if return_manager:
        return hs, products, im
    return hs, products


def save_npz(path, hs, gammas, sites, names):
    """`.npz` layout of `smc++ posterior` (README.rst:348-372): `hidden_states`, `<file>`, `<file>_sites`."""
    out = {"hidden_states": hs}
    for nm, g, s in zip(names, gammas, sites):
        out[nm] = g
        out[nm + "_sites"] = s
    np.savez_compressed(path, **out)


def save_products_npz(path, hs, products, names):
    """`.npz` of `posterior_products`: `hidden_states` and per file `<file>_sites`, `<file>_path`, `<file>_mean_tmrca`,
    `<file>_qstate` and, where they were asked for, `<file>_windows`, `<file>_transitions`, `<file>_transition_windows`,
    `<file>_path_state`, `<file>_path_up`, `<file>_path_down`, `<file>_grid_positions`, `<file>_grid_path`, `<file>_grid_mean_tmrca`,
    `<file>_grid_qstate`, `<file>_loglik_windows`."""
    out = {"hidden_states": hs}
    for nm, prod in zip(names, products):
        for key in ("sites", "path", "mean_tmrca", "qstate", "windows", "transitions", "transition_windows", "path_state", "path_up",
                    "path_down", "grid_positions", "grid_path", "grid_mean_tmrca", "grid_qstate", "loglik_windows"):
            if key in prod:
                out[f"{nm}_{key}"] = prod[key]
    np.savez_compressed(path, **out)
