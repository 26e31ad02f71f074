"""The evidence side of a fit, below the contig level: the log-likelihood per window of positions (`im.loglik_windows`,
include/smcpp_engine.h: smcpp_loglik_windows), the comparison of two fits of the same data with a block jackknife, and surprisal
per base pair.  The reference reports one number per contig (`HMM::loglik`, hmm.h); its `cv` scores whole contigs for that reason.
And the derivative of the evidence, below the contig level as well: the score per window (`im.score_windows`, smcpp_score_windows),
the block-wise outer product of scores as an information estimate, and the standard errors it gives without a refit."""
from __future__ import annotations

import numpy as np

from .posterior import _decode_setup


def loglik_track(model, contigs, M, n, theta, rho, window, alpha=1.0, polarization_error=0.5, a=None, device=-1, return_manager=False):
    """The log-likelihood of every contig under `model`, per window of `window` positions.  `M` is the number of hidden states
    (balanced under the model, as `posterior_products` does) or the array of hidden-state break points itself - pass the same
    array for two models whose tracks are to be compared.  One manager, set up as `posterior_products` sets it up (one or two
    populations, the missing row in front of every contig: window w covers the caller's base pairs [w W - 1, (w + 1) W - 1)), and
    ONE PLAIN E-step: the track is a forward-only product and needs no `save_gamma`.
    Returns `(hidden_states, track)`, `track[c]` the `[ceil(P_c / window)]` window values of contig c; they sum to the contig's
    log-likelihood.  `return_manager=True` appends the inference manager."""
    hidden_states = None if np.isscalar(M) else np.asarray(M, dtype=float)
    nstates = int(M) if hidden_states is None else len(hidden_states) - 1
    hs, obs, im = _decode_setup(model, contigs, nstates, n, theta, rho, alpha, polarization_error, hidden_states, device, a, None, None, 1,
                                save_gamma=False)
    track = [im.loglik_windows(c, int(window)) for c in range(len(obs))]
    if return_manager:
        return hs, track, im
    return hs, track


def compare_tracks(track_a, track_b, block=1):
    """Two window tracks of the SAME data and window under two models -> dict of
      `delta`   D = sum_b d_b, the difference of the log-likelihoods (a minus b);
      `se`      sqrt(B / (B - 1) sum_b (d_b - D / B)^2): the delete-one-block jackknife standard error of a sum;
      `z`       D / se;
      `blocks`  d_b, the difference per block.
    A block is `block` consecutive windows of one contig (the last block of a contig may hold fewer); neighbouring positions are
    dependent, so the blocks have to be long against the correlation length of the data for `se` to mean anything.  Refuses tracks
    of different shapes and fewer than two blocks."""
    block = int(block)
    if block < 1:
        raise ValueError("compare_tracks: block < 1")
    if len(track_a) != len(track_b):
        raise ValueError(f"compare_tracks: {len(track_a)} contigs against {len(track_b)}")
    d = []
    for c, (ta, tb) in enumerate(zip(track_a, track_b)):
        ta, tb = np.asarray(ta, dtype=np.float64), np.asarray(tb, dtype=np.float64)
        if ta.ndim != 1 or ta.shape != tb.shape:
            raise ValueError(f"compare_tracks: contig {c}: tracks of shapes {ta.shape} and {tb.shape}")
        if len(ta):
            d.append(np.add.reduceat(ta - tb, np.arange(0, len(ta), block)))
    d = np.concatenate(d) if d else np.zeros(0)
    B = len(d)
    if B < 2:
        raise ValueError(f"compare_tracks: {B} block(s): the jackknife needs at least two (use a smaller block)")
    D = float(d.sum())
    se = float(np.sqrt(B / (B - 1.0) * np.sum((d - D / B) ** 2)))
    return {"delta": D, "se": se, "z": D / se if se > 0.0 else float(np.copysign(np.inf, D)) if D != 0.0 else 0.0, "blocks": d}


def score_track(model, contigs, M, n, theta, rho, window, alpha=1.0, polarization_error=0.5, a=None, device=-1, return_manager=False,
                seeds=None, form=None, exact=False):
    """The score of every contig under `model`, per window of `window` base pairs: d loglik / d direction, window by window
    (`im.score_windows`, include/smcpp_engine.h: smcpp_score_windows).  Built like `loglik_track` - `M` the number of hidden states
    (at most 64; at most 256 with `form="vectors"`) or their break points, one manager, the missing row in front of every contig - but on ONE `save_gamma` E-step, and
    the model has to carry derivative seeds: `PiecewiseModel.differentiable = True` (one direction per piece), an
    `AdPiecewiseModel`'s `dlist`, or `seeds`, a `[pieces, nder]` array d a_k / d x_j for a one-population model (it replaces the
    model's own).  Returns `(hidden_states, track)`, `track[c]` the `[nder, ceil(P_c / window)]` window values of contig c; summed
    over windows and contigs they are the gradient of the log-likelihood in those directions.  `return_manager=True` appends the
    inference manager.  `form`: "matrix" or "vectors", the form of the engine's row walk (SMCPP_SCORE_FORM, set around this
    function's own score calls and put back afterwards; None: whatever the environment says, the matrix form when it says nothing).
    The vectors form serves one-population models up to 256 hidden states; a manager that is kept answers later calls in the form
    the switch names then.  `exact=True`: `im.score_windows_exact` instead - a row that a window boundary cuts gives every window
    the score of the positions that lie in it, not an even share (what un-binned data need, where one row spans many windows).  It
    exists in the vectors form only: `form=None` then means "vectors", and `form="matrix"` is refused."""
    if form not in (None, "matrix", "vectors"):
        raise ValueError(f"score_track: form {form!r} (expected None, 'matrix' or 'vectors')")
    if exact and form == "matrix":
        raise ValueError("score_track: exact windows exist in the vectors form only (form='vectors', or leave form unset)")
    if exact and form is None:
        form = "vectors"
    hidden_states = None if np.isscalar(M) else np.asarray(M, dtype=float)
    nstates = int(M) if hidden_states is None else len(hidden_states) - 1
    if seeds is not None:
        if not np.isscalar(n) and len(n) == 2:
            raise ValueError("score_track: explicit seeds go with a one-population model (a TwoPopulationModel carries its own)")
        from .model import PiecewiseModel
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        vals = np.asarray([float(x) for x in model.stepwise_values()], dtype=np.float64)
        if seeds.ndim != 2 or seeds.shape[0] != len(vals) or seeds.shape[1] < 1:
            raise ValueError(f"score_track: seeds of shape {seeds.shape} for {len(vals)} pieces (expected [pieces, nder >= 1])")
        model = PiecewiseModel(vals, model.s, getattr(model, "N0", 1e4), getattr(model, "pid", None))
        model.derivative_seeds = lambda: seeds
    hs, obs, im = _decode_setup(model, contigs, nstates, n, theta, rho, alpha, polarization_error, hidden_states, device, a, None, None, 1,
                                save_gamma=True)
    windows = (lambda c: im.score_windows_exact(c, int(window))) if exact else (lambda c: im.score_windows(c, int(window)))
    if form is None:
        track = [windows(c) for c in range(len(obs))]
    else:
        import os
        from . import _engine
        before = os.environ.get("SMCPP_SCORE_FORM")
        _engine.set_option("SMCPP_SCORE_FORM", form)
        try:
            track = [windows(c) for c in range(len(obs))]
        finally:
            _engine.set_option("SMCPP_SCORE_FORM", before)
    if return_manager:
        return hs, track, im
    return hs, track


def information(tracks, block=1):
    """Score tracks (`score_track`: per contig `[nder, n_windows]`) -> dict of
      `score`   sum_b s_b `[nder]`, the gradient of the log-likelihood;
      `J`       B / (B - 1) sum_b (s_b - sbar)(s_b - sbar)^T `[nder, nder]`, sbar the mean of the s_b: the outer product of gradients
                (OPG / BHHH) estimate of the information the data hold about the directions;
      `blocks`  s_b `[B, nder]`, the score per block.
    A block is `block` consecutive windows of one contig, formed exactly as `compare_tracks` forms them (the last block of a contig
    may hold fewer).  Refuses fewer than two blocks, as `compare_tracks` does.
    What this assumes, plainly: J estimates the Fisher information only AT A STATIONARY POINT OF THE UNPENALISED LOG-LIKELIHOOD
    (`score` near zero on the scale of sqrt(diag J)); neighbouring positions are dependent, so blocks must be long against the
    correlation length of the data; and a fit that was regularised is not at such a point - there the estimate is not valid and `parametric_bootstrap` remains
    the tool."""
    block = int(block)
    if block < 1:
        raise ValueError("information: block < 1")
    s, nder = [], None
    for c, t in enumerate(tracks):
        t = np.asarray(t, dtype=np.float64)
        if t.ndim != 2 or (nder is not None and t.shape[0] != nder):
            raise ValueError(f"information: contig {c}: a track of shape {t.shape}" + ("" if nder is None else f" next to {nder} directions"))
        nder = t.shape[0]
        if t.shape[1]:
            s.append(np.add.reduceat(t, np.arange(0, t.shape[1], block), axis=1).T)
    s = np.concatenate(s, axis=0) if s else np.zeros((0, nder or 0))
    B = len(s)
    if B < 2:
        raise ValueError(f"information: {B} block(s): the estimate needs at least two (use a smaller block)")
    dev = s - s.mean(axis=0, keepdims=True)
    return {"score": s.sum(axis=0), "J": B / (B - 1.0) * (dev.T @ dev), "blocks": s}


def covariance(info, rcond=1e-10):
    """`information`'s dict -> dict of `cov` = pinv(J) (singular values below `rcond` times the largest are dropped: a direction
    the data say nothing about gets variance 0 there, not infinity - look at J's spectrum) and `se` = sqrt(diag cov).  The
    assumptions are `information`'s: the OPG estimate, at a stationary point of the unpenalised log-likelihood, with blocks long
    against the correlation length; it does not replace `parametric_bootstrap` for a regularised fit."""
    cov = np.linalg.pinv(np.asarray(info["J"], dtype=np.float64), rcond=rcond, hermitian=True)
    return {"cov": cov, "se": np.sqrt(np.clip(np.diag(cov), 0.0, None))}


def surprisal(track, window, lengths):
    """-log-likelihood per base pair: per contig `-track[c] / width`, the width of a window being `window` except for the last
    window of a contig, which is divided by its true width `lengths[c] - (n_windows - 1) window` (`lengths[c]` = the positions the
    track of contig c covers, P_c)."""
    window = int(window)
    out = []
    for c, (t, N) in enumerate(zip(track, lengths)):
        t = np.asarray(t, dtype=np.float64)
        N = int(N)
        if len(t) != -(-N // window):
            raise ValueError(f"surprisal: contig {c}: {len(t)} windows of {window} do not cover {N} positions")
        width = np.full(len(t), float(window))
        if len(t):
            width[-1] = N - (len(t) - 1) * window
        out.append(-t / width)
    return out
