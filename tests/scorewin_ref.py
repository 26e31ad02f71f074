"""Oracle of the score track's EXACT windows (smcpp_score_windows_exact): tests/scoreref.py's position-level pass on the rows
EXPANDED into rows of span 1, added up by window.  Position p >= 1 of a contig lies in window (p - 1) // W; column 0 (the initial
part) goes to window 0.  No GPU, nothing of the kernel: no item table, no blocks, no flush.

The bar scale is tests/test_gpu_score_track.oracle's B[l, d] = s_l (max |G_T,d| + max_j |G_E,d[k_l](j)|), split by POSITIONS instead
of by rows: B_w[d] = sum over the positions p of window w of (max |G_T,d| + max_j |G_E,d[key of p](j)|), plus max |G_pi,d| for
window 0.  A row that lies inside one window contributes what it contributes to B[l, d]: no new tolerance."""
import math

import numpy as np

import scoreref
from transref import row_key_ids


def expand(obs):
    """Every row (s, a, b, nb) becomes s rows (1, a, b, nb)."""
    obs = np.asarray(obs)
    out = np.repeat(obs, obs[:, 0].astype(np.int64), axis=0)
    out[:, 0] = 1
    return np.ascontiguousarray(out)


def window_sums(v, W):
    """v [.., N + 1] per position (column 0 = position 0) -> [.., ceil(N / W)]: column p >= 1 into window (p - 1) // W, column 0 into
    window 0, every window by math.fsum."""
    v = np.asarray(v, dtype=np.float64)
    N = v.shape[-1] - 1
    nwin = -(-N // W)
    flat = v.reshape(-1, N + 1)
    if W == 1:                                                     # (a window is one position; the sum of two numbers is exact in fsum's sense)
        out = flat[:, 1:].copy()
        out[:, 0] = [math.fsum([x, y]) for x, y in zip(flat[:, 1], flat[:, 0])]
        return out.reshape(v.shape[:-1] + (nwin,))
    out = np.empty((flat.shape[0], nwin))
    for r in range(flat.shape[0]):
        for w in range(nwin):
            out[r, w] = math.fsum(flat[r, 1 + w * W:1 + min((w + 1) * W, N)])
        if nwin:
            out[r, 0] = math.fsum([out[r, 0], flat[r, 0]])
    return out.reshape(v.shape[:-1] + (nwin,))


def positions(pi, T, keys, E, dpi, dT, dE, obs):
    """-> (u [nder, N + 1]: the score per POSITION, (initial + emission) + transition of scoreref.score_rows on the expansion;
    b [nder, N + 1]: the bar scale per position).  Computed once per input; the windows of any W are sums of these."""
    ex = expand(obs)
    parts = scoreref.score_rows(pi, T, keys, E, dpi, dT, dE, ex)
    u = (parts[0] + parts[1]) + parts[2]
    Gpi, GT, GE = scoreref._ratio(dpi, pi), scoreref._ratio(dT, T), scoreref._ratio(dE, E)
    kid = row_key_ids(ex, keys)
    b = np.empty_like(u)
    b[:, 0] = np.abs(Gpi).max(axis=0)
    b[:, 1:] = np.abs(GT).max(axis=(0, 1))[:, None] + np.abs(GE).max(axis=1)[kid].T
    return u, b


def exact_windows(pi, T, keys, E, dpi, dT, dE, obs, W):
    """-> (values [nder, ceil(N / W)], B_w [nder, ceil(N / W)])."""
    u, b = positions(pi, T, keys, E, dpi, dT, dE, obs)
    return window_sums(u, W), window_sums(b, W)


def unbinned_input():
    """The un-binned input of the exact windows' tests: -> (contigs, theta, rho).  The rows are test_gpu_score_vectors' un-binned
    ones (spans to 1000, below 10 000 positions, a one-row and a two-row contig among them); theta and rho are TEN times the per
    base pair rates of test_gpu_gamma.  At those rates a row of a few hundred positions moves the posterior as much as a row of a few
    thousand does on a genome (the rows `smc++ posterior` reads are 10^4 .. 10^5 long where these stop at 1000), so that the score of
    a cut row is visibly NOT uniform over its base pairs: tests/test_score_windows_ref.py holds the input to that."""
    import test_gpu_gamma as tg
    import test_gpu_score_vectors as sv
    contigs = sv.big_inputs("long:M0")[2]
    return contigs, 10.0 * tg.TH_U, 10.0 * tg.RH_U
