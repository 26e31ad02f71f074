"""Dense float64 reference of the log-likelihood track (smcpp_loglik_rows / _positions / _windows): the forward pass of the PURE
hidden Markov model - initial distribution pi, transition matrix T [M x M], one emission vector per key - one position at a time,
renormalised at every position, the logs of the normalisers accumulated:

    a_0 = pi;   u_p = e_p o (T^T a_{p-1}),  z_p = sum(u_p),  a_p = u_p / z_p;   l(0) = 0,  l(p) = l(p - 1) + log z_p.

Positions run 0 .. N (N = the sum of the spans); position 0 carries no observation, row l covers positions P_{l-1} + 1 .. P_l.
Like tests/posref.py it is built from what a manager's getters hand out and shares nothing with the kernel: no generators of T, no
float vectors, no floor, no stored log c.  About 3 s per million positions at M <= 64.

The reference's own float noise.  oracle/oracle.py restates the reference's E-step INCLUDING its float alpha (floored at 1e-10) and
its eigen-power steps over long rows; `noise` measures how far that moves the evidence of a row and of a window from this file's
float64 values - the yardstick tests/test_gpu_loglik_track.py holds the engine to (4 x, per input and window width).  The oracle has
no value inside a row; there its row value is split in this file's own proportions, so a window's noise is that of the rows and
parts of rows it holds.  Measured (tests/test_llref.py prints them), d_row / d_win(100) / d_win(10^4):
    G1_M16_n4              6.37e-07  5.74e-07  1.97e-06
    G2_M51_n6_longspans    6.93e-07  6.03e-07  5.70e-07
    G4_M64_n20_2Mbp        3.48e-07  7.18e-07  1.89e-05
and the totals l(N) agree with the oracle's loglik to 3.6e-09, 1.8e-09 and 4.2e-09 relative."""
import numpy as np

from transref import emission_table, row_key_ids  # noqa: F401  (re-exported for the tests)

EPS = 2.0 ** -52


def track(pi, T, keys, E, obs):
    """l [N + 1] at every position of the contig `obs` (rows of span, key...)."""
    pi = np.asarray(pi, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    obs = np.asarray(obs)
    spans = obs[:, 0].astype(np.int64)
    kid = row_key_ids(obs, keys)
    Tt = np.ascontiguousarray(T.T)
    N = int(spans.sum())
    z = np.empty(N + 1)
    z[0] = 1.0
    a = pi / pi.sum()
    p = 1
    for l in range(len(obs)):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            s = a.sum()
            a /= s
            z[p] = s
            p += 1
    return np.cumsum(np.log(z))                      # (sequential: l(p) = l(p - 1) + log z_p)


def prefix(obs):
    return np.concatenate([[0], np.cumsum(np.asarray(obs)[:, 0].astype(np.int64))])


def rows(ell, obs):
    """[L + 1]: log c of every row, l(P_l) - l(P_{l-1}); row 0 gives 0."""
    P = prefix(obs)
    return np.concatenate([[0.0], np.diff(ell[P])])


def grid(ell, pos0=0, pos1=None, step=1):
    return ell[pos0:(len(ell) if pos1 is None else pos1):step].copy()


def windows(ell, W):
    """[ceil(N / W)]: l(min((w + 1) W, N)) - l(w W)."""
    N = len(ell) - 1
    b = np.minimum(np.arange(0, N + W, W, dtype=np.int64), N)
    b = b[:-(-N // W) + 1]
    return np.diff(ell[b])


def split_rows(ell, obs, log_c):
    """l' [N + 1] with the per-row values `log_c` [L + 1] (row 0 unused) at the row ends and every row's value split inside the row
    in the proportions of `ell`: l'(P_{l-1} + q) = l'(P_{l-1}) + log_c[l] (l(P_{l-1} + q) - l(P_{l-1})) / (l(P_l) - l(P_{l-1}))."""
    P = prefix(obs)
    spans = np.diff(P)
    lc = np.asarray(log_c, dtype=np.float64)[1:]
    start = np.concatenate([[0.0], np.cumsum(lc)])[:-1]
    own = np.diff(ell[P])
    out = np.empty_like(ell)
    out[0] = 0.0
    rep = lambda v: np.repeat(v, spans)
    frac = (ell[1:] - rep(ell[P[:-1]])) / rep(np.where(own != 0.0, own, 1.0))
    out[1:] = rep(start) + rep(lc) * frac
    return out


def noise(pi, T, keys, E, obs, widths=()):
    """The reference's own float noise on this input: -> (ell, d_row, {W: d_win}, relative difference of the totals), the oracle's
    restatement of the reference against `track`."""
    from oracle import oracle
    ell = track(pi, T, keys, E, obs)
    o = oracle.estep(pi, T, keys, E, obs)
    lc = np.asarray(o["log_c"], dtype=np.float64)
    d_row = float(np.max(np.abs(rows(ell, obs)[1:] - lc[1:])))
    ell_o = split_rows(ell, obs, lc)
    d_win = {int(W): float(np.max(np.abs(windows(ell, int(W)) - windows(ell_o, int(W))))) for W in widths}
    return ell, d_row, d_win, abs(ell[-1] - o["loglik"]) / abs(o["loglik"])
