"""numpy oracle of the posterior transition products (smcpp_posterior_transitions / _transition_windows): a position-level
forward-backward pass in float64 over the PURE hidden Markov model - initial distribution pi, transition matrix T [M x M], one
emission vector per key - that forms the dense xi_p(i, j) of every position and adds up its diagonal and its two triangles per row.

It is built from what a manager's getters hand out (`im.pi`, `im.transition`, `im.emission_probs`, `im.keys`) and the rows the manager
was given.  On purpose it shares nothing with the kernel: no generators of T, no three-addend split of the forward step, no float
vectors, no floor; vectors are renormalised at every position (xi_p is scale free).  Written for clarity, not speed: two Python loops
over the positions (about 10 s per million positions at M = 64); memory is one vector per row boundary plus one row's interior.

`transition_windows` is the second product from the explicit overlap matrix of rows and windows, in blocks of windows."""
import numpy as np

EPS = 2.0 ** -52


def row_key_ids(obs, keys):
    """Row -> index of its key (the columns behind the span) in `keys` [K x keylen]."""
    lut = {tuple(int(x) for x in k): i for i, k in enumerate(np.asarray(keys))}
    return np.array([lut[tuple(int(x) for x in r[1:])] for r in np.asarray(obs)], dtype=np.int64)


def emission_table(im):
    """[K x M] in the order of `im.keys`, from the manager's own getter."""
    ep = im.emission_probs
    return np.array([ep[tuple(k)] for k in im.keys.tolist()], dtype=np.float64)


def transitions(pi, T, keys, E, obs, cells=1 << 22):
    """-> [3 x (L + 1)]: rows stay, up, down; column l >= 1 belongs to row l of `obs` (span, key...), column 0 is zero.

    a_0 = pi, a_p = e_p o (T^T a_{p-1}); b_N = 1, b_{p-1} = T (e_p o b_p); xi_p(i, j) = a_{p-1}(i) T(i, j) e_p(j) b_p(j) / (its sum);
    stay = trace, up = strict upper triangle (i < j: to a higher state), down = strict lower triangle, summed over the row's positions."""
    pi = np.asarray(pi, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    obs = np.asarray(obs)
    M, L = len(pi), len(obs)
    spans = obs[:, 0].astype(np.int64)
    kid = row_key_ids(obs, keys)
    # forward vectors at the row boundaries
    A = np.empty((L + 1, M))
    a = pi / pi.sum()
    A[0] = a
    Tt = np.ascontiguousarray(T.T)
    for l in range(L):
        e = E[kid[l]]
        for _ in range(int(spans[l])):
            a = e * (Tt @ a)
            a /= a.sum()
        A[l + 1] = a
    out = np.zeros((3, L + 1))
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    lower = upper.T
    diag = np.eye(M, dtype=bool)
    b = np.ones(M) / M                                     # after the last position
    blk = max(1, cells // (M * M))
    for l in range(L - 1, -1, -1):
        e, s = E[kid[l]], int(spans[l])
        X = np.empty((s, M))                               # X[t] = a before position t of the row
        a = A[l]
        for t in range(s):
            X[t] = a
            a = e * (Tt @ a)
            a /= a.sum()
        W = np.empty((s, M))                               # W[t] = e o b after position t
        for t in range(s - 1, -1, -1):
            W[t] = e * b
            b = T @ W[t]
            b /= b.sum()
        acc = np.zeros(3)
        for t0 in range(0, s, blk):
            xi = X[t0:t0 + blk, :, None] * T[None, :, :] * W[t0:t0 + blk, None, :]          # dense, per position
            xi /= xi.sum(axis=(1, 2), keepdims=True)
            acc += (xi[:, diag].sum(), xi[:, upper].sum(), xi[:, lower].sum())
        out[:, l + 1] = acc
    return out


def transition_windows(v, spans, W, block=2048):
    """[3 x ceil(P / W)] from per-row values v [3 x (L + 1)] (column 0 takes no part): out[x, w] = sum_l O[l, w] / s_l * v[x, l] with
    the explicit overlap matrix O[l, w] = |[P_{l-1}, P_l) n [w W, (w + 1) W)|, formed for `block` windows and the rows that reach
    into them at a time.  -> (out, covered base pairs per window)."""
    v = np.asarray(v, dtype=np.float64)[:, 1:]
    spans = np.asarray(spans, dtype=np.int64)
    assert v.shape == (3, len(spans)) and W >= 1
    P1 = np.cumsum(spans)
    P0 = P1 - spans
    total = int(P1[-1])
    nwin = -(-total // W)
    lo = np.arange(nwin, dtype=np.int64) * W
    hi = np.minimum(lo + W, total)
    per_bp = v / spans
    out = np.empty((3, nwin))
    for w0 in range(0, nwin, block):
        w1 = min(nwin, w0 + block)
        l0 = int(np.searchsorted(P1, lo[w0], side="right"))               # first row that ends behind the block's start
        l1 = int(np.searchsorted(P0, hi[w1 - 1], side="left"))            # first row that starts at or behind its end
        O = np.clip(np.minimum(P1[l0:l1, None], hi[None, w0:w1]) - np.maximum(P0[l0:l1, None], lo[None, w0:w1]), 0, None)
        out[:, w0:w1] = per_bp[:, l0:l1] @ O.astype(np.float64)
    return out, (hi - lo).astype(np.float64)
