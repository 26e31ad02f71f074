"""Dense reference of Q and its gradient in extended precision (plain module: no fixtures, no GPU).

Q's four terms in the engine's order - [gamma0 . log pi, gamma sums . log E over keys with nb == 0, the same over keys with
nb > 0, xi . log T] (HMM::Q of the reference, summed over contigs) - and their forward-mode gradients sum (w / x) dx, written
once in numpy.longdouble with numpy.sum (pairwise) accumulation.  The parameters come from the HOST preparation
(`_engine.host_prep_onepop_jac`: tests/test_prep.py pins it against the compiled reference, G10 against the reference's own
automatic differentiation); the device kernels share no code path with this: they never form T or dT and prepare E and dE
themselves.  `richardson` is a second reference that uses no dual number at all."""
import numpy as np

LD = np.longdouble


def edge_keys(n):
    """Every emission key a sample of n undistinguished lineages can show, plus the missing-data keys (as
    tests/test_gpu_prep.py::test_device_kernels_edge_sizes lists them)."""
    return np.array([[-1, 0, 0], [0, 0, 0], [1, 0, 0]] + [[a, b, n] for a in (0, 1) for b in range(n + 1) if not (a == 0 and b == 0)]
                    + ([[0, 1, n - 1], [-1, 1, n]] if n >= 2 else []), dtype=np.int32)


def dense_q(g0, xi, gs, keys, pi, T, E, dpi=None, dT=None, dE=None):
    """val [4] and (with the Jacobians [.., nder]) jac [4, nder], longdouble.  A zero weight contributes nothing (the engine and
    the reference skip keys no contig holds)."""
    g0, xi, gs = (np.asarray(x, dtype=LD) for x in (g0, xi, gs))
    pi, T, E = (np.asarray(x, dtype=LD) for x in (pi, T, E))
    nb = np.asarray(keys)[:, 2] > 0

    def term(w, x):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = w * np.log(x)
        return np.sum(np.where(w == 0, LD(0), t))

    val = np.array([term(g0, pi), term(gs[~nb], E[~nb]), term(gs[nb], E[nb]), term(xi, T)], dtype=LD)
    if dpi is None:
        return val
    nder = np.asarray(dpi).shape[-1]

    def dterm(w, x, dx):
        f = (w / x).reshape(-1, 1)
        return np.sum(f * np.asarray(dx, dtype=LD).reshape(-1, nder), axis=0) if f.size else np.zeros(nder, dtype=LD)

    dE = np.asarray(dE)
    jac = np.array([dterm(g0, pi, dpi), dterm(gs[~nb], E[~nb], dE[~nb]), dterm(gs[nb], E[nb], dE[nb]), dterm(xi, T, dT)], dtype=LD)
    return val, jac


def manager_statistics(im):
    """The statistics Q weighs, summed over the manager's contigs in longdouble: g0 [M], xi [M, M], gs [keys, M] in the order of
    `im.keys`; a key absent from a contig's dictionary contributes zero."""
    keys = im.keys
    M = im.M
    g0 = np.zeros(M, dtype=LD); xi = np.zeros((M, M), dtype=LD); gs = np.zeros((len(keys), M), dtype=LD)
    for g in im.gammas:
        g0 += g[:, 0]
    for x in im.xisums:
        xi += x
    for d in im.gamma_sums:
        for i, k in enumerate(keys):
            v = d.get(tuple(int(x) for x in k))
            if v is not None:
                gs[i] += v
    return g0, xi, gs


def host_reference(n, hs, pol, a, da, s, theta, rho, alpha, keys, g0, xi, gs):
    """(val, jac) of the dense evaluation on the host preparation of these parameters, and that preparation."""
    from smcpp_amd import _engine
    da = np.asarray(da, dtype=np.float64).reshape(len(a), -1)
    if da.shape[1] == 0:
        pi, T, E = _engine.host_prep_onepop(n, hs, pol, a, s, theta, rho, alpha, keys)
        return dense_q(g0, xi, gs, keys, pi, T, E), np.zeros((4, 0), dtype=LD), (pi, T, E, None, None, None)
    p = _engine.host_prep_onepop_jac(n, hs, pol, a, da, s, theta, rho, alpha, keys)
    val, jac = dense_q(g0, xi, gs, keys, *p)
    return val, jac, p


def synthetic_statistics(rng, M, K):
    """Statistics of the right shapes and magnitudes without an E-step (banded xi, one key no contig holds)."""
    g0 = rng.random(M)
    xi = rng.random((M, M)) * np.exp(-np.abs(np.subtract.outer(np.arange(M), np.arange(M))))
    gs = rng.random((K, M)) * 100.0
    if K > 3:
        gs[3] = 0.0
    return g0, xi, gs


def richardson(n, hs, pol, a, da, s, theta, rho, alpha, keys, g0, xi, gs, h=1e-3):
    """dQ/d(direction) [4, nder] by Richardson-extrapolated central differences (4 D(h) - D(2 h)) / 3 of the longdouble dense Q
    over the host preparation's VALUES at a +- h da[:, d], statistics held fixed.  No dual number takes part."""
    from smcpp_amd import _engine
    a = np.asarray(a, dtype=np.float64)
    da = np.asarray(da, dtype=np.float64)

    def q_at(x):
        return dense_q(g0, xi, gs, keys, *_engine.host_prep_onepop(n, hs, pol, x, s, theta, rho, alpha, keys))

    out = np.zeros((4, da.shape[1]), dtype=LD)
    for d in range(da.shape[1]):
        D = [(q_at(a + k * h * da[:, d]) - q_at(a - k * h * da[:, d])) / (2 * k * LD(h)) for k in (1, 2)]
        out[:, d] = (4 * D[0] - D[1]) / 3
    return out


def errors(val, jac, rval, rjac):
    """Worst relative error of the four values and worst error of a Jacobian row in units of the row's largest entry (rows of the
    reference that are identically zero are compared absolutely: both must then be zero)."""
    val = np.asarray(val, dtype=LD); rval = np.asarray(rval, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        ev = np.where(rval == 0, np.abs(val), np.abs(val - rval) / np.abs(rval))
    ej = 0.0
    rjac = np.asarray(rjac, dtype=LD)
    if rjac.size:
        jac = np.asarray(jac, dtype=LD)
        sc = np.abs(rjac).max(axis=1)
        d = np.abs(jac - rjac).max(axis=1)
        ej = float(np.max(np.where(sc == 0, d, d / np.where(sc == 0, 1, sc))))
    return float(ev.max()), ej


# ---- the shape sweep of the M-step tests: (M, n, contigs, pieces K, nder) ----
SWEEP = [(1, 4, 1, 6, 2), (2, 1, 2, 6, 1),                    # single state; one undistinguished lineage
         (17, 7, 3, 6, 5), (50, 6, 2, 16, 7),                 # M != Mp, several contigs, tail group of 1 and of 3
         (64, 20, 22, 16, 16),                                # the whole-genome contig count at the headline shape
         (100, 6, 3, 16, 3), (130, 6, 1, 16, 9),              # 64 < M <= 256, M != Mp
         (256, 50, 2, 16, 4), (300, 10, 1, 16, 2), (1024, 10, 1, 16, 1),
         (48, 55, 1, 16, 6), (48, 56, 1, 16, 6),              # last sample size the device preparation accepts / first it refuses
         (32, 10, 1, 33, 33), (32, 10, 1, 3, 8)]              # nine direction groups with a tail; more directions than pieces
IDENTITY_SEEDS = (64, 20, 22, 16, 16)
MARKED_SEEDS = [(50, 6, 2, 16, 7), (32, 10, 1, 33, 33)]       # one zero column (3), two equal columns in different groups (1, 6)
POL = 0.3


def sweep_id(case):
    return "M%d-n%d-c%d-K%d-d%d" % tuple(case)


def sweep_inputs(case, seed=2024):
    """Hidden states, pieces and derivative seeds of one sweep case (dense standard-normal seeds but for IDENTITY_SEEDS)."""
    from smcpp_amd import synth
    M, n, _, K, nder = case
    hs = synth.hidden_states(M) if M > 2 else np.array([0.0, np.inf] if M == 1 else [0.0, 0.3, np.inf])
    a, s = synth.model_pieces(K)
    da = np.random.default_rng(seed).standard_normal((K, nder))
    if tuple(case) == IDENTITY_SEEDS:
        da = np.eye(K)
    if tuple(case) in MARKED_SEEDS:
        da[:, 3] = 0.0
        da[:, 6] = da[:, 1]
    return dict(n=n, hs=hs, pol=POL, a=a, da=np.ascontiguousarray(da), s=s, theta=synth.THETA, rho=synth.RHO, alpha=synth.ALPHA)


def check_marked_columns(case, jac):
    """The zero seed column's gradient is exactly 0.0; the two equal columns' gradients are equal bit for bit."""
    if tuple(case) not in MARKED_SEEDS:
        return
    jac = np.asarray(jac)
    assert np.all(jac[:, 3] == 0.0), jac[:, 3]
    assert np.array_equal(jac[:, 1], jac[:, 6]), (jac[:, 1], jac[:, 6])
    assert np.abs(jac[:, 1]).max() > 0


def floor_inputs():
    """Inputs on which the floors of the preparation bind (M = 256, n = 20): hidden states log-spaced from 0.01 to 100 coalescent
    units instead of synth.hidden_states' 0.01 .. 10.  Transitions from the oldest states to the youngest fall below the 1e-20 floor
    of T, the youngest (narrowest) states keep emission entries of many derived alleles on the 1e-10 floor of E."""
    case = (256, 20, 1, 16, 4)
    p = sweep_inputs(case)
    m = np.arange(1, 256)
    p["hs"] = np.concatenate(([0.0], 0.01 * (100.0 / 0.01) ** ((m - 1) / 254.0), [np.inf]))
    return case, p


def floored_entries(prep):
    """Boolean masks (T, E) of the entries whose whole derivative row is zero in a host preparation with Jacobian ("the derivative
    of a floored entry is zero"); emission entries that are the constant 1 (fully missing observation) do not count."""
    pi, T, E, dpi, dT, dE = prep
    return np.all(dT == 0, axis=-1), np.all(dE == 0, axis=-1) & (E != 1.0)
