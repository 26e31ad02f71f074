"""The coefficient planes of the score track's vector form (smcpp_host_score_planes; smcpp_amd/csrc/engine_params.hpp: score_planes)
against the dense Jacobian the engine expands from the same generator planes, and the numpy restatement of the vector form
(tests/scorevec_ref.py) against the dense oracle (tests/scoreref.py).  No GPU.

Bars, counted from the operations (eps = 2^-52, om = 1 - 1e-5, c0 = 1e-5 / (M + 1)):

  below the diagonal   dT = fl(ded om).  Rebuilt: cL T with cL = fl(fl(ded om) / g), g the engine's own fl(fl(ed om) + c0), which is
                       T(i, j) but for one rounding where a compiler fuses the multiply-add on one side only: three roundings and
                       that one.  Bar 6 eps |cL| T.
  above                dT = fl(fl(fl(dpf W) + fl(pf dW)) om): four roundings of two terms.  Rebuilt: fl(fl(cP + cW) fl(T - c0)) with
                       cP = fl(dpf / pf), cW = fl(dW / W) and T = fl(fl(fl(pf W) om) + c0), whose roundings are absolute in T - c0 -
                       which is why the absolute terms of the entry are (|cP| + |cW|) (T + c0): eight roundings in all, beside the
                       four of dT on terms of the same size.  Bar 12 eps (|cP| + |cW|) (T + c0).
  the diagonal         dT = -fl(om ds), ds the sequential sum of the row's M - 1 entry derivatives (three roundings each): (M + 2) eps of
                       the row's sum of |terms|.  Rebuilt: cD T(j, j) = fl(fl(fl(-dsum om) / T(j, j)) T(j, j)), dsum from a prefix sum of
                       ded and suffix sums of W and dW - differently ordered, M additions and four roundings more.  Bar (2 M + 12) eps of
                       om (sum_{c<j} |ded_c| + |dpf_j| sum_{c>j} W_c + pf_j sum_{c>j} |dW_c|).
  floored entries      above the diagonal an entry whose raw value pf_i W_j lies below 1e-20 has dT = 0 while the planes keep
                       raw (cP + cW): excluded from the comparison, counted, and each bound 1e-20 / c0 |cP_i + cW_j| on what it moves
                       a position's xi-weighted sum by is held below 1e-12 of the scale max |dT_d / T| (FLOOR_BAR has the grids).

  the restatement      D, L, U1, U2 of every row from the dense xi sums, contracted with the planes, against scoreref's transition
                       part: both are sums of M^2 products O(i, j) c; the entries differ by the bars above (<= (2 M + 12) eps of
                       their absolute terms), the sums add M^2 roundings in different orders.  Bar (M^2 + 2 M + 12) eps of
                       sum |O(i, j)| |terms of the entry| (it holds with a factor of hundreds to spare), plus the floored entries'
                       bound times the row's span."""
import numpy as np
import pytest

import scoreref
import scorevec_ref as sv
from smcpp_amd import _engine as E
from smcpp_amd import synth

EPS = sv.EPS
RHO = 2e-4
STATES = (1, 2, 5, 64, 65, 256)
NDER = (1, 3, 16)
# hidden states stretched until young-to-old entries fall below the 1e-20 floor of the upper triangle
STRETCH = {"plain": 1.0, "stretched": 6.0}
# The floored entries' bound against the scale max |G_T,d|: 1e-12 on the model's own grids.  The stretched grids are there for the
# floor to be reached at all (4 entries at M = 5, 118 at 64, 120 at 65); their far entries carry the largest log-derivatives of the
# matrix beside the smallest c0, so they are held to what matters downstream instead: 1e-5 of the bar the device's columns are held
# to, GAMMA_TOL (2e-5) of the same scale.  Measured: 6e-13 at M = 64 / 65, 2e-12 at M = 256, 2e-11 at M = 5 with 16 directions.
FLOOR_BAR = {"plain": 1e-12, "stretched": 1e-5 * 2e-5}


def seeds(nder):
    a, _ = synth.model_pieces()
    K = len(a)
    if nder == 1:
        return a[:, None].copy()
    if nder == K:
        return np.diag(a)
    s = np.zeros((K, nder))
    s[:5, 0] = 1.0
    s[5:11, 1] = -0.5 * a[5:11]
    s[11:, 2] = np.linspace(1.0, 2.0, K - 11)
    return s


def planes(M, nder, stretch=1.0):
    a, s = synth.model_pieces()
    hs = np.asarray(synth.hidden_states(M), dtype=np.float64).copy()
    hs[1:-1] *= stretch
    return E.host_score_planes(a, seeds(nder), s, hs, RHO)


@pytest.mark.parametrize("kind", sorted(STRETCH))
@pytest.mark.parametrize("nder", NDER)
@pytest.mark.parametrize("M", STATES)
def test_planes_rebuild_the_dense_jacobian(M, nder, kind):
    if nder == 16:
        assert len(synth.model_pieces()[0]) == 16
    o = planes(M, nder, STRETCH[kind])
    T, dT = o["T"], o["dT"]
    assert dT.shape == (M, M, nder) and all(o[k].shape == (nder, M) for k in ("cD", "cL", "cW", "cP"))
    assert all(np.all(np.isfinite(o[k])) for k in o)
    c0, om = 1e-5 / (M + 1), 1.0 - 1e-5
    rebuilt, mag = sv.dense_from_planes(T, o["cD"], o["cL"], o["cW"], o["cP"])
    i, j = np.indices((M, M))
    err = np.abs(rebuilt - dT)
    # floored entries of the upper triangle: T is exactly the floor there
    floored = (i < j) & (T == 1e-20 * om + c0)
    nfl = int(floored.sum())
    below, above, diag = i > j, (i < j) & ~floored, i == j
    worst = {}
    for name, mask, factor in (("below", below, 6.0), ("above", above, 12.0)):
        if mask.any():
            r = err[mask] / np.maximum(factor * EPS * mag[mask], 1e-300)
            worst[name] = float(r.max())
            assert worst[name] <= 1.0, (name, worst[name])
    # the diagonal: the row's sum of |terms|, from the rebuilt entries' magnitudes (om |dx_c| each, floored or not)
    up_terms = np.where((i < j)[..., None], (np.abs(o["cP"].T)[:, None, :] + np.abs(o["cW"].T)[None, :, :]) * np.abs(T - c0)[..., None], 0.0)
    row_terms = np.where(below[..., None], mag, 0.0).sum(axis=1) + up_terms.sum(axis=1)
    r = err[diag] / np.maximum((2 * M + 12) * EPS * row_terms, 1e-300)
    worst["diagonal"] = float(r.max())
    assert np.all((err[diag] == 0.0) | (r <= 1.0)), worst
    # the floored entries: how many, and what each can move
    GT = scoreref._ratio(dT, T)
    scale = np.abs(GT).max(axis=(0, 1))              # [nder]: max |G_T,d|, what one position adds to the scale B[l, d] of its row l
    if nfl:
        assert not dT[floored].any()
        bound = (1e-20 / c0) * np.abs(o["cP"].T[:, None, :] + o["cW"].T[None, :, :])[floored]
        ratio = bound / np.maximum(scale[None, :], 1e-300)
        worst["floor bound / row scale"] = float(ratio.max())
        assert np.all(ratio <= FLOOR_BAR[kind]), worst
    print(f"M = {M}, nder = {nder}, {kind}: {nfl} floored entries above the diagonal; worst error in units of its bar {worst}")
    assert (nfl > 0) == (kind == "stretched" and M >= 5), (M, nfl)            # the model's own grid never reaches the floor


def hmm(M, spans, seed):
    """A pure HMM on the model's T: positive emission vectors of four keys, rows of the given spans."""
    rng = np.random.default_rng(seed)
    K = 4
    keys = np.stack([np.arange(K), np.zeros(K, dtype=np.int64), np.arange(K) % 2], axis=1)
    Et = np.exp(-rng.uniform(0.2, 3.0, size=(K, M)))
    pi = rng.uniform(0.5, 1.5, size=M)
    obs = np.concatenate([np.asarray(spans)[:, None], keys[np.arange(len(spans)) % K]], axis=1)
    return pi / pi.sum(), keys, Et, obs


@pytest.mark.parametrize("kind", sorted(STRETCH))
@pytest.mark.parametrize("M", (5, 65))
def test_vector_form_equals_the_dense_oracle(M, kind):
    nder = 3
    o = planes(M, nder, STRETCH[kind])
    T, dT = o["T"], o["dT"]
    spans = (1, 64, 65, 200, 1, 2)
    pi, keys, Et, obs = hmm(M, spans, 7 + M)
    zero_pi, zero_E = np.zeros((M, nder)), np.zeros((len(Et), M, nder))
    ref = scoreref.score_rows(pi, T, keys, Et, zero_pi, dT, zero_E, obs)[2][:, 1:]                 # [nder, rows]
    O = sv.xi_sums(pi, T, keys, Et, obs)
    GT = scoreref._ratio(dT, T)
    # the xi sums are scoreref's: the same contraction gives its transition part
    mine = np.einsum("lij,ijd->dl", O, GT)
    assert np.all(np.abs(mine - ref) <= 4 * M * M * EPS * np.einsum("lij,ijd->dl", O, np.abs(GT)))
    assert np.allclose(O.sum(axis=(1, 2)), spans, rtol=1e-12)
    got = sv.contract(*sv.shares(O, T), o["cD"], o["cL"], o["cW"], o["cP"])
    mag = sv.contract(*sv.shares(O, T, absolute=True), *(np.abs(o[k]) for k in ("cD", "cL", "cW", "cP")))
    c0, om = 1e-5 / (M + 1), 1.0 - 1e-5
    i, j = np.indices((M, M))
    floored = (i < j) & (T == 1e-20 * om + c0)
    fb = np.zeros((nder, len(spans)))
    if floored.any():
        per_entry = (1e-20 * om / T)[..., None] * np.abs(o["cP"].T[:, None, :] + o["cW"].T[None, :, :])      # raw / T |cP + cW|
        fb = np.einsum("lij,ijd->dl", O * floored[None], per_entry)
    bar = (M * M + 2 * M + 12) * EPS * mag + 2.0 * fb
    ratio = np.abs(got - ref) / np.maximum(bar, 1e-300)
    print(f"M = {M}, {kind}: {int(floored.sum())} floored entries, their share at most {fb.max():.3g}; "
          f"worst |vector form - dense oracle| / bar = {ratio.max():.3g}")
    assert np.all(ratio <= 1.0), ratio.max()
    assert np.abs(ref).max() > 0.0
