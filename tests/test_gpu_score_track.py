"""The score track on the device - `score_rows`, `score_windows` (smcpp_score_rows / _windows; smcpp_amd/csrc/score_track_dev.hpp) -
on every column of every contig, every part, every direction.

The truth is tests/scoreref.py: a float64 forward-backward pass over the pure HMM built from the manager's own getters (pi, T, E and
the three Jacobian getters), which forms the dense xi_p at every position.  Managers come from `test_gpu_gamma`'s helpers; the model
is made differentiable BEFORE the E-step (`PiecewiseModel.differentiable = True`: one direction per piece of `synth.model_pieces()`,
16 of them; explicit seed columns for nder = 1 and 3; a `TwoPopulationModel` of two differentiable populations, 24 directions).  The
oracle does dense M^2 work per position, so every case stays below 3e4 positions.

Bounds.  With G = dX / X the log-derivative tables, the score of row l in direction d is an expectation of G under xi_p and gamma_p,
so its natural scale is  B[l, d] = s_l (max |G_T,d| + max |G_E,d[k_l]|),  and  max |G_pi,d|  for column 0:

  every column, every part, the total   absolute GAMMA_TOL B[l, d]    (2e-5, the project's bar for a posterior entry)
  sum over columns and contigs          each part against rows 0, 1 + 2, 3 of Q_with_gradient() on the same E-step, relative
                                        STAT_TOL (5e-6) of sum_l |oracle[l, d]|.  Row 0 of Q's Jacobian weighs log pi with the
                                        reference's gamma[:, 0], which is NOT normalised (its mass m_c was 0.03 on binned:M64), while
                                        the score's gamma_0 has to be for the sum to be the gradient of the log-likelihood (what
                                        tests/test_scoreref.py holds the oracle to): row 0 is compared with sum_c m_c u_0,c, m_c
                                        read from posterior_columns(c, 0, 1, normalize=False) - the same tolerance, the same scale
  windows at W = 1, 100, one window     (W + 8) 2^-52 of sum |terms| against the overlap-matrix oracle applied to the device's own
                                        per-row values; the windows sum (exactly, math.fsum) to the rows' sum within the same bound;
                                        column 0's initial part sits in window 0
  selections with step > 1, parts on / off, repetition, the other posterior and loglik products before and after, SMCPP_SCORE_WAVES
  = 1, 3 and unset (rows exceed wavefronts, from describe()), SMCPP_DEBUG_POISON=255, a repeated E-step: the same bits

Measured on one MI355X (worst |value - oracle| over every column, part and direction in units of its bar GAMMA_TOL B; the sums over
columns and contigs against Q's Jacobian, initial / emission / transition part, in units of sum |oracle|, bar 5e-6):

  case           directions   of the bar   initial   emission   transition
  binned:M64     16           7.2e-04      7.8e-16   3.0e-09    1.3e-08
  unbinned:M32   16           4.3e-04      6.0e-16   6.4e-09    7.0e-10
  unbinned:M64   16           8.0e-04      7.6e-16   6.2e-08    5.1e-10
  binned:M1      16           1.5e-11      0         1.6e-09    0
  binned:M2      16           2.3e-04      6.1e-17   4.8e-10    1.2e-09
  binned:M5      16           2.3e-03      3.0e-16   5.2e-09    3.2e-09
  binned:M63     16           1.2e-03      5.1e-16   3.1e-09    7.4e-09
  seeds1:M13     1            7.7e-04      1.7e-16   2.2e-10    1.5e-08
  seeds3:M64     3            7.3e-04      2.0e-16   5.4e-10    8.0e-09
  twopop:M48     24           1.6e-03      8.1e-16   2.5e-09    9.9e-09

The worst column uses 0.23 % of its bar (headroom 430): B takes the LARGEST log-derivative of a table where the posterior weighs
typical ones.  Each case takes less than a second beside its manager (the whole file: 5 s).

The caps of 2^31 - 1 output elements and of 1 GiB of scratch are reached on un-binned rows of 10^5 and 2 10^8 positions, which a
save_gamma E-step crosses by eigen-power steps (test_refusals_of_the_caps); both refusals come before any launch or allocation.
Not reached by any test: rows cut into pieces (the plan cuts rows beyond 64 states only, where the score track does not exist, so
k_score_select always sees whole rows today)."""
import math

import numpy as np
import pytest

import scoreref
import test_gpu_gamma as tg
import transref
from test_gpu_parity import GAMMA_TOL, STAT_TOL

pytestmark = pytest.mark.gpu

EPS = scoreref.EPS
SPANS_U = (64, 65, 128, 129, 1000)
CASES = ["binned:M64", "unbinned:M32", "unbinned:M64", "binned:M1", "binned:M2", "binned:M5", "binned:M63", "seeds1:M13", "seeds3:M64",
         "twopop:M48"]
MAX_POSITIONS = 30_000

_INPUTS = {}
_ORACLE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# managers and the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def inputs(case):
    """-> (kind, M, contigs, theta, rho); built once per case and process."""
    kind, M = case.split(":M")
    M = int(M)
    key = (kind, M if kind == "binned" else None)
    if key not in _INPUTS:
        if kind == "unbinned":
            cs = tg.unbinned_contigs(100, spans=SPANS_U, cap=200)
            assert all(s in set(cs[0][:, 0]) for s in SPANS_U)
            r = (cs, tg.TH_U, tg.RH_U)
        elif kind == "twopop":
            r = (tg.twopop_contigs(150_000), None, None)
        else:
            cs = tg.binned_contigs(40 + M, 1_500_000 if (kind, M) == ("binned", 64) else 300_000)
            assert all(s in set(cs[0][:, 0]) for s in (2, 63, 64))
            r = (cs, tg.TH_B, tg.RH_B)
        assert sum(int(c[:, 0].sum()) for c in r[0]) <= MAX_POSITIONS, sum(int(c[:, 0].sum()) for c in r[0])
        assert any(len(c) == 1 for c in r[0]) and any(len(c) == 2 for c in r[0])
        _INPUTS[key] = r
    return (kind, M) + _INPUTS[key]


def seed_columns(kind, K):
    """nder = 1: every piece moves with its own size (d / d log of the overall scale); nder = 3: young, middle, old pieces, signed."""
    from smcpp_amd import synth
    a, _ = synth.model_pieces()
    if kind == "seeds1":
        return a[:, None].copy()
    s = np.zeros((K, 3))
    s[:5, 0] = 1.0
    s[5:11, 1] = -0.5 * a[5:11]
    s[11:, 2] = np.linspace(1.0, 2.0, K - 11)
    return s


def manager(case, estep=True, differentiable=True, save_gamma=True):
    """-> (im, contigs): a differentiable model, a save_gamma E-step (estep=False: none yet)."""
    kind, M, contigs, theta, rho = inputs(case)
    if kind == "twopop":
        im = tg._twopop(M, contigs)
        if differentiable:
            im.model.model1.differentiable = True
            im.model.model2.differentiable = True
            im.model.update_observers("model update")
    else:
        im = tg._onepop(M, contigs, theta, rho)
        m = im.model
        if differentiable and kind.startswith("seeds"):
            seeds = seed_columns(kind, len(m.a))
            m.derivative_seeds = lambda: seeds
        elif differentiable:
            m.differentiable = True
        if differentiable:
            m.update_observers("model update")
    im.save_gamma = bool(save_gamma)
    if estep:
        im.E_step()
        plan = im.describe()["plan"]
        print(f"{case}: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family', 'rows', 'positions')} }")
        assert plan["states_per_lane"] == 1 and not plan["long_rows_cut"], plan
    return im, contigs


def jacobians(im):
    """dpi [M, nder], dT [M, M, nder], dE [K, M, nder] from the C getters (the emission getter brings the table to the host: a later
    Q takes the host route - call this behind everything that asserts the device route)."""
    from smcpp_amd import _engine as E
    M, K, nder = im.M, len(im.keys), E.lib().smcpp_num_derivatives(im._im)
    dpi, dT, dE = np.zeros((M, nder)), np.zeros((M, M, nder)), np.zeros((K, M, nder))
    E.check(E.lib().smcpp_get_pi_jac(im._im, E.dptr(dpi)))
    E.check(E.lib().smcpp_get_transition_jac(im._im, E.dptr(dT)))
    E.check(E.lib().smcpp_get_emission_probs_jac(im._im, E.dptr(dE)))
    return dpi, dT, dE


def oracle(case, im, contigs):
    """tests/scoreref.py on every contig of the case, from the manager's getters; once per case and process, never changed.
    -> (per contig [3, nder, L + 1], the scales B per contig [nder, L + 1])."""
    if case not in _ORACLE:
        dpi, dT, dE = jacobians(im)
        pi, T, keys, Et = im.pi, im.transition, im.keys, transref.emission_table(im)
        Gpi, GT, GE = scoreref._ratio(dpi, pi), scoreref._ratio(dT, T), scoreref._ratio(dE, Et)
        refs, scales = [], []
        for ob in contigs:
            refs.append(scoreref.score_rows(pi, T, keys, Et, dpi, dT, dE, ob))
            kid = transref.row_key_ids(ob, keys)
            B = np.empty((dpi.shape[1], len(ob) + 1))
            B[:, 0] = np.abs(Gpi).max(axis=0)
            B[:, 1:] = ob[:, 0][None, :] * (np.abs(GT).max(axis=(0, 1))[:, None] + np.abs(GE).max(axis=1)[kid].T)
            refs[-1].setflags(write=False)
            scales.append(B)
        _ORACLE[case] = (refs, scales)
    return _ORACLE[case]


def products(im, c):
    return {"parts": im.score_rows(c, parts=True), "rows": im.score_rows(c), "w100": im.score_windows(c, 100), "w7": im.score_windows(c, 7)}


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.float64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        assert np.all(np.isfinite(a[k])), k


def fsum_rows(x):
    return np.array([math.fsum(r) for r in np.asarray(x)])


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------
def check_columns(parts, total, ref, B, label):
    """Every column, every part and the total against the oracle: GAMMA_TOL B[l, d].  -> the worst ratio to the bar."""
    assert parts.shape == ref.shape and parts.dtype == np.float64 and total.shape == ref.shape[1:], (label, parts.shape, ref.shape)
    assert np.all(np.isfinite(parts)) and np.all(B >= 0.0), label
    assert not parts[0, :, 1:].any() and not parts[1:, :, 0].any(), label            # where the parts live
    assert np.array_equal(total, (parts[0] + parts[1]) + parts[2]), label            # the documented order
    # (B = 0 - one hidden state: pi and T are constants - asks for the oracle's value itself: any difference is beyond the bar)
    ratio = np.abs(parts - ref) / np.maximum(GAMMA_TOL * B[None], 1e-300)
    rt = np.abs(total - ref.sum(axis=0)) / np.maximum(GAMMA_TOL * B, 1e-300)
    worst = max(float(ratio.max()), float(rt.max()))
    print(f"{label}: {ref.shape[2] - 1} rows x {ref.shape[1]} directions, worst |value - oracle| / (GAMMA_TOL B) by part "
          f"{[float(f'{ratio[x].max():.3g}') for x in range(3)]}, total {rt.max():.3g}")
    bad = np.argwhere(ratio > 1.0)
    assert len(bad) == 0, f"{label}: {len(bad)} entries beyond the bar, e.g. (part, direction, column) {bad[:6].tolist()}: got " \
                          f"{[parts[tuple(b)] for b in bad[:6]]}, want {[ref[tuple(b)] for b in bad[:6]]}, B {[B[b[1], b[2]] for b in bad[:6]]}"
    assert rt.max() <= 1.0, (label, float(rt.max()))
    return worst


def check_windows(im, c, v, spans, label):
    total = int(np.sum(spans))
    for W in (1, 100, total):
        got = im.score_windows(c, W)
        want, mag = scoreref.score_windows(v, spans, W)
        assert got.dtype == np.float64 and got.shape == want.shape == (v.shape[0], -(-total // W)), (label, W, got.shape)
        tol = (W + 8) * EPS
        err = np.abs(got - want)
        bad = err > tol * mag
        assert not bad.any(), f"{label}, W = {W}: {int(bad.sum())} entries off, worst {np.max(err / np.maximum(mag, 1e-300)) / EPS:.1f} eps (bar {W + 8})"
        serr = np.abs(fsum_rows(got) - fsum_rows(v))
        assert np.all(serr <= tol * fsum_rows(mag)), f"{label}, W = {W}: the windows miss the rows' sum by {np.max(serr / fsum_rows(mag)) / EPS:.1f} eps"
        if W == 1:
            # window 0 = column 0's initial part + row 1's first base pair, nothing else
            first = v[:, 0] + v[:, 1] / spans[0]
            assert np.all(np.abs(got[:, 0] - first) <= 4 * EPS * (np.abs(v[:, 0]) + np.abs(v[:, 1] / spans[0]))), label
            assert got.shape[1] == total


def check_selections(im, c, parts, total, L, label):
    for start, stop, step in ((0, L + 1, 1), (0, L + 1, 3), (1, L + 1, 2), (L, L + 1, 1), (0, 1, 1), (2, max(3, L - 1), 5)):
        if start >= stop or stop > L + 1:
            continue
        sl = slice(start, stop, step)
        assert np.array_equal(im.score_rows(c, start, stop, step), total[:, sl]), (label, start, stop, step)
        assert np.array_equal(im.score_rows(c, start, stop, step, parts=True), parts[:, :, sl]), (label, start, stop, step)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_column_against_the_oracle(engine_opt, case):
    """Every column, part and direction against the position-level oracle; the sums over columns and contigs against
    Q_with_gradient() of the same E-step - which stays on the route the header promises; the windows; the selections."""
    engine_opt("SMCPP_SCORE_WAVES", None)
    im, contigs = manager(case)
    im.Q_with_gradient()
    before = im.describe()["q_route"]
    got = [(im.score_rows(c, parts=True), im.score_rows(c)) for c in range(len(contigs))]
    # include/smcpp_engine.h: "a later smcpp_q KEEPS its device route after a score call" (the two-population preparation runs on the
    # host, and Q with it, before and after)
    q, jac = im.Q_with_gradient()
    route = im.describe()["q_route"]
    print(f"{case}: q_route before / after the score calls: {before} / {route}")
    assert route == before and (route == "device" or case != "binned:M64"), (before, route)
    refs, scales = oracle(case, im, contigs)
    nder = refs[0].shape[1]
    assert jac.shape == (4, nder) and nder == {"seeds1": 1, "seeds3": 3, "twopop": 24}.get(case.split(":")[0], 16)
    worst = 0.0
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        parts, total = got[c]
        worst = max(worst, check_columns(parts, total, refs[c], scales[c], label))
        check_windows(im, c, total, ob[:, 0], label)
        check_selections(im, c, parts, total, len(ob), label)
    # the three parts, summed over every column of every contig, are rows of Q's Jacobian - the initial part of contig c weighted by
    # the mass m_c of its column 0 AS STORED (include/smcpp_engine.h: Q weighs log pi with the reference's unnormalised gamma[:, 0])
    mass = [float(im.posterior_columns(c, 0, 1, normalize=False).sum()) for c in range(len(contigs))]
    assert all(0.0 < m <= 1.0 + 1e-12 for m in mass), mass
    weight = lambda m: np.array([m, 1.0, 1.0])[:, None]                                   # noqa: E731
    sums = np.sum([weight(m) * fsum_rows(g[0].reshape(3 * nder, -1)).reshape(3, nder) for g, m in zip(got, mass)], axis=0)
    mag = np.sum([weight(m) * np.abs(r).sum(axis=2) for r, m in zip(refs, mass)], axis=0)
    want = np.stack([jac[0], jac[1] + jac[2], jac[3]])
    rel = np.abs(sums - want) / np.maximum(mag, 1e-300)
    rel = np.where(mag == 0.0, np.where(sums == want, 0.0, np.inf), rel)
    print(f"{case}: WORST column {worst:.3g} of the bar; sum over columns against Q's Jacobian, by part {[float(f'{rel[x].max():.3g}') for x in range(3)]} "
          f"of sum |oracle| (bar {STAT_TOL})")
    assert np.all(rel <= STAT_TOL), (case, rel.max(axis=1), sums, want)
    # (no part is trivially zero - but for one hidden state, where pi and T are constants)
    assert np.abs(want[1]).max() > 0.0 and (case == "binned:M1" or all(np.abs(refs[0][x]).max() > 0.0 for x in range(3)))


def test_same_bits(engine_opt):
    """Repetition, SMCPP_SCORE_WAVES = 1, 3 and unset (rows exceed wavefronts), the other posterior and loglik products before and
    after (and they unchanged), a repeated E-step, poisoned allocations."""
    from smcpp_amd import _engine
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    for case in ("unbinned:M64", "binned:M5"):
        im, contigs = manager(case)
        nc = len(contigs)
        good = [products(im, c) for c in range(nc)]
        for c in range(nc):
            same_bits(products(im, c), good[c])                                   # repetition
        rows0 = len(contigs[0])
        im.score_rows(0)
        d = im.describe()
        assert d["score_items"] == rows0 and d["score_waves"] == min(rows0, 1024) and d["score_park"] == "lds", d
        for waves in ("1", "3", None):
            engine_opt("SMCPP_SCORE_WAVES", waves)
            for c in range(nc):
                same_bits(products(im, c), good[c])
            im.score_rows(0)
            d = im.describe()
            assert d["score_waves"] == (min(rows0, 1024) if waves is None else int(waves)) and d["score_items"] == rows0 > 3 * 3, d
            assert d["options"].get("SMCPP_SCORE_WAVES") == waves, d["options"]
        # the other products in between: neither side disturbs the other
        for c in range(nc):
            gam = im.posterior_columns(c, normalize=False)
            tr = im.posterior_transitions(c)
            llw, llr = im.loglik_windows(c, 7), im.loglik_rows(c)
            im.posterior_windows_exact(c, 7)
            im.posterior_sample_rows(c, n_paths=2, seed=1)
            same_bits(products(im, c), good[c])
            assert np.array_equal(im.posterior_columns(c, normalize=False), gam)
            tr2 = im.posterior_transitions(c)
            assert all(np.array_equal(tr[k], tr2[k]) for k in tr)
            assert np.array_equal(im.loglik_windows(c, 7), llw) and np.array_equal(im.loglik_rows(c), llr)
        xis, ll = [x.copy() for x in im.xisums], im.logliks().copy()
        im.score_windows(0, 50)
        assert all(np.array_equal(a, b) for a, b in zip(im.xisums, xis)) and np.array_equal(im.logliks(), ll)
        # a repeated E-step on the same parameters
        im.E_step()
        for c in range(nc):
            same_bits(products(im, c), good[c])
        # poisoned allocations: a fresh manager, every fresh device buffer filled with 0xFF bytes
        _engine.set_option("SMCPP_DEBUG_POISON", "255")
        try:
            im3, _ = manager(case)
            for c in range(nc):
                same_bits(products(im3, c), good[c])
        finally:
            _engine.set_option("SMCPP_DEBUG_POISON", None)


def test_refusals(engine_opt):
    """Every refusal raises RuntimeError with a message before anything is launched, and a valid call afterwards succeeds."""
    engine_opt("SMCPP_SCORE_WAVES", None)
    case = "binned:M5"
    im, contigs = manager(case)
    L, nc = len(contigs[0]), len(contigs)
    good = products(im, 0)

    def raises(call, match, usable=im):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip(), "an error without a message"
        if usable is not None:
            same_bits(products(usable, 0), good)

    both = lambda m, c=0: (lambda: m.score_rows(c), lambda: m.score_rows(c, parts=True), lambda: m.score_windows(c, 100))    # noqa: E731
    for c in (-1, nc, nc + 5):
        for call in both(im, c):
            raises(call, "contig")
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(start=4, stop=2), dict(step=0), dict(step=-1), dict(start=L + 1)):
        raises(lambda: im.score_rows(0, **kw), "start|stop|step|selection")
    for W in (0, -5):
        raises(lambda: im.score_windows(0, W), "window_bp")
    # no E-step yet; then one without save_gamma; then a valid one
    fresh, _ = manager(case, estep=False, save_gamma=False)
    for call in both(fresh):
        raises(call, "no E-step", None)
    fresh.E_step()
    for call in both(fresh):
        raises(call, "save_gamma", None)
    fresh.save_gamma = True
    fresh.E_step()
    same_bits(products(fresh, 0), good)
    # parameters set again without an E-step: the stored vectors belong to the earlier ones
    fresh.theta = 2 * tg.TH_B
    for call in both(fresh):
        raises(call, "set again", None)
    fresh.theta = tg.TH_B
    fresh.E_step()
    same_bits(products(fresh, 0), good)
    # no derivative seeds: a model that is not differentiable
    plain, _ = manager(case, differentiable=False)
    for call in both(plain):
        raises(call, "no derivative seeds", None)
    plain.model.differentiable = True
    plain.model.update_observers("model update")
    plain.E_step()
    same_bits(products(plain, 0), good)
    # smcpp_set_raw: the model's own tables (T keeps its structure) carry no seeds; an arbitrary T lacks the structure
    _, M, cs, theta, rho = inputs(case)
    pi, T, keys, Et = im.pi, im.transition, im.keys, transref.emission_table(im)
    plain.set_raw(pi, T, keys, Et)
    plain.E_step()
    for call in both(plain):
        raises(call, "set_raw", None)
    plain.model.update_observers("model update")
    plain.E_step()
    same_bits(products(plain, 0), good)
    raw = tg._unstructured(8, cs, theta, rho)
    raw.save_gamma = True
    raw.E_step()
    for call in both(raw):
        raises(call, "semiseparable structure", None)
    # more than 64 hidden states
    big = tg._onepop(65, cs, theta, rho)
    big.model.differentiable = True
    big.model.update_observers("model update")
    big.save_gamma = True
    big.E_step()
    ll = big.logliks().copy()
    for call in both(big):
        raises(call, "64 hidden states", None)
    assert np.array_equal(big.logliks(), ll) and big.posterior_transitions(0)["stay"].shape == (L + 1,)
    same_bits(products(im, 0), good)


def test_refusals_of_the_caps(engine_opt):
    """The two caps, on un-binned rows that a save_gamma E-step crosses by eigen-power steps (the hybrid plan).  Contig 0 holds a
    row of 2 10^8 positions: 3.1e6 checkpoint vectors of 512 bytes for one wavefront, beyond 1 GiB of scratch whatever is asked of
    it.  Contig 1 holds 1400 rows of 10^5 positions (1562 checkpoints each: small): its windows of one base pair would be
    16 x 1.4e8 outputs, beyond 2^31 - 1.  Both are refused before anything is launched or allocated (the bindings make the
    checks-only call first); logliks() and the posterior products are unchanged, contig 2 answers as before, and contig 1 gives
    its windows of 10^7 base pairs."""
    from smcpp_amd import synth
    engine_opt("SMCPP_SCORE_WAVES", None)
    n, G = tg.N, 10**5
    long_rows = np.array([[1, 1, 2, n], [2 * 10**8, 0, 0, n], [50, 0, 0, n], [1, 1, 2, n]], dtype=np.int32)
    many = np.array([[G, 0, 0, n], [1, 1, 3, n]] * 1400, dtype=np.int32)
    small = inputs("binned:M5")[2][0][:200]
    contigs = [np.ascontiguousarray(c, dtype=np.int32) for c in (long_rows, many, small)]
    im = tg._onepop(64, contigs, tg.TH_U, tg.RH_U)
    im.model.differentiable = True
    im.model.update_observers("model update")
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    print(f"caps: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family', 'hybrid_rows')} }")
    assert plan["hybrid_rows"] and plan["states_per_lane"] == 1 and not plan["long_rows_cut"], plan
    ll = im.logliks().copy()
    assert np.all(np.isfinite(ll))
    good = products(im, 2)
    gam = [im.posterior_columns(c, normalize=False) for c in range(3)]
    tr = im.posterior_transitions(2)

    def usable():
        assert np.array_equal(im.logliks(), ll)
        same_bits(products(im, 2), good)
        assert all(np.array_equal(im.posterior_columns(c, normalize=False), gam[c]) for c in range(3))
        tr2 = im.posterior_transitions(2)
        assert all(np.array_equal(tr[k], tr2[k]) for k in tr)

    for call in (lambda: im.score_rows(0), lambda: im.score_rows(0, 0, 1), lambda: im.score_rows(0, parts=True),
                 lambda: im.score_windows(0, 10**6)):
        with pytest.raises(RuntimeError, match="cap of 1 GiB") as e:
            call()
        assert "score track" in str(e.value)
        usable()
    nder = len(synth.model_pieces()[0])
    assert nder * int(many[:, 0].sum()) > 2**31 - 1
    with pytest.raises(RuntimeError, match="cap of 2\\^31 - 1") as e:
        im.score_windows(1, 1)
    assert "score track" in str(e.value)
    usable()
    w = im.score_windows(1, 10**7)                                     # a valid call on the contig that was refused: 1024 wavefronts walk its rows
    assert w.shape == (nder, -(-int(many[:, 0].sum()) // 10**7)) and np.all(np.isfinite(w))
    rows = im.score_rows(1)
    tol = (10**7 + 8) * EPS * np.abs(rows).sum(axis=1)
    assert np.all(np.abs(fsum_rows(w) - fsum_rows(rows)) <= tol)
    d = im.describe()
    assert d["score_items"] == len(many) and d["score_waves"] == 1024, d
    usable()


def test_evidence_score_track_and_information(engine_opt):
    """evidence.score_track: one manager, one save_gamma E-step, the arrays of im.score_windows; explicit seeds replace the model's;
    information / covariance on the device's track; the total score is the gradient Q_with_gradient() reports."""
    from smcpp_amd import synth
    from smcpp_amd.evidence import covariance, information, score_track
    from smcpp_amd.model import PiecewiseModel
    engine_opt("SMCPP_SCORE_WAVES", None)
    _, M, contigs, theta, rho = inputs("binned:M5")
    a, s = synth.model_pieces()
    model = PiecewiseModel(a, s, 1e4, "pop1")
    body = [c for c in contigs if len(c) > 2]
    with pytest.raises(RuntimeError, match="no derivative seeds"):
        score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100)
    model.differentiable = True
    hs, track, im = score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, return_manager=True)
    assert len(track) == len(body) and all(t.shape[0] == len(a) and t.dtype == np.float64 for t in track)
    for c in range(len(body)):
        assert np.array_equal(track[c], im.score_windows(c, 100))
    _, jac = im.Q_with_gradient()
    info = information(track, block=5)
    # the scale of the sum: |part| over every part, column and contig (the parts of a row may cancel in its total)
    mag = np.sum([np.abs(im.score_rows(c, parts=True)).sum(axis=(0, 2)) for c in range(len(body))], axis=0)
    # (rows 1 .. 3 of Q's Jacobian are the emission and transition parts; row 0 weighs the initial part by the stored mass of column 0)
    u0 = np.sum([im.score_rows(c, 0, 1, parts=True)[0, :, 0] for c in range(len(body))], axis=0)
    assert np.all(np.abs(info["score"] - u0 - jac[1:].sum(axis=0)) <= STAT_TOL * mag), (info["score"], u0, jac[1:].sum(axis=0))
    cov = covariance(info)
    assert cov["cov"].shape == (len(a), len(a)) and np.all(np.isfinite(cov["se"])) and np.all(cov["se"] >= 0.0)
    # explicit seeds replace the model's: one direction, the sum of the first three pieces' directions
    seeds = np.zeros((len(a), 1))
    seeds[:3, 0] = 1.0
    plain = PiecewiseModel(a, s, 1e4, "pop1")
    _, t1, im1 = score_track(plain, body, synth.hidden_states(M), tg.N, theta, rho, 100, seeds=seeds, return_manager=True)
    assert all(t1[c].shape == (1, track[c].shape[1]) for c in range(len(body)))
    _, jac1 = im1.Q_with_gradient()
    assert jac1.shape == (4, 1)
    got = sum(math.fsum(t[0]) for t in t1) - sum(float(im1.score_rows(c, 0, 1, parts=True)[0, 0, 0]) for c in range(len(body)))
    assert abs(got - jac1[1:].sum()) <= STAT_TOL * mag[:3].sum() and abs(got - jac[1:, :3].sum()) <= 2 * STAT_TOL * mag[:3].sum(), (got, jac1)
