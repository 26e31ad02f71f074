"""The VECTOR form of the score track on the device (SMCPP_SCORE_FORM=vectors; smcpp_amd/csrc/score_vec_dev.hpp): four O(M)
accumulators per row against the coefficient planes of the transition Jacobian instead of the M x M accumulator, at one to four
states per lane.

Truth, bars and helpers are tests/test_gpu_score_track.py's: the position-level oracle tests/scoreref.py from the manager's own
getters (the DENSE Jacobian of T among them, which the vectors form never expands), every column, part and direction at
GAMMA_TOL B[l, d], the sums over columns and contigs against Q's Jacobian at STAT_TOL of sum |oracle|, the windows against the
overlap-matrix oracle, the selections bit for bit.

  1. M <= 64, the parent's one-population cases: both forms on ONE manager, each at the bar; the largest difference between them is
     printed in units of the bar.  describe()["score_form"] / ["score_park"] follow the last call.
  2. beyond 64 states: binned rows with spans 65, 129 and 200 among them, which the plan cuts into pieces (k_score_select adds the
     pieces of a caller's row up for the first time), at M = 65 (two states per lane, 63 of the second dead), 128, 129 (three), 193
     and 256 (four); un-binned rows of up to 1000 positions at M = 128 (fp64 checkpoints).  Q keeps its device route.
  3. the same bits under SMCPP_SCORE_WAVES = 1, 2, 3 and unset, on repetition, with other products in between, under every selection.
  4. the same bits on a manager whose every fresh float allocation was filled with NaN (dead lanes, parked blocks, checkpoints).
  5. refusals, each before any launch, each leaving the manager usable.
  6. evidence.score_track(form="vectors"), information, covariance at M = 128.

The oracle does dense M^2 work per position: the cases beyond 64 states stay below 10 000 positions (a few seconds each)."""
import math
import os

import numpy as np
import pytest

import scoreref
import test_gpu_gamma as tg
import test_gpu_score_track as st
from test_gpu_parity import GAMMA_TOL, STAT_TOL

pytestmark = pytest.mark.gpu

SMALL = ["binned:M64", "unbinned:M32", "unbinned:M64", "binned:M1", "binned:M2", "binned:M5", "binned:M63", "seeds1:M13", "seeds3:M64"]
BIG = ["cut:M65", "cut:M128", "cut:M129", "cut:M193", "cut:M256", "long:M128"]
SPANS_CUT = (2, 63, 64, 65, 129, 200)
SPANS_LONG = (64, 65, 128, 129, 1000)
MAX_BIG = 10_000

_BIG_INPUTS = {}


def big_inputs(case):
    kind, M = case.split(":M")
    M = int(M)
    if kind not in _BIG_INPUTS:
        if kind == "cut":
            cs = tg.binned_contigs(41, 300_000, spans=SPANS_CUT)
            r = (cs, tg.TH_B, tg.RH_B)
        else:
            cs = tg.unbinned_contigs(100, seeds=(11,), spans=SPANS_LONG, cap=200)
            r = (cs, tg.TH_U, tg.RH_U)
        want = SPANS_CUT if kind == "cut" else SPANS_LONG
        assert all(s in set(cs[0][:, 0]) for s in want)
        assert sum(int(c[:, 0].sum()) for c in cs) <= MAX_BIG, sum(int(c[:, 0].sum()) for c in cs)
        assert any(len(c) == 1 for c in cs) and any(len(c) == 2 for c in cs)
        _BIG_INPUTS[kind] = r
    return (kind, M) + _BIG_INPUTS[kind]


def big_manager(case, estep=True, differentiable=True, save_gamma=True):
    """A one-population manager beyond 64 states, differentiable, after a save_gamma E-step; the plan is what the case is there for."""
    kind, M, contigs, theta, rho = big_inputs(case)
    im = tg._onepop(M, contigs, theta, rho)
    if differentiable:
        im.model.differentiable = True
        im.model.update_observers("model update")
    im.save_gamma = bool(save_gamma)
    if estep:
        im.E_step()
        plan = im.describe()["plan"]
        print(f"{case}: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family', 'rows', 'positions')} }")
        assert plan["states_per_lane"] == (M + 63) // 64, plan
        assert bool(plan["long_rows_cut"]) == (kind == "cut"), plan
    return im, contigs


def form_of(im):
    d = im.describe()
    return d["score_form"], d["score_park"]


def q_sums(im, contigs, got, refs, jac, case, label):
    """The three parts summed over every column of every contig against rows 0, 1 + 2, 3 of Q's Jacobian (test_gpu_score_track has
    the weights of the initial part): STAT_TOL of sum |oracle|."""
    nder = refs[0].shape[1]
    mass = [float(im.posterior_columns(c, 0, 1, normalize=False).sum()) for c in range(len(contigs))]
    weight = lambda m: np.array([m, 1.0, 1.0])[:, None]                                   # noqa: E731
    sums = np.sum([weight(m) * st.fsum_rows(g[0].reshape(3 * nder, -1)).reshape(3, nder) for g, m in zip(got, mass)], axis=0)
    mag = np.sum([weight(m) * np.abs(r).sum(axis=2) for r, m in zip(refs, mass)], axis=0)
    want = np.stack([jac[0], jac[1] + jac[2], jac[3]])
    rel = np.abs(sums - want) / np.maximum(mag, 1e-300)
    rel = np.where(mag == 0.0, np.where(sums == want, 0.0, np.inf), rel)
    print(f"{case} {label}: sum over columns against Q's Jacobian, by part {[float(f'{rel[x].max():.3g}') for x in range(3)]} of "
          f"sum |oracle| (bar {STAT_TOL})")
    assert np.all(rel <= STAT_TOL), (case, label, rel.max(axis=1))


def all_rows(im, nc):
    return [(im.score_rows(c, parts=True), im.score_rows(c)) for c in range(nc)]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. both forms at M <= 64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL)
def test_both_forms_on_the_parents_cases(engine_opt, case):
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", None)
    im, contigs = st.manager(case)
    nc = len(contigs)
    im.Q_with_gradient()
    before = im.describe()["q_route"]
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    vec = all_rows(im, nc)
    assert form_of(im) == ("vectors", "global")
    engine_opt("SMCPP_SCORE_FORM", "matrix")
    mat = all_rows(im, nc)
    assert form_of(im) == ("matrix", "lds")
    engine_opt("SMCPP_SCORE_FORM", None)
    assert np.array_equal(im.score_rows(0), mat[0][1]) and form_of(im) == ("matrix", "lds")        # unset means matrix
    q, jac = im.Q_with_gradient()
    route = im.describe()["q_route"]
    print(f"{case}: q_route before / after the score calls: {before} / {route}")
    assert route == before and (route == "device" or case != "binned:M64"), (before, route)
    refs, scales = st.oracle(case, im, contigs)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    worst, apart = 0.0, 0.0
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        worst = max(worst, st.check_columns(vec[c][0], vec[c][1], refs[c], scales[c], label + " vectors"))
        st.check_columns(mat[c][0], mat[c][1], refs[c], scales[c], label + " matrix")
        st.check_windows(im, c, vec[c][1], ob[:, 0], label)
        st.check_selections(im, c, vec[c][0], vec[c][1], len(ob), label)
        assert form_of(im) == ("vectors", "global")
        apart = max(apart, float((np.abs(vec[c][0] - mat[c][0]) / np.maximum(GAMMA_TOL * scales[c][None], 1e-300)).max()))
    q_sums(im, contigs, vec, refs, jac, case, "vectors")
    q_sums(im, contigs, mat, refs, jac, case, "matrix")
    print(f"{case}: WORST column of the vectors form {worst:.3g} of the bar; the two forms are at most {apart:.3g} of the bar apart")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. beyond 64 states
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BIG)
def test_beyond_64_states(engine_opt, case):
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    # (an input this small is cut whatever its rows look like: the un-binned case asks for whole rows, as a genome-sized one gets them)
    engine_opt("SMCPP_SPLIT_SPANS", "0" if case.startswith("long") else None)
    im, contigs = big_manager(case)
    nc = len(contigs)
    im.Q_with_gradient()
    before = im.describe()["q_route"]
    got = all_rows(im, nc)
    assert form_of(im) == ("vectors", "global")
    d = im.describe()
    if case.startswith("cut"):
        assert d["score_items"] > len(contigs[nc - 1]), d                     # engine rows: the pieces, not the caller's rows
    q, jac = im.Q_with_gradient()
    route = im.describe()["q_route"]
    # (un-binned rows crossed by eigen-power steps send Q to the host before and after, as on the parent's un-binned cases)
    assert route == before and (route == "device" or case.startswith("long")), (before, route)
    refs, scales = st.oracle(case, im, contigs)
    worst = 0.0
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        worst = max(worst, st.check_columns(got[c][0], got[c][1], refs[c], scales[c], label))
        st.check_windows(im, c, got[c][1], ob[:, 0], label)
        st.check_selections(im, c, got[c][0], got[c][1], len(ob), label)
    q_sums(im, contigs, got, refs, jac, case, "vectors")
    print(f"{case}: WORST column {worst:.3g} of the bar")
    assert all(np.abs(refs[0][x]).max() > 0.0 for x in range(3))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cut:M65", "cut:M256"])
def test_same_bits(engine_opt, case):
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    im, contigs = big_manager(case)
    nc = len(contigs)
    good = [st.products(im, c) for c in range(nc)]
    for c in range(nc):
        st.same_bits(st.products(im, c), good[c])                             # repetition
    im.score_rows(0)
    items = im.describe()["score_items"]
    assert items > len(contigs[0]) > 3 * 3
    for waves in ("1", "2", "3", None):                                       # a wavefront's second and third row and beyond
        engine_opt("SMCPP_SCORE_WAVES", waves)
        for c in range(nc):
            st.same_bits(st.products(im, c), good[c])
        im.score_rows(0)
        d = im.describe()
        assert (3 < d["score_waves"] <= min(items, 4096) if waves is None else d["score_waves"] == int(waves)) and d["score_items"] == items, d
    for c in range(nc):                                                       # other products in between, and they unchanged
        tr = im.posterior_transitions(c)
        llr = im.loglik_rows(c)
        im.posterior_columns(c, normalize=False)
        im.posterior_sample_rows(c, n_paths=2, seed=1)
        st.same_bits(st.products(im, c), good[c])
        tr2 = im.posterior_transitions(c)
        assert all(np.array_equal(tr[k], tr2[k]) for k in tr) and np.array_equal(im.loglik_rows(c), llr)
        st.check_selections(im, c, good[c]["parts"], good[c]["rows"], len(contigs[c]), f"{case} contig {c}")
    im.E_step()                                                               # a repeated E-step on the same parameters
    for c in range(nc):
        st.same_bits(st.products(im, c), good[c])


@pytest.mark.parametrize("case", ["cut:M65", "cut:M129"])
def test_poisoned_memory(engine_opt, case):
    from smcpp_amd import _engine
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    im, contigs = big_manager(case)
    good = [st.products(im, c) for c in range(len(contigs))]
    _engine.set_option("SMCPP_DEBUG_POISON", "nan")
    try:
        im2, _ = big_manager(case)
        for waves in (None, "2"):
            engine_opt("SMCPP_SCORE_WAVES", waves)
            for c in range(len(contigs)):
                st.same_bits(st.products(im2, c), good[c])
    finally:
        _engine.set_option("SMCPP_DEBUG_POISON", None)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine_opt):
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    case = "cut:M65"
    im, contigs = big_manager(case)
    L, nc = len(contigs[0]), len(contigs)
    good = st.products(im, 0)

    def raises(call, match, usable=im, want=good):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip()
        if usable is not None:
            st.same_bits(st.products(usable, 0), want)

    both = lambda m, c=0: (lambda: m.score_rows(c), lambda: m.score_rows(c, parts=True), lambda: m.score_windows(c, 100))    # noqa: E731
    # what the matrix form refuses as well, but for the state count
    for c in (-1, nc):
        for call in both(im, c):
            raises(call, "contig")
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(step=0)):
        raises(lambda: im.score_rows(0, **kw), "start|stop|step|selection")
    raises(lambda: im.score_windows(0, 0), "window_bp")
    fresh, _ = big_manager(case, estep=False, save_gamma=False)
    for call in both(fresh):
        raises(call, "no E-step", None)
    fresh.E_step()
    for call in both(fresh):
        raises(call, "save_gamma", None)
    fresh.save_gamma = True
    fresh.E_step()
    st.same_bits(st.products(fresh, 0), good)
    fresh.theta = 2 * tg.TH_B
    for call in both(fresh):
        raises(call, "set again", None)
    fresh.theta = tg.TH_B
    fresh.E_step()
    st.same_bits(st.products(fresh, 0), good)
    plain, _ = big_manager(case, differentiable=False)
    for call in both(plain):
        raises(call, "no derivative seeds", None)
    # a value of the switch the engine does not know
    engine_opt("SMCPP_SCORE_FORM", "columns")
    for call in both(im):
        raises(call, "SMCPP_SCORE_FORM", None)
    # the switch unset: the matrix form, which stops at 64 states (its message is the parent's to the letter)
    engine_opt("SMCPP_SCORE_FORM", None)
    for call in both(im):
        raises(call, "64 hidden states", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    st.same_bits(st.products(im, 0), good)
    # more than 256 states: eight states per lane
    _, _, cs, theta, rho = big_inputs(case)
    huge = tg._onepop(257, cs, theta, rho)
    huge.model.differentiable = True
    huge.model.update_observers("model update")
    huge.save_gamma = True
    huge.E_step()
    assert huge.describe()["plan"]["states_per_lane"] == 8
    for call in both(huge):
        raises(call, "256 hidden states", None)
    assert huge.posterior_transitions(0)["stay"].shape == (L + 1,)
    # no generator planes: a model prepared on the host (M <= 64: the message names the matrix form, and the matrix form answers) ...
    engine_opt("SMCPP_PREP", "host")
    hosted, hc = st.manager("binned:M5")
    engine_opt("SMCPP_SCORE_FORM", None)
    hgood = st.products(hosted, 0)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    for call in both(hosted):
        raises(call, "generator planes.*matrix form", None)
    engine_opt("SMCPP_SCORE_FORM", None)
    st.same_bits(st.products(hosted, 0), hgood)
    engine_opt("SMCPP_PREP", None)
    # ... and a two-population manager
    two, _ = st.manager("twopop:M48")
    tgood = st.products(two, 0)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    for call in both(two):
        raises(call, "generator planes.*two-population", None)
    engine_opt("SMCPP_SCORE_FORM", None)
    st.same_bits(st.products(two, 0), tgood)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    st.same_bits(st.products(im, 0), good)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Python glue
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evidence_in_the_vectors_form(engine_opt):
    from smcpp_amd import synth
    from smcpp_amd.evidence import covariance, information, score_track
    from smcpp_amd.model import PiecewiseModel
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", None)
    _, M, contigs, theta, rho = big_inputs("cut:M128")
    a, s = synth.model_pieces()
    model = PiecewiseModel(a, s, 1e4, "pop1")
    model.differentiable = True
    body = [c for c in contigs if len(c) > 2]
    with pytest.raises(RuntimeError, match="64 hidden states"):
        score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100)
    with pytest.raises(ValueError, match="form"):
        score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, form="columns")
    hs, track, im = score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, return_manager=True, form="vectors")
    assert "SMCPP_SCORE_FORM" not in os.environ and "SMCPP_SCORE_FORM" not in im.describe()["options"]      # put back
    assert form_of(im) == ("vectors", "global")
    assert len(track) == len(body) and all(t.shape[0] == len(a) and t.dtype == np.float64 for t in track)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    for c in range(len(body)):
        assert np.array_equal(track[c], im.score_windows(c, 100))
    _, jac = im.Q_with_gradient()
    info = information(track, block=5)
    mag = np.sum([np.abs(im.score_rows(c, parts=True)).sum(axis=(0, 2)) for c in range(len(body))], axis=0)
    u0 = np.sum([im.score_rows(c, 0, 1, parts=True)[0, :, 0] for c in range(len(body))], axis=0)
    assert np.all(np.abs(info["score"] - u0 - jac[1:].sum(axis=0)) <= STAT_TOL * mag), (info["score"], u0, jac[1:].sum(axis=0))
    cov = covariance(info)
    assert cov["cov"].shape == (len(a), len(a)) and np.all(np.isfinite(cov["se"])) and np.all(cov["se"] >= 0.0)
    assert math.isfinite(float(np.abs(info["J"]).max())) and scoreref.EPS > 0.0
