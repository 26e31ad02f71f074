"""EXACT windows of the score track on the device - `score_windows_exact` (smcpp_score_windows_exact;
smcpp_amd/csrc/score_seg_dev.hpp): a row that a window boundary cuts strictly inside gives every window the score of the positions
that lie in it, where `score_windows` spreads the row's total evenly over its base pairs.

Truth: tests/scorewin_ref.py - tests/scoreref.py on the rows expanded into rows of span 1, from the manager's own getters, added up by
window; the bar GAMMA_TOL B_w is test_gpu_score_track's GAMMA_TOL B[l, d] split by positions (scorewin_ref has the formula).  Managers,
getters and engine_opt as tests/test_gpu_score_vectors.py builds them; every input stays below 10 000 positions; every case runs
under SMCPP_SCORE_FORM=vectors.

  1. every window and direction against the oracle at W = 1 (every position its own segment), 7 (several flushes per block), 64 and
     65 (boundaries at and beside block and piece seams), 100, N - 1 (the last window is one base pair) and N (no item: the segment
     kernel is not launched, and the result is score_windows' within its own bar), on every contig - the one-row and the two-row
     contig included - of: un-binned rows at M = 32 and 64, binned rows at M = 5 and 63, rows cut into pieces at M = 65, 129 and 256
     (spans 2, 63, 64, 65, 129, 200), un-binned rows of up to 1000 positions at M = 128 (fp64 checkpoints)
  2. the gap is real: on the un-binned input score_windows is beyond 10 GAMMA_TOL B_w of the oracle where the exact call is within
     the bar
  3. the exact windows sum (math.fsum) to the rows' sum; on the expanded rows as the manager's data no row can be cut and exact and
     plain windows agree, both within the window bar of test_gpu_score_track
  4. the same bits under SMCPP_SCORE_WAVES = 1, 2, 3 and unset (items exceed wavefronts), on repetition, with other products in
     between (which keep their bits as well)
  5. the same bits on a manager whose fresh allocations were filled with 0xFF bytes
  6. refusals, each before any launch, each leaving the manager usable
  7. evidence.score_track(exact=True), information, covariance at M = 128

The oracle does dense M^2 work per POSITION (the expansion has no rows to add up first): 6 s at M = 256, once per case."""
import math
import os

import numpy as np
import pytest

import scoreref
import scorewin_ref
import test_gpu_gamma as tg
import test_gpu_score_track as st
import test_gpu_score_vectors as sv
import transref
from test_gpu_parity import GAMMA_TOL

pytestmark = pytest.mark.gpu

EPS = scoreref.EPS
CASES = ["unbinned:M32", "unbinned:M64", "binned:M5", "binned:M63", "cut:M65", "cut:M129", "cut:M256", "long:M128"]
MAX_POSITIONS = 10_000
GAP_W = 100

_ORACLE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# managers and the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def setup(engine_opt, case):
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    # (an input this small is cut whatever its rows look like: the un-binned cases ask for whole rows, as a genome-sized one gets them)
    engine_opt("SMCPP_SPLIT_SPANS", "0" if case.split(":")[0] in ("long", "unbinned") else None)


def manager(case, **kw):
    """-> (im, contigs): differentiable, after a save_gamma E-step, as test_gpu_score_vectors / test_gpu_score_track build them; the
    un-binned cases on scorewin_ref.unbinned_input()."""
    kind, M = case.split(":M")
    if kind == "binned":
        im, contigs = st.manager(case, **kw)
    elif kind in ("cut", "long"):
        im, contigs = sv.big_manager(case, **kw)
    else:
        contigs, theta, rho = scorewin_ref.unbinned_input()
        im = tg._onepop(int(M), contigs, theta, rho)
        im.model.differentiable = True
        im.model.update_observers("model update")
        im.save_gamma = True
        im.E_step()
        plan = im.describe()["plan"]
        assert plan["states_per_lane"] == 1 and not plan["long_rows_cut"], plan
    assert sum(int(c[:, 0].sum()) for c in contigs) <= MAX_POSITIONS
    assert any(len(c) == 1 for c in contigs) and any(len(c) == 2 for c in contigs)
    return im, contigs


def oracle(case, im, contigs):
    """Per contig (u [nder, N + 1], b [nder, N + 1]): the score and the bar scale per position (scorewin_ref.positions), from the
    manager's getters; once per case and process, never changed."""
    if case not in _ORACLE:
        dpi, dT, dE = st.jacobians(im)
        pi, T, keys, Et = im.pi, im.transition, im.keys, transref.emission_table(im)
        out = []
        for ob in contigs:
            u, b = scorewin_ref.positions(pi, T, keys, Et, dpi, dT, dE, ob)
            u.setflags(write=False)
            b.setflags(write=False)
            out.append((u, b))
        _ORACLE[case] = out
    return _ORACLE[case]


def widths(N):
    return sorted({W for W in (1, 7, 64, 65, 100, N - 1, N) if 1 <= W})


def exact_items(im):
    d = im.describe()
    return d["score_exact_items"], d["score_exact_segments"], d["score_exact_waves"]


def window_bar(v, spans, W):
    """The bar of test_gpu_score_track.check_windows: (W + 8) 2^-52 of the sum of |terms| of the apportioned windows."""
    _, mag = scoreref.score_windows(v, spans, W)
    return (W + 8) * EPS * mag


def exact_products(im, c):
    return {"x7": im.score_windows_exact(c, 7), "x100": im.score_windows_exact(c, 100)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_window_against_the_oracle(engine_opt, case):
    setup(engine_opt, case)
    im, contigs = manager(case)
    ref = oracle(case, im, contigs)
    worst, walked = 0.0, 0
    for c, ob in enumerate(contigs):
        u, b = ref[c]
        spans = ob[:, 0]
        N = int(spans.sum())
        for W in widths(N):
            got = im.score_windows_exact(c, W)
            items, segs, waves = exact_items(im)
            want, B = scorewin_ref.window_sums(u, W), scorewin_ref.window_sums(b, W)
            assert got.dtype == np.float64 and got.shape == want.shape == (u.shape[0], -(-N // W)), (case, c, W, got.shape)
            assert np.all(np.isfinite(got)), (case, c, W)
            ratio = np.abs(got - want) / (GAMMA_TOL * B)
            worst = max(worst, float(ratio.max()))
            print(f"{case} contig {c} (N = {N}), W = {W}: {items} items, {segs} segments, {waves} wavefronts; worst |value - oracle| "
                  f"{ratio.max():.3g} of GAMMA_TOL B_w")
            bad = np.argwhere(ratio > 1.0)
            assert len(bad) == 0, f"{case} contig {c}, W = {W}: {len(bad)} windows beyond the bar, e.g. (direction, window) {bad[:6].tolist()}"
            assert (items == 0) == (waves == 0) and segs >= 2 * items, (items, segs, waves)
            walked += items
            if W == N:
                # one window: no boundary, no item, the segment kernel is not launched; score_windows adds the same rows
                assert items == 0 and waves == 0, (case, c, items, waves)
                plain = im.score_windows(c, W)
                tol = window_bar(im.score_rows(c), spans, W)
                assert np.all(np.abs(got - plain) <= tol), (case, c, float(np.max(np.abs(got - plain) / np.maximum(tol, 1e-300))))
            if W == 1 and N > 1:
                # every engine row of more than one position is an item and every position of it a segment (where the plan cut the
                # caller's rows the engine rows are the pieces: no fewer items, and a piece of one position is none)
                long_rows = spans[spans > 1]
                if case.startswith("cut"):
                    assert items >= len(long_rows) and 2 * items <= segs <= int(long_rows.sum()), (items, segs)
                else:
                    assert (items, segs) == (len(long_rows), int(long_rows.sum())), (items, segs)
    print(f"{case}: WORST window {worst:.3g} of the bar; {walked} items walked in all")
    assert walked > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the gap is real
# ---------------------------------------------------------------------------------------------------------------------------------
def test_apportioned_windows_miss_what_exact_windows_hold(engine_opt):
    case = "unbinned:M32"
    setup(engine_opt, case)
    im, contigs = manager(case)
    u, b = oracle(case, im, contigs)[0]
    want, B = scorewin_ref.window_sums(u, GAP_W), scorewin_ref.window_sums(b, GAP_W)
    plain = np.abs(im.score_windows(0, GAP_W) - want) / (GAMMA_TOL * B)
    exact = np.abs(im.score_windows_exact(0, GAP_W) - want) / (GAMMA_TOL * B)
    beyond = (plain > 10.0).any(axis=0)
    print(f"{case}, W = {GAP_W}: score_windows worst {plain.max():.3g} of GAMMA_TOL B_w, {int(beyond.sum())} of {len(beyond)} windows "
          f"beyond 10; score_windows_exact worst {exact.max():.3g}, there {exact[:, beyond].max() if beyond.any() else 0.0:.3g}")
    assert beyond.any(), plain.max()
    assert exact.max() <= 1.0 and np.all(exact[:, beyond] <= 1.0), exact.max()
    assert exact_items(im)[0] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. consistency
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unbinned:M32", "cut:M65"])
def test_windows_sum_to_the_rows(engine_opt, case):
    setup(engine_opt, case)
    im, contigs = manager(case)
    for c, ob in enumerate(contigs):
        v = im.score_rows(c)
        N = int(ob[:, 0].sum())
        for W in sorted({min(100, N), N}):
            got = im.score_windows_exact(c, W)
            _, mag = scoreref.score_windows(v, ob[:, 0], W)
            serr = np.abs(st.fsum_rows(got) - st.fsum_rows(v))
            bar = (W + 8) * EPS * st.fsum_rows(mag)
            print(f"{case} contig {c}, W = {W}: the exact windows miss the rows' sum by {np.max(serr / np.maximum(st.fsum_rows(mag), 1e-300)) / EPS:.2f} "
                  f"eps of sum |terms| (bar {W + 8})")
            assert np.all(serr <= bar), (case, c, W)


def test_expanded_rows_cannot_be_cut(engine_opt):
    case = "cut:M65"
    setup(engine_opt, case)
    _, M, contigs, theta, rho = sv.big_inputs(case)
    expanded = [scorewin_ref.expand(c) for c in contigs]
    im = tg._onepop(M, expanded, theta, rho)
    im.model.differentiable = True
    im.model.update_observers("model update")
    im.save_gamma = True
    im.E_step()
    for c, ob in enumerate(expanded):
        N = len(ob)
        v = im.score_rows(c)
        for W in widths(N):
            got, plain = im.score_windows_exact(c, W), im.score_windows(c, W)
            assert exact_items(im) == (0, 0, 0), (c, W, exact_items(im))
            tol = window_bar(v, ob[:, 0], W)
            assert got.shape == plain.shape and np.all(np.abs(got - plain) <= tol), (c, W, float(np.max(np.abs(got - plain) / np.maximum(tol, 1e-300))))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_same_bits(engine_opt):
    case = "cut:M65"
    setup(engine_opt, case)
    im, contigs = manager(case)
    nc = len(contigs)
    good = [exact_products(im, c) for c in range(nc)]
    for c in range(nc):
        st.same_bits(exact_products(im, c), good[c])                          # repetition
    im.score_windows_exact(0, 7)
    items, segs, waves = exact_items(im)
    assert items > 3 * 3 and waves == min(items, 4096) and segs > 2 * items, (items, segs, waves)
    for w in ("1", "2", "3", None):                                           # a wavefront's second and third item and beyond
        engine_opt("SMCPP_SCORE_WAVES", w)
        for c in range(nc):
            st.same_bits(exact_products(im, c), good[c])
        im.score_windows_exact(0, 7)
        got = exact_items(im)
        assert got == (items, segs, min(items, 4096) if w is None else int(w)) and (w is None or items > int(w)), (w, got)
    for c in range(nc):                                                       # other products in between, and they unchanged
        rows, llw, pwx = im.score_rows(c, parts=True), im.loglik_windows(c, 7), im.posterior_windows_exact(c, 7)
        plain = im.score_windows(c, 7)
        st.same_bits(exact_products(im, c), good[c])
        assert np.array_equal(im.score_rows(c, parts=True), rows) and np.array_equal(im.loglik_windows(c, 7), llw)
        assert np.array_equal(im.posterior_windows_exact(c, 7), pwx) and np.array_equal(im.score_windows(c, 7), plain)
        st.same_bits(exact_products(im, c), good[c])
        # (the loglik track keeps its own table: its describe keys are those of ITS last call)
        im.loglik_windows(c, 7)
        ll_items = im.describe()["ll_items"]
        im.score_windows_exact(c, 100)
        assert im.describe()["ll_items"] == ll_items
    im.E_step()                                                               # a repeated E-step on the same parameters
    for c in range(nc):
        st.same_bits(exact_products(im, c), good[c])


@pytest.mark.parametrize("case", ["cut:M65", "long:M128"])
def test_poisoned_memory(engine_opt, case):
    setup(engine_opt, case)
    im, contigs = manager(case)
    good = [exact_products(im, c) for c in range(len(contigs))]
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im2, _ = manager(case)
    for w in (None, "2"):
        engine_opt("SMCPP_SCORE_WAVES", w)
        for c in range(len(contigs)):
            st.same_bits(exact_products(im2, c), good[c])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine_opt):
    case = "cut:M65"
    setup(engine_opt, case)
    im, contigs = manager(case)
    nc = len(contigs)
    good = exact_products(im, 0)

    def raises(call, match, usable=im):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip()
        if usable is not None:
            st.same_bits(exact_products(usable, 0), good)

    # the matrix form, named or by default: refused with the switch that serves the call
    for form in (None, "matrix"):
        engine_opt("SMCPP_SCORE_FORM", form)
        raises(lambda: im.score_windows_exact(0, 100), "SMCPP_SCORE_FORM=vectors", None)
    small, _ = st.manager("binned:M5")                                        # (M <= 64, where the matrix form serves score_windows)
    raises(lambda: small.score_windows_exact(0, 100), "SMCPP_SCORE_FORM=vectors", None)
    assert small.score_windows(0, 100).shape[0] == 16
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    st.same_bits(exact_products(im, 0), good)
    for c in (-1, nc):
        raises(lambda: im.score_windows_exact(c, 100), "contig")
    for W in (0, -5):
        raises(lambda: im.score_windows_exact(0, W), "window_bp")
    fresh, _ = sv.big_manager(case, estep=False, save_gamma=False)
    raises(lambda: fresh.score_windows_exact(0, 100), "no E-step", None)
    fresh.E_step()
    raises(lambda: fresh.score_windows_exact(0, 100), "save_gamma", None)
    fresh.save_gamma = True
    fresh.E_step()
    st.same_bits(exact_products(fresh, 0), good)
    fresh.theta = 2 * tg.TH_B
    raises(lambda: fresh.score_windows_exact(0, 100), "set again.*run the E-step again", None)
    fresh.theta = tg.TH_B
    fresh.E_step()
    st.same_bits(exact_products(fresh, 0), good)
    plain, _ = sv.big_manager(case, differentiable=False)
    raises(lambda: plain.score_windows_exact(0, 100), "no derivative seeds.*set them with seeds", None)
    _, _, cs, theta, rho = sv.big_inputs(case)
    huge = tg._onepop(257, cs, theta, rho)
    huge.model.differentiable = True
    huge.model.update_observers("model update")
    huge.save_gamma = True
    huge.E_step()
    raises(lambda: huge.score_windows_exact(0, 100), "256 hidden states.*fewer hidden states", None)
    st.same_bits(exact_products(im, 0), good)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the Python glue
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evidence_with_exact_windows(engine_opt):
    from smcpp_amd import synth
    from smcpp_amd.evidence import covariance, information, score_track
    from smcpp_amd.model import PiecewiseModel
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", None)
    _, M, contigs, theta, rho = sv.big_inputs("cut:M128")
    a, s = synth.model_pieces()
    model = PiecewiseModel(a, s, 1e4, "pop1")
    model.differentiable = True
    body = [c for c in contigs if len(c) > 2]
    with pytest.raises(ValueError, match="vectors"):
        score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, exact=True, form="matrix")
    hs, track, im = score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, return_manager=True, exact=True)
    assert "SMCPP_SCORE_FORM" not in os.environ and "SMCPP_SCORE_FORM" not in im.describe()["options"]      # put back
    assert sv.form_of(im) == ("vectors", "global") and exact_items(im)[0] > 0
    assert len(track) == len(body) and all(t.shape[0] == len(a) and t.dtype == np.float64 for t in track)
    _, track2 = score_track(model, body, synth.hidden_states(M), tg.N, theta, rho, 100, exact=True, form="vectors")
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    for c in range(len(body)):
        assert np.array_equal(track[c], im.score_windows_exact(c, 100)) and np.array_equal(track2[c], track[c])
        assert not np.array_equal(track[c], im.score_windows(c, 100))
    info = information(track, block=5)
    cov = covariance(info)
    assert info["J"].shape == (len(a), len(a)) and math.isfinite(float(np.abs(info["J"]).max()))
    assert cov["cov"].shape == (len(a), len(a)) and np.all(np.isfinite(cov["se"])) and np.all(cov["se"] >= 0.0)
