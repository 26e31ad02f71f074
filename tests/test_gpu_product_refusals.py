"""The exact text of every refusal of the product calls (smcpp_posterior_*, smcpp_loglik_rows / _positions / _windows, smcpp_score_*,
smcpp_simulate; smcpp_amd/csrc/engine_products.hpp).  The other product suites match on substrings; here `str(e)` is compared with the
whole message, and where two checks of one call both fail, with the message of the one that comes first: the texts and their order
are part of the C ABI (smcpp_last_error hands them to both bindings).

Every case is a call that throws before anything is launched.  The managers are those of the products' own refusal tests: the two
small un-binned contigs of test_gpu_loglik_track (15 and 7 rows, spans up to 500) at M = 8 with a differentiable model; the same
without derivative seeds; `set_raw` with an arbitrary matrix; M = 65; and for the caps of 2^31 - 1 elements and 1 GiB of scratch
the un-binned rows of test_gpu_score_track (one row of 2 10^8 positions; 1400 rows of 10^5) and test_gpu_loglik_track (rows of
10^9 positions, nine of them here: the transition windows refuse beyond 4 (2^31 - 1) windows), which an E-step crosses by
eigen-power steps.  Calls with `out == NULL` go to the C ABI directly: which of them refuse and which return the window count is
decided by where a cap check stands relative to `if (!out) return 0`.

Not reached: "the generators of T are missing", "the transition matrix is missing", "the Jacobians of pi, T and E are not
available" (states no sequence of calls produces), "more than 2^31 - 1 segments of cut rows" (the cap on the windows refuses
first) and the score track's cap on "the outputs" (4.4 10^7 rows at the least)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_gamma as tg
import test_gpu_loglik_track as tl
import transref

pytestmark = pytest.mark.gpu

PP = "posterior products: "
CONTIG = "contig index out of range"
DIRTY = ("posterior transitions: the parameters were set again after the last E-step, whose stored vectors belong to the earlier ones: "
         "run the E-step again")
UNSTRUCTURED = ("posterior transitions: the transition matrix does not have the semiseparable structure of the model's (smcpp_set_raw "
                "with an arbitrary matrix): the O(M) steps that walk a row's interior do not exist for it")
CAP_PATHS = " exceed the cap of 2^31 - 1 elements per call: ask for fewer paths or a narrower window"
CAP_POS = " exceed the cap of 2^31 - 1 elements per array: ask for a narrower or a coarser grid"
CAP_LL = " exceed the cap of 2^31 - 1 elements per call: ask for a narrower or a coarser grid, or a wider window"
CAP_SC = " exceed the cap of 2^31 - 1 elements per call: ask for a narrower selection or a wider window"
BIG = 2 ** 31 - 1


def small(differentiable=True, save_gamma=True, estep=True):
    cs = tl.two_contigs()
    im = tg._onepop(8, cs, tg.TH_B, tg.RH_B, n=tl.N4)
    if differentiable:
        im.model.differentiable = True
        im.model.update_observers("model update")
    im.save_gamma = save_gamma
    if estep:
        im.E_step()
    return im, cs


def check(table):
    """table: (label, call, expected message); every case runs, the differences are shown together."""
    wrong = []
    for label, call, want in table:
        try:
            call()
            got = None
        except RuntimeError as e:
            got = str(e)
        if got != want:
            wrong.append((label, got, want))
    for label, got, want in wrong:
        print(f"{label}:\n  got   {got!r}\n  want  {want!r}")
    assert not wrong, [w[0] for w in wrong]


def lib():
    from smcpp_amd import _engine
    return _engine.lib()


def rc_of(rc):
    """The C ABI's return code -> the message, or None where the call did not refuse."""
    return None if rc == 0 else lib().smcpp_last_error().decode()


def every_call(im, c=0):
    """One plain call of every product entry point: (name, call)."""
    return [("columns", lambda: im.posterior_columns(c)), ("summary", lambda: im.posterior_summary(c)),
            ("windows", lambda: im.posterior_windows(c, 100)), ("transitions", lambda: im.posterior_transitions(c)),
            ("transition_windows", lambda: im.posterior_transition_windows(c, 100)),
            ("sample_rows", lambda: im.posterior_sample_rows(c)), ("sample_positions", lambda: im.posterior_sample_positions(c)),
            ("positions", lambda: im.posterior_positions(c)), ("position_summary", lambda: im.posterior_position_summary(c)),
            ("windows_exact", lambda: im.posterior_windows_exact(c, 100)),
            ("loglik_rows", lambda: im.loglik_rows(c)), ("loglik_positions", lambda: im.loglik_positions(c)),
            ("loglik_windows", lambda: im.loglik_windows(c, 100)),
            ("score_rows", lambda: im.score_rows(c)), ("score_windows", lambda: im.score_windows(c, 100))]


POSTERIOR = ("columns", "summary", "windows", "transitions", "transition_windows", "sample_rows", "sample_positions", "positions",
             "position_summary", "windows_exact")
WALKS = ("transitions", "transition_windows", "sample_rows", "sample_positions", "positions", "position_summary", "windows_exact",
         "loglik_positions", "loglik_windows")


def test_arguments():
    """Contig, selection, grid, window, quantile, weight and path-count refusals on a manager every product serves."""
    from smcpp_amd import _engine
    im, cs = small()
    L, N, nc, M = len(cs[0]), int(cs[0][:, 0].sum()), len(cs), im.M
    assert (L, N, M) == (15, 739, 8) and cs[0][:, 0].max() > 64
    t = []
    for c in (-1, nc):
        t += [(f"{name} contig {c}", call, CONTIG) for name, call in every_call(im, c)]
    # the column selection is the posterior products' in every call that takes one
    sel = [(dict(start=-1), PP + "start < 0"), (dict(stop=L + 2), PP + "stop > L + 1 (the contig has 16 columns)"),
           (dict(start=3, stop=3), PP + "empty column selection (start >= stop)"),
           (dict(start=4, stop=2), PP + "empty column selection (start >= stop)"), (dict(step=0), PP + "step < 1"),
           (dict(start=-1, stop=L + 2, step=0), PP + "start < 0"), (dict(stop=L + 2, step=0), PP + "stop > L + 1 (the contig has 16 columns)"),
           (dict(start=3, stop=3, step=0), PP + "empty column selection (start >= stop)")]
    for f in (im.posterior_columns, im.posterior_summary, im.posterior_transitions, im.posterior_sample_rows, im.loglik_rows, im.score_rows):
        t += [(f"{f.__name__} {kw}", lambda f=f, kw=kw: f(0, **kw), want) for kw, want in sel]
    # a grid of positions, a window of positions
    for who, fs in (("posterior positions: ", (im.posterior_positions, im.posterior_position_summary)), ("loglik track: ", (im.loglik_positions,))):
        grid = [(dict(pos0=-1), who + "pos0 < 0"), (dict(pos1=N + 2), who + "pos1 > P_L + 1 (the contig has 740 positions)"),
                (dict(pos0=3, pos1=3), who + "empty grid (pos0 >= pos1)"), (dict(pos0=N + 1), who + "empty grid (pos0 >= pos1)"),
                (dict(step=0), who + "step < 1"), (dict(pos0=-1, pos1=N + 2, step=0), who + "pos0 < 0"),
                (dict(pos1=N + 2, step=0), who + "pos1 > P_L + 1 (the contig has 740 positions)"),
                (dict(pos0=3, pos1=3, step=0), who + "empty grid (pos0 >= pos1)")]
        for f in fs:
            t += [(f"{f.__name__} {kw}", lambda f=f, kw=kw: f(0, **kw), want) for kw, want in grid]
    who = "posterior paths: "
    t += [(f"sample_positions {kw}", lambda kw=kw: im.posterior_sample_positions(0, **kw), want) for kw, want in (
        (dict(pos0=-1), who + "pos0 < 0"), (dict(pos1=N + 2), who + "pos1 > P_L + 1 (the contig has 740 positions)"),
        (dict(pos0=5, pos1=5), who + "empty window of positions (pos0 >= pos1)"),
        (dict(pos0=9, pos1=4), who + "empty window of positions (pos0 >= pos1)"), (dict(pos0=-1, pos1=N + 2), who + "pos0 < 0"))]
    # windows
    for W in (0, -5):
        t += [(f"windows {W}", lambda W=W: im.posterior_windows(0, W), "posterior windows: window_bp < 1"),
              (f"windows_exact {W}", lambda W=W: im.posterior_windows_exact(0, W), "posterior windows: window_bp < 1"),
              (f"transition_windows {W}", lambda W=W: im.posterior_transition_windows(0, W), "posterior transition windows: window_bp < 1"),
              (f"loglik_windows {W}", lambda W=W: im.loglik_windows(0, W), "loglik track: window_bp < 1"),
              (f"score_windows {W}", lambda W=W: im.score_windows(0, W), "score track: window_bp < 1")]
    # quantile levels and weights
    w_bad = np.linspace(0.0, 1.0, M)
    w_bad[4] = np.inf
    w_nan = np.ones(M)
    w_nan[0] = np.nan
    one = np.array([0.5])
    for who, f, cfn in (("posterior summary: ", im.posterior_summary, lambda q: lib().smcpp_posterior_summary(im._im, 0, 0, 1, 1, None, 1, q, None, None, None, None)),
                        ("posterior position summary: ", im.posterior_position_summary,
                         lambda q: lib().smcpp_posterior_position_summary(im._im, 0, 0, 1, 1, None, 1, q, None, None, None))):
        t += [(who + "9 levels", lambda f=f: f(0, quantiles=np.linspace(0.1, 0.9, 9)), who + "between 0 and 8 quantile levels"),
              (who + "no levels", lambda cfn=cfn: check_rc(cfn(None)), who + "quantile levels are missing"),
              (who + "weight 4", lambda f=f: f(0, weights=w_bad), who + "weight 4 is not finite"),
              (who + "weight 0", lambda f=f: f(0, weights=w_nan), who + "weight 0 is not finite"),
              (who + "level before weight", lambda f=f: f(0, weights=w_bad, quantiles=(0.5, 1.0)), who + "a quantile level must lie in (0, 1)")]
        t += [(who + f"level {q}", lambda f=f, q=q: f(0, quantiles=(0.5, q)), who + "a quantile level must lie in (0, 1)")
              for q in (0.0, 1.0, -0.5, 1.5, np.nan)]
        assert rc_of(cfn(_engine.dptr(one))) is None          # (no output asked for: the checks alone pass)
    t += [("summary: selection before level", lambda: im.posterior_summary(0, quantiles=(1.0,), step=0), PP + "step < 1"),
          ("position summary: grid before level", lambda: im.posterior_position_summary(0, quantiles=(1.0,), step=0), "posterior positions: step < 1")]
    # paths
    who = "posterior paths: "
    word = who + "first_path + n_paths > 2^31 (the path index is one 32-bit word of the counter)"
    for name, f in (("sample_rows", im.posterior_sample_rows), ("sample_positions", im.posterior_sample_positions)):
        t += [(f"{name} {kw}", lambda f=f, kw=kw: f(0, **kw), want) for kw, want in (
            (dict(n_paths=0), who + "n_paths < 1"), (dict(n_paths=-3, first_path=-1), who + "n_paths < 1"),
            (dict(first_path=-1), who + "first_path < 0"), (dict(first_path=BIG, n_paths=2), word), (dict(first_path=2 ** 31 + 1), word),
            (dict(n_paths=2 ** 31 + 1), word))]
    t += [("sample_rows outputs", lambda: im.posterior_sample_rows(0, n_paths=BIG), who + f"the outputs ({BIG} paths x 16)" + CAP_PATHS),
          ("sample_rows engine rows", lambda: im.posterior_sample_rows(0, n_paths=BIG, stop=1),
           who + f"the per-row products over the engine's rows ({BIG} paths x 16)" + CAP_PATHS),
          ("sample_positions outputs", lambda: im.posterior_sample_positions(0, n_paths=BIG), who + f"the outputs ({BIG} paths x 740)" + CAP_PATHS),
          ("sample_rows: selection before paths", lambda: im.posterior_sample_rows(0, n_paths=0, step=0), PP + "step < 1"),
          ("sample_positions: paths before window", lambda: im.posterior_sample_positions(0, n_paths=0, pos0=-1), who + "n_paths < 1")]
    check(t)
    assert np.all(np.isfinite(im.score_rows(0))) and im.posterior_positions(0).shape == (M, N + 1)


def check_rc(rc):
    from smcpp_amd import _engine
    _engine.check(rc)


def test_states():
    """No E-step; save_gamma off; parameters set again; no derivative seeds; smcpp_set_raw; more than 64 states."""
    im, cs = small(differentiable=False, save_gamma=False, estep=False)
    t = []
    for name, call in every_call(im):
        who = PP if name in POSTERIOR else "loglik track: " if name.startswith("loglik") else "score track: "
        t.append((f"no E-step: {name}", call, who + "no E-step has been run on this manager yet"))
    check(t)
    im.E_step()
    t = []
    for name, call in every_call(im):
        if name in POSTERIOR or name.startswith("score"):
            t.append((f"no save_gamma: {name}", call, (PP if name in POSTERIOR else "score track: ") + "save_gamma was not set for the last E-step"))
    t.append(("no save_gamma: a bad contig comes behind", lambda: im.posterior_columns(-1), PP + "save_gamma was not set for the last E-step"))
    check(t)
    assert im.loglik_positions(0).shape == (740,)                                # (the loglik track needs no save_gamma)
    im.save_gamma = True
    im.E_step()
    nder0 = "score track: the parameters carry no derivative seeds (nder = 0): set them with seeds and run the E-step again"
    check([("nder = 0: score_rows", lambda: im.score_rows(0), nder0), ("nder = 0: score_windows", lambda: im.score_windows(0, 100), nder0),
           ("nder = 0: the seeds before the selection", lambda: im.score_rows(0, step=0), nder0),
           ("nder = 0: the contig before the seeds", lambda: im.score_rows(-1), CONTIG)])
    # the parameters set again: what walks a row refuses, the stored columns are still handed out
    im.theta = 2 * tg.TH_B
    t = []
    for name, call in every_call(im):
        if name in WALKS:
            t.append((f"set again: {name}", call, DIRTY))
        elif name == "loglik_rows":
            t.append((f"set again: {name}", call, "loglik track: the parameters were set again after the last E-step, whose stored values "
                                                    "belong to the earlier ones: run the E-step again"))
        elif name.startswith("score"):
            t.append((f"set again: {name}", call, "score track: the parameters were set again after the last E-step, whose stored vectors "
                                                    "belong to the earlier ones: run the E-step again"))
    t += [("set again: the window before the parameters", lambda: im.posterior_transition_windows(0, 0), "posterior transition windows: window_bp < 1"),
          ("set again: the window before the parameters, exact", lambda: im.posterior_windows_exact(0, 0), "posterior windows: window_bp < 1"),
          ("set again: the parameters before the window", lambda: im.loglik_windows(0, 0), DIRTY),
          ("set again: the selection before the parameters", lambda: im.posterior_transitions(0, step=0), PP + "step < 1"),
          ("set again: the parameters before the paths", lambda: im.posterior_sample_rows(0, n_paths=0), DIRTY),
          ("set again: the parameters before the grid", lambda: im.posterior_positions(0, step=0), DIRTY)]
    check(t)
    assert im.posterior_columns(0).shape == (8, 16) and im.posterior_windows(0, 100).shape == (8, 8)
    im.theta = tg.TH_B
    im.E_step()
    # smcpp_set_raw with the model's own tables: T keeps its structure, the score track has no seeds
    good, _ = small()
    im.set_raw(good.pi, good.transition, good.keys, transref.emission_table(good))
    im.E_step()
    raw = "score track: the parameters were set with smcpp_set_raw: no model, no derivative seeds"
    check([("set_raw: score_rows", lambda: im.score_rows(0), raw), ("set_raw: score_windows", lambda: im.score_windows(0, 100), raw)])
    assert im.posterior_transitions(0)["stay"].shape == (16,)
    # an arbitrary matrix
    un = tg._unstructured(8, cs, tg.TH_B, tg.RH_B, n=tl.N4)
    un.save_gamma = True
    un.E_step()
    t = []
    for name, call in every_call(un):
        if name in WALKS:
            t.append((f"unstructured: {name}", call, UNSTRUCTURED))
        elif name.startswith("score"):
            t.append((f"unstructured: {name}", call, "score track: " + UNSTRUCTURED))
    check(t)
    assert un.posterior_columns(0).shape == (8, 16) and un.loglik_rows(0).shape == (16,)
    # more than 64 hidden states
    big = tg._onepop(65, cs, tg.TH_B, tg.RH_B, n=tl.N4)
    big.model.differentiable = True
    big.model.update_observers("model update")
    big.save_gamma = True
    big.E_step()
    m65 = ("score track: more than 64 hidden states (65): the kernel keeps one column of the M x M accumulator per lane and exists at one "
           "state per lane only")
    check([("M = 65: score_rows", lambda: big.score_rows(0), m65), ("M = 65: score_windows", lambda: big.score_windows(0, 100), m65)])


def test_caps():
    """2^31 - 1 elements, 1 GiB of scratch, the windows of one launch: refused before anything is allocated; with `out == NULL` the
    window calls whose cap stands behind the early return give the count instead."""
    n = tg.N
    long_rows = np.array([[1, 1, 2, n], [2 * 10**8, 0, 0, n], [50, 0, 0, n], [1, 1, 2, n]], dtype=np.int32)
    many = np.array([[10**5, 0, 0, n], [1, 1, 3, n]] * 1400, dtype=np.int32)
    huge = np.array([[10**9, 0, 0, n]] * 9 + [[50, 0, 0, n], [1, 1, 2, n]], dtype=np.int32)
    im = tg._onepop(64, [np.ascontiguousarray(c) for c in (long_rows, many, huge)], tg.TH_U, tg.RH_U)
    im.model.differentiable = True
    im.model.update_observers("model update")
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    assert plan["hybrid_rows"] and plan["states_per_lane"] == 1 and not plan["long_rows_cut"], plan
    ll = im.logliks().copy()
    assert np.all(np.isfinite(ll))
    N1, N2 = int(many[:, 0].sum(dtype=np.int64)), int(huge[:, 0].sum(dtype=np.int64))
    assert (N1, N2) == (140_001_400, 9_000_000_051)
    L = lib()
    nw = C.c_longlong(0)
    dummy = np.zeros(1)
    dp = dummy.ctypes.data_as(C.POINTER(C.c_double))
    sc_gib = ("score track: the scratch (16 directions x 3 parts x 5 engine rows, the checkpoints of a row of 200000000 positions) exceeds "
              "the cap of 1 GiB")
    pq_gib = "posterior positions: the checkpoints of a row of 200000000 positions exceed the scratch cap of 1 GiB"
    pp_gib = "posterior paths: the checkpoints of a row of 200000000 positions exceed the scratch cap of 1 GiB"
    pw_many = "posterior windows: too many windows for one launch (widen the window)"
    ptw_many = "posterior transition windows: too many windows for one launch (widen the window)"
    t = [("score_rows 1 GiB", lambda: im.score_rows(0), sc_gib), ("score_rows 1 GiB, one column", lambda: im.score_rows(0, 0, 1), sc_gib),
         ("score_windows 1 GiB", lambda: im.score_windows(0, 10**6), sc_gib),
         ("score_windows 1 GiB before the window", lambda: im.score_windows(0, 0), sc_gib),
         ("score_windows 2^31", lambda: im.score_windows(1, 1), f"score track: the windows (16 x {N1})" + CAP_SC),
         ("loglik_positions 2^31", lambda: im.loglik_positions(2), f"loglik track: the grid positions ({N2 + 1})" + CAP_LL),
         ("loglik_positions 2^31 exactly", lambda: im.loglik_positions(2, 0, 2**31, 1), "loglik track: the grid positions (2147483648)" + CAP_LL),
         ("loglik_windows 2^31", lambda: im.loglik_windows(2, 1), f"loglik track: the windows ({N2})" + CAP_LL),
         ("positions 2^31", lambda: im.posterior_positions(2), f"posterior positions: the columns (64 x {N2 + 1} positions)" + CAP_POS),
         ("position_summary 2^31", lambda: im.posterior_position_summary(2), f"posterior positions: the summaries (1 x {N2 + 1} positions)" + CAP_POS),
         ("position_summary 2^31, 3 levels", lambda: im.posterior_position_summary(2, quantiles=(0.1, 0.5, 0.9), pos1=10**9),
          "posterior positions: the summaries (3 x 1000000000 positions)" + CAP_POS),
         ("positions 1 GiB", lambda: im.posterior_positions(0, 5, 6), pq_gib),
         ("position_summary 1 GiB", lambda: im.posterior_position_summary(0, pos0=5, pos1=6), pq_gib),
         ("windows_exact 1 GiB", lambda: im.posterior_windows_exact(0, 10**6), pq_gib),
         ("sample_positions 1 GiB", lambda: im.posterior_sample_positions(0, 1, 7, 0, 0, 3), pp_gib),
         ("sample_rows 1 GiB", lambda: im.posterior_sample_rows(0, 1, 7, 0, 0, 1), pp_gib),
         # (out != NULL, never written: the refusal comes first)
         ("windows: too many", lambda: check_rc(L.smcpp_posterior_windows(im._im, 2, 1, C.byref(nw), dp)), pw_many),
         ("transition_windows: too many", lambda: check_rc(L.smcpp_posterior_transition_windows(im._im, 2, 1, C.byref(nw), dp)), ptw_many),
         ("windows_exact 2^31", lambda: check_rc(L.smcpp_posterior_windows_exact(im._im, 2, 1, C.byref(nw), dp)),
          f"posterior positions: the windows (64 x {N2} positions)" + CAP_POS),
         # (of the 1400 rows of 10^5 positions at W = 10, every tenth starts on a boundary: 10 000 segments, the others 10 001)
         ("windows_exact: segment sums", lambda: im.posterior_windows_exact(1, 10),
          "posterior positions: the segment sums of the cut rows (14001260 vectors) exceed the scratch cap of 1 GiB (widen the window)")]
    check(t)
    # out == NULL: what refuses all the same ...
    check([("NULL: score_rows", lambda: check_rc(L.smcpp_score_rows(im._im, 0, 0, 1, 1, 0, None)), sc_gib),
           ("NULL: score_windows", lambda: check_rc(L.smcpp_score_windows(im._im, 1, 1, C.byref(nw), None)), f"score track: the windows (16 x {N1})" + CAP_SC),
           ("NULL: loglik_positions", lambda: check_rc(L.smcpp_loglik_positions(im._im, 2, 0, N2 + 1, 1, None)),
            f"loglik track: the grid positions ({N2 + 1})" + CAP_LL),
           ("NULL: loglik_windows", lambda: check_rc(L.smcpp_loglik_windows(im._im, 2, 1, C.byref(nw), None)), f"loglik track: the windows ({N2})" + CAP_LL),
           ("NULL: positions", lambda: check_rc(L.smcpp_posterior_positions(im._im, 0, 5, 6, 1, None)), pq_gib),
           ("NULL: position_summary", lambda: check_rc(L.smcpp_posterior_position_summary(im._im, 0, 5, 6, 1, None, 0, None, None, None, None)), pq_gib),
           ("NULL: sample_rows", lambda: check_rc(L.smcpp_posterior_sample_rows(im._im, 2, 7, 0, BIG, 0, 12, 1, None, None, None)),
            f"posterior paths: the outputs ({BIG} paths x 12)" + CAP_PATHS)])
    # ... and what gives the count (or passes the checks) instead
    for name, f, W, count in (("windows", L.smcpp_posterior_windows, 1, N2), ("transition_windows", L.smcpp_posterior_transition_windows, 1, N2),
                              ("windows_exact", L.smcpp_posterior_windows_exact, 1, N2), ("windows_exact, segment sums", L.smcpp_posterior_windows_exact, 10, None)):
        c = 1 if count is None else 2
        nw.value = -1
        assert rc_of(f(im._im, c, W, C.byref(nw), None)) is None, name
        assert nw.value == (-(-N1 // W) if count is None else count), (name, nw.value)
    assert rc_of(L.smcpp_posterior_sample_positions(im._im, 0, 7, 0, 1, 0, 3, None)) is None
    assert rc_of(L.smcpp_posterior_sample_rows(im._im, 0, 7, 0, 1, 0, 1, 1, None, None, None)) is None
    # the manager is as it was
    assert np.array_equal(im.logliks(), ll)
    assert im.posterior_windows(1, 10**7).shape == (64, 15) and np.all(np.isfinite(im.score_windows(1, 10**7)))


def test_simulate():
    """smcpp_simulate: the arguments, the resume states, the parameters, the outputs."""
    from smcpp_amd import _smcpp, synth
    im, cs = small(estep=False)
    keys = im.keys
    K, M = len(keys), im.M
    A = np.arange(K, dtype=np.int32)
    quiet = int(np.nonzero((keys[:, 0] == 0) & (keys[:, 1] == 0) & (keys[:, 2] == tl.N4))[0][0])
    who = "simulate: "

    def sim(lengths=(300,), alphabet=A, q=quiet, contig0=0, rep0=0, nreps=1, cap=64, resume=None):
        return lambda: im._simulate_call(list(lengths), alphabet, q, 5, contig0, rep0, nreps, cap, resume)

    twice = np.concatenate([A, A[3:4]])
    t = [("no lengths", sim(lengths=()), who + "no contig lengths"),
         ("N < 1", sim(lengths=(300, 0, -5)), who + "contig 1 has N < 1 positions"),
         ("n_replicates", sim(nreps=0), who + "n_replicates < 1"), ("cap", sim(cap=0), who + "cap < 1 (events per replicate and call)"),
         ("first_replicate", sim(rep0=-1), who + "first_replicate < 0"),
         ("replicate word", sim(rep0=BIG, nreps=2), who + "first_replicate + n_replicates > 2^31 (the replicate index is one 32-bit word of the counter)"),
         ("contig word", sim(contig0=-1), who + "the contig index does not fit one 32-bit word of the counter"),
         ("contig word, above", sim(contig0=2 ** 32), who + "the contig index does not fit one 32-bit word of the counter"),
         ("no alphabet", sim(alphabet=A[:0]), who + "the alphabet is empty"),
         ("entry out of range", sim(alphabet=np.concatenate([A[:-1], [K]]).astype(np.int32)),
          who + f"alphabet entry {K - 1} (key index {K}) is out of range: the manager holds {K} keys"),
         ("entry negative", sim(alphabet=np.concatenate([[-1], A[1:]]).astype(np.int32)),
          who + f"alphabet entry 0 (key index -1) is out of range: the manager holds {K} keys"),
         ("given twice", sim(alphabet=twice), who + "key index 3 is given twice in the alphabet"),
         ("quiet", sim(alphabet=A[A != quiet]), who + f"the quiet key (key index {quiet}) is not in the alphabet"),
         ("outputs", sim(nreps=2 ** 20, cap=2 ** 12, lengths=(300, 300)),
          who + "the outputs (2 contigs x 1048576 replicates x 4096 events) exceed the cap of 2^31 - 1 elements per call: ask for fewer "
                "replicates or a smaller cap"),
         ("resume state", sim(nreps=2, resume=np.array([[0, 0, -1], [5, 10, M]])), who + "resume state 1 is not one a call has returned for this contig"),
         ("resume position", sim(resume=np.array([[5, 301, 0]])), who + "resume state 0 is not one a call has returned for this contig"),
         ("the order: lengths before replicates", sim(lengths=(0,), nreps=0), who + "contig 0 has N < 1 positions"),
         ("the order: the alphabet before the outputs", sim(alphabet=twice, nreps=2 ** 20, cap=2 ** 12), who + "key index 3 is given twice in the alphabet")]
    check(t)
    x0, nev, pos, state, key, rout = sim()()
    assert x0.shape == (1, 1) and 0 <= x0[0, 0] < M
    # an output array is missing (none of them: the checks alone)
    L = lib()
    ll = C.POINTER(C.c_longlong)
    lengths = np.array([300], dtype=np.int64)
    rc = L.smcpp_simulate(im._im, 1, lengths.ctypes.data_as(ll), K, A.ctypes.data_as(C.POINTER(C.c_int)), quiet, 5, 0, 0, 1, 64, None,
                          x0.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, None)
    assert rc_of(rc) == who + "an output array is missing"
    # no parameters; a state without mass; a negative emission probability
    bare = _smcpp.PyOnePopInferenceManager(tl.N4, cs, synth.hidden_states(M), ("pop1",), 0.5)
    unset = who + "parameters are not set (set_params or set_raw first)"
    pi, T, Et = im._hmm_tables()
    E0 = Et.copy()
    E0[:, 7] = 0.0
    Eneg = Et.copy()
    Eneg[2, 5] = -1e-3

    def raw_sim(Etab):
        def call():
            bare.set_raw(pi, T, keys, Etab)
            bare._simulate_call([300], A, quiet, 5, 0, 0, 1, 64, None)
        return call

    check([("parameters", lambda: bare._simulate_call([300], A, quiet, 5, 0, 0, 1, 64, None), unset),
           ("the arguments before the parameters", lambda: bare._simulate_call([300], A, quiet, 5, 0, 0, 0, 64, None), who + "n_replicates < 1"),
           ("no mass", raw_sim(E0), who + "state 7 gives the alphabet no mass: no observation can be drawn there"),
           ("negative", raw_sim(Eneg), who + "the emission probability of alphabet entry 2 in state 5 is negative or not finite")])
    bare.set_raw(pi, T, keys, Et)
    got = bare._simulate_call([300], A, quiet, 5, 0, 0, 1, 64, None)
    assert all(np.array_equal(a, b) for a, b in zip(got, (x0, nev, pos, state, key, rout)))
