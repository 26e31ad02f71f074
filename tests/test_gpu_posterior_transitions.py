"""The posterior transition products - `posterior_transitions`, `posterior_transition_windows` (smcpp_amd/csrc/posterior_trans_dev.hpp)
and `posterior.posterior_products(transitions=True)` - on every column of every contig.

Managers come from `test_gpu_gamma.run_case`, which asserts the route each case ran (scan steps at 1, 2, 8 and 16 states per lane,
a forced chunking, rows cut into pieces at 2 and 8 states per lane, two populations), from an own case on un-binned rows at
M = 32 and M = 64 under default switches (the hybrid scan chains; spans 64, 65, 128, 129 and 10^5 placed by hand, the other spans
capped at 1000 so that the position-level oracle walks 3.4e5 positions per M; contigs of one and of two rows) and from golden G4
through `test_gpu_parity.make_im`.

The truth is tests/transref.py: a float64 forward-backward pass over the pure HMM built from the manager's own getters, which forms
the dense xi_p at every position.  Bounds, per column l of span s_l (the project's bars for the per-row posterior, which is built
from the same stored vectors):

  each of stay / up / down        absolute 2e-5 s_l                    GAMMA_TOL
  values of at least 1e-3 s_l     relative 1e-4                        GAMMA_LARGE_TOL
  stay + up + down against s_l    relative 1e-9                        GAMMA_SUM_RTOL
  column 0                        exactly zero
  sum over the rows of a contig   relative 5e-6 (STAT_TOL) against the trace and the strict upper / lower triangle sums of the
                                  engine's own xisum; for G4 against the golden's xisum (the compiled reference) as well
  windows                         relative (W + 8) 2^-52 against the overlap-matrix oracle applied to the device's own per-row values
                                  (each side sums at most W non-negative terms); the three rows of a window sum to its covered
                                  base pairs within the same bound
  selections, repetition, call order, a repeated E-step, poisoned allocations: the same bits

Measured on one MI355X (worst over the contigs of a case; absolute in units of the span / relative on the large values / sum
against the span / sum over the rows against the engine's xisum):

  case                 of the span   large values   sum vs span   rows vs xisum
  scan:M64             5.6e-09       2.7e-07        2.2e-16       1.0e-08
  scan:M300            3.3e-09       1.9e-07        2.2e-16       4.3e-09
  scan:M520            2.0e-09       1.6e-07        2.2e-16       5.2e-09
  scan:M100:chunk37    6.3e-09       2.7e-07        2.2e-16       4.4e-09
  cut:M100             1.6e-08       5.7e-07        2.2e-16       1.2e-08
  cut:M300             4.2e-09       1.7e-07        2.2e-16       6.8e-09
  twopop:M130          1.2e-08       5.0e-07        2.2e-16       1.4e-08
  unbinned:M32         1.5e-08       3.7e-07        2.2e-16       3.9e-08
  unbinned:M64         1.0e-08       7.2e-07        2.2e-16       1.5e-08
  G4                   7.8e-09       3.7e-07        3.3e-16       6.2e-10   (against the golden's xisum: see the test's output)
  eig_b:M13            9.6e-09       6.1e-07        2.2e-16       9.0e-09   (SMCPP_GAMMA_SCAN=0)
  pieces:M65           7.8e-10       3.3e-07        2.2e-16       3.5e-08   (SMCPP_SPLIT_SPANS=0, dense chains)
  dense:M64            7.0e-09       3.3e-07        3.0e-16       3.2e-08   (SMCPP_SS=0)

More rows than wavefronts.  The kernel is persistent: wavefront gw owns one slice of scratch (the parked addends of a block, the
fp64 checkpoints of a long row) and takes rows 1 + gw, 1 + gw + nwaves, ..; the host gives it the fewest of the rows, 4096 slots
(1024 from 8 states per lane) and the wavefronts whose scratch fits 1 GiB.  The `stride:` cases assert from `describe()`
(`transition_waves`, the plan) that the first contig has more rows than wavefronts, check every column, the sums over the rows and
the windows of 100 base pairs as above, and ask for the same bits on repetition, after the other posterior products and on
poisoned allocations (wall time of the test with the oracle, of which the device's calls are a few ms):

  case          rows on wavefronts (scratch each)              of the span   large values   sum vs span   rows vs xisum   time
  stride:M64    1442 on 1264 (848 896 bytes: the 1 GiB cap;    5.6e-08       4.0e-07        2.2e-16       1.5e-08         38 s
                543 rows of 2 .. 1563 blocks, default plan)
  stride:M100   4274 on 4096 (98 304 bytes, 2 states a lane)   4.2e-09       1.6e-07        3.3e-16       4.4e-09         0.8 s
  stride:M300   1235 on 1024 (393 216 bytes, 8 states a lane)  1.6e-08       9.2e-08        2.2e-16       4.3e-09         1.7 s
  stride:M520   1235 on 1024 (786 432 bytes, 16 states a lane) 5.5e-09       1.1e-07        2.2e-16       3.1e-09         6.2 s

(stride:M64 walks 3.0e5 positions in the oracle, as unbinned:M64 walks 3.4e5 in 58 s.)
"""
import numpy as np
import pytest

import test_gpu_gamma as tg
import transref
from conftest import load_golden
from test_gpu_parity import GAMMA_LARGE_TOL, GAMMA_SUM_RTOL, GAMMA_TOL, STAT_TOL, make_im
from test_gpu_posterior_products import _selections, window_widths

pytestmark = pytest.mark.gpu

EPS = transref.EPS
ROUTES = ["scan:M64", "scan:M300", "scan:M520", "scan:M100:chunk37", "cut:M100", "cut:M300", "twopop:M130"]
OWN = ["unbinned:M32", "unbinned:M64", "G4"]
CASES = ROUTES + OWN
SHORT = {"cut:M100"}                                        # contigs short enough for one window per base pair
NAMES = ("stay", "up", "down")

_UNBINNED = {}
_ORACLE = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# managers and the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def unbinned_inputs():
    """Un-binned rows, two contigs of 120 and 90 rows + the one- and two-row contigs; the longest row holds 10^5 positions."""
    if "c" not in _UNBINNED:
        _UNBINNED["c"] = tg.unbinned_contigs(120, cap=1000)
        total = sum(int(c[:, 0].sum()) for c in _UNBINNED["c"])
        assert total <= 2_000_000 and max(int(c[:, 0].max()) for c in _UNBINNED["c"]) == 100_000
        assert any(len(c) == 1 for c in _UNBINNED["c"]) and any(len(c) == 2 for c in _UNBINNED["c"])
    return _UNBINNED["c"]


def manager(case, engine_opt, estep=True):
    """-> (im, contigs) after a save_gamma E-step (estep=False: before any E-step; own cases and routes of one population)."""
    if case in ROUTES and estep:
        return tg.run_case(case, engine_opt)
    if case in ROUTES:
        kind, M, switches, chunk, _ = tg.CASES[case]
        assert kind != "twopop" and not switches
        contigs, theta, rho = tg.case_inputs(kind, M)
        return tg._onepop(M, contigs, theta, rho), contigs
    if case == "G4":
        g = load_golden("G4_M64_n20_2Mbp")
        im, contigs = make_im(g), [np.ascontiguousarray(g["obs"], dtype=np.int32)]
    else:
        M = int(case.split(":M")[1])
        contigs = unbinned_inputs()
        im = tg._onepop(M, contigs, tg.TH_U, tg.RH_U)
    if estep:
        im.save_gamma = True
        im.E_step()
        plan = im.describe()["plan"]
        print(f"{case}: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family')} }")
        if case != "G4":
            # default switches on rows of up to 10^5 positions at M <= 64: the hybrid scan chains, nothing cut
            assert plan["chain_family"] == 6 and plan["states_per_lane"] == 1 and not plan["long_rows_cut"], plan
    return im, contigs


def oracle(case, im, contigs):
    """tests/transref.py on every contig of the case, from the manager's getters; once per case and process."""
    if case not in _ORACLE:
        pi, T, keys, E = im.pi, im.transition, im.keys, transref.emission_table(im)
        _ORACLE[case] = [transref.transitions(pi, T, keys, E, ob) for ob in contigs]
    return _ORACLE[case]


def trans(im, c, *sel):
    t = im.posterior_transitions(c, *sel)
    assert sorted(t) == ["down", "stay", "up"]
    return np.stack([t[k] for k in NAMES])


def products(im, c):
    return {"rows": trans(im, c), "w100": im.posterior_transition_windows(c, 100), "w7": im.posterior_transition_windows(c, 7)}


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.float64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        assert np.all(np.isfinite(a[k])), k


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------
def check_rows(v, ref, spans, label):
    """Every column against the oracle; returns the worst of each measure."""
    L = len(spans)
    assert v.shape == ref.shape == (3, L + 1) and v.dtype == np.float64, (label, v.shape, ref.shape)
    assert np.all(np.isfinite(v)) and np.all(v >= 0.0), label
    assert np.all(v[:, 0] == 0.0), (label, v[:, 0])
    s = np.asarray(spans, dtype=np.float64)
    d = np.abs(v[:, 1:] - ref[:, 1:])
    scale = d / s
    large = ref[:, 1:] >= 1e-3 * s
    rel = np.where(large, d / np.where(large, ref[:, 1:], 1.0), 0.0)
    sums = np.abs(v[:, 1:].sum(axis=0) - s) / s
    worst = {"scale": float(scale.max(initial=0.0)), "large": float(rel.max(initial=0.0)), "sum": float(sums.max(initial=0.0))}
    print(f"{label}: {L} rows, worst value of its span {worst['scale']:.2e}, large values rel {worst['large']:.2e}, "
          f"stay + up + down vs span {worst['sum']:.2e}")
    bad = np.nonzero((scale > GAMMA_TOL).any(axis=0))[0]
    assert len(bad) == 0, f"{label}: {len(bad)} columns off by more than {GAMMA_TOL} of their span, e.g. rows {bad[:8] + 1} " \
                          f"(spans {s[bad[:8]]}, got {v[:, 1:][:, bad[:8]]}, want {ref[:, 1:][:, bad[:8]]})"
    bad = np.nonzero((rel > GAMMA_LARGE_TOL).any(axis=0))[0]
    assert len(bad) == 0, f"{label}: {len(bad)} columns with a large value off by more than {GAMMA_LARGE_TOL} relative, e.g. rows " \
                          f"{bad[:8] + 1} (spans {s[bad[:8]]}, got {v[:, 1:][:, bad[:8]]}, want {ref[:, 1:][:, bad[:8]]})"
    bad = np.nonzero(sums > GAMMA_SUM_RTOL)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} columns do not sum to their span, e.g. rows {bad[:8] + 1} (spans {s[bad[:8]]})"
    return worst


def triangles(X):
    X = np.asarray(X, dtype=np.float64)
    return np.array([np.trace(X), np.triu(X, 1).sum(), np.tril(X, -1).sum()])


def check_statistic(v, X, label):
    """sum_l stay / up / down against the trace and the triangle sums of an xisum."""
    got, want = v.sum(axis=1), triangles(X)
    rel = np.abs(got - want) / np.maximum(want, 1e-300)
    rel = np.where(want == 0.0, np.where(got == 0.0, 0.0, np.inf), rel)            # (one hidden state: no triangles)
    print(f"{label}: sum over rows {got}, xisum trace / upper / lower {want}, relative {rel}")
    assert np.all(rel <= STAT_TOL), (label, got, want, rel)
    return float(rel.max())


def check_windows(im, c, v, spans, short, label):
    total = int(np.sum(spans))
    for W in window_widths(total, short):
        got = im.posterior_transition_windows(c, W)
        want, covered = transref.transition_windows(v, spans, W)
        assert got.dtype == np.float64 and got.shape == want.shape == (3, -(-total // W)), (label, W, got.shape)
        tol = (W + 8) * EPS
        err = np.abs(got - want)
        bad = err > tol * np.abs(want)
        assert not bad.any(), f"{label}, W = {W}: {int(bad.sum())} entries off, worst {np.max(err / np.maximum(want, 1e-300)) / EPS:.1f} eps"
        serr = np.abs(got.sum(axis=0) - covered) / covered
        assert np.all(serr <= tol), f"{label}, W = {W}: a window's three rows miss its base pairs by {serr.max() / EPS:.1f} eps (bar {W + 8})"
        if W == 1:
            assert got.shape[1] == total


def check_selections(im, c, v, L, label):
    for start, stop, step in _selections(L):
        got = trans(im, c, start, stop, step)
        assert np.array_equal(got, v[:, slice(start, stop, step)]), (label, start, stop, step)


def check_all(case, im, contigs, short=False, refs=None):
    refs = oracle(case, im, contigs) if refs is None else refs
    xis = im.xisums
    worst = {"scale": 0.0, "large": 0.0, "sum": 0.0, "stat": 0.0}
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        v = trans(im, c)
        w = check_rows(v, refs[c], ob[:, 0], label)
        w["stat"] = check_statistic(v, xis[c], label)
        for k in worst:
            worst[k] = max(worst[k], w[k])
        check_windows(im, c, v, ob[:, 0], short, label)
        check_selections(im, c, v, len(ob), label)
    print(f"{case}: WORST scale {worst['scale']:.2e} large {worst['large']:.2e} sum {worst['sum']:.2e} stat {worst['stat']:.2e}")
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_column_against_the_oracle(engine_opt, case):
    """stay / up / down of every column of every contig against the position-level oracle, their sums over the rows against the
    engine's own xisum (G4: and the golden's), the windows, the selections."""
    im, contigs = manager(case, engine_opt)
    if case != "G4":
        assert any(len(ob) == 1 for ob in contigs) and any(len(ob) == 2 for ob in contigs)
    check_all(case, im, contigs, case in SHORT)
    if case == "G4":
        g = load_golden("G4_M64_n20_2Mbp")
        check_statistic(trans(im, 0), g["xisum"], "G4 against the golden's xisum")


@pytest.mark.parametrize("case", ["eig_b:M13", "pieces:M65", "dense:M64"])
def test_non_default_switches_give_the_same_numbers(engine_opt, case):
    """The kernel reads the stored vectors, the emission table and the generators of T, nothing else of the E-step's plan: per-row
    posteriors from eigensystems (SMCPP_GAMMA_SCAN=0), un-cut rows of up to 10^5 positions beyond 64 states on the dense chains
    (SMCPP_SPLIT_SPANS=0: checkpointed rows at two states per lane) and the scan chains switched off (SMCPP_SS=0) stay within the
    bounds of the default plan."""
    if case == "dense:M64":
        engine_opt("SMCPP_SS", "0")
        contigs, theta, rho = tg.case_inputs("binned", 64)
        im = tg._onepop(64, contigs, theta, rho)
        im.save_gamma = True
        im.E_step()
        assert im.describe()["plan"]["chain_family"] not in (5, 6)
    else:
        im, contigs = tg.run_case(case, engine_opt)
    check_all(case, im, contigs)


@pytest.mark.parametrize("case", ["scan:M64", "cut:M300", "twopop:M130", "unbinned:M64"])
def test_order_and_repetition(engine_opt, case):
    """Repeated calls, another call order, the per-row posterior products in between, another E-step with the same parameters: the
    same bits; other contigs' results are unchanged by a call."""
    im, contigs = manager(case, engine_opt)
    nc = len(contigs)
    first = [products(im, c) for c in range(nc)]
    for c in range(nc):
        same_bits(products(im, c), first[c])
    for c in reversed(range(nc)):
        w7 = im.posterior_transition_windows(c, 7)                          # (windows before rows, contigs descending)
        assert np.array_equal(w7, first[c]["w7"])
        assert np.array_equal(trans(im, c), first[c]["rows"])
    gam = im.gammas                                                          # (the merge buffer of cut rows, the posterior products)
    im.posterior_windows(0, 100)
    im.posterior_summary(nc - 1)
    for c in range(nc):
        same_bits(products(im, c), first[c])
    assert all(np.array_equal(a, b) for a, b in zip(gam, im.gammas))
    im.E_step()
    for c in (1, 0) + tuple(range(2, nc)):
        same_bits(products(im, c), first[c])


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100"])
def test_second_estep_with_other_parameters(engine_opt, case):
    """Other parameters, then an E-step: the products follow (checked on every column again); parameters set WITHOUT an E-step:
    refused, and the E-step makes the manager usable again."""
    im, contigs = manager(case, engine_opt)
    before = [trans(im, c) for c in range(len(contigs))]
    im.rho = im.rho * 1.7
    with pytest.raises(RuntimeError, match="E-step"):
        im.posterior_transitions(0)
    with pytest.raises(RuntimeError, match="E-step"):
        im.posterior_transition_windows(0, 100)
    im.E_step()
    after = [trans(im, c) for c in range(len(contigs))]
    assert not np.array_equal(after[0], before[0])
    pi, T, keys, E = im.pi, im.transition, im.keys, transref.emission_table(im)
    check_all(case + " (rho x 1.7)", im, contigs, refs=[transref.transitions(pi, T, keys, E, ob) for ob in contigs])


@pytest.mark.parametrize("case", ["scan:M100:chunk37", "unbinned:M64"])
def test_poisoned_allocations(engine_opt, case):
    """Every fresh allocation filled with 0xFF bytes: no NaN and the same bits as without - no output or scratch buffer of the
    products is read before it is written."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = manager(case, engine_opt)
    clean = [products(im, c) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im, contigs = manager(case, engine_opt)
    poisoned = [products(im, c) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(clean, poisoned):
        same_bits(b, a)


# ---------------------------------------------------------------------------------------------------------------------------------
# more rows than wavefronts: a wavefront's second row
# ---------------------------------------------------------------------------------------------------------------------------------
# case -> (states, states per lane, wavefront slots, rows / positions of the first contig)
STRIDE = {"stride:M64": (64, 1, 4096, 1442, 199_056), "stride:M100": (100, 2, 4096, 4274, 18_128),
          "stride:M300": (300, 8, 1024, 1235, 5136), "stride:M520": (520, 16, 1024, 1235, 5136)}
_STRIDE = {}


def stride_inputs(case):
    """-> (contigs, theta, rho).  stride:M64: un-binned rows of at most 200 positions beside 64 / 65 / 128 / 129 / 10^5 placed by
    hand - 848 896 bytes of scratch per wavefront, so the 1 GiB cap, not the rows or the slots, sets the wavefront count; the
    others: more binned rows than slots."""
    key = "M64" if case == "stride:M64" else "M100" if case == "stride:M100" else "M300"
    if key not in _STRIDE:
        _STRIDE[key] = (tg.unbinned_contigs(1400, seeds=(11,), cap=200), tg.TH_U, tg.RH_U) if key == "M64" else \
                       (tg.binned_contigs(140, 1_800_000), tg.TH_B, tg.RH_B) if key == "M100" else \
                       (tg.binned_contigs(340, 500_000), tg.TH_B, tg.RH_B)
    return _STRIDE[key]


def stride_manager(case, engine_opt):
    """An own manager under default switches after a save_gamma E-step, its plan asserted."""
    engine_opt("SMCPP_SPLIT_SPANS", None)
    M, npl, slots, L, N = STRIDE[case]
    contigs, theta, rho = stride_inputs(case)
    assert (len(contigs[0]), int(contigs[0][:, 0].sum())) == (L, N), (case, len(contigs[0]), int(contigs[0][:, 0].sum()))
    im = tg._onepop(M, contigs, theta, rho)
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    print(f"{case}: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family')} }")
    assert plan["states_per_lane"] == npl and not plan["long_rows_cut"], plan
    if case == "stride:M64":
        assert plan["chain_family"] == 6, plan
    return im, contigs


def stride_waves(case, ob):
    """The wavefronts the launch rule gives the contig: its rows, the slots, or what fits 1 GiB of scratch."""
    M, npl, slots, _, _ = STRIDE[case]
    nck = (int(ob[:, 0].max()) + 63) // 64 - 1
    per_wave = 64 * 3 * 64 * npl * 4 + nck * 64 * npl * 8
    return min(len(ob), slots, (1 << 30) // per_wave), per_wave


def stride_rows(case, im, contigs, c):
    """stay / up / down of contig c, the launch printed; contig 0: fewer wavefronts than rows, asserted."""
    v = trans(im, c)
    waves, L = im.describe()["transition_waves"], len(contigs[c])
    want, per_wave = stride_waves(case, contigs[c])
    print(f"{case} contig {c}: {L} rows on {waves} wavefronts ({per_wave} bytes of scratch each)")
    assert waves == want, (case, c, waves, want)
    if c == 0:
        assert waves < L, (case, waves, L)
    return v


@pytest.mark.parametrize("case", sorted(STRIDE))
def test_second_row_of_a_wavefront(engine_opt, case):
    """More rows than wavefronts - by the 1 GiB scratch cap at one state per lane (rows of many blocks: wavefronts that parked
    checkpoints go on to another row), by the 4096 / 1024 slots at 2, 8 and 16 states per lane: every column against the oracle,
    the sums over the rows against the engine's xisum, the windows of 100 base pairs."""
    im, contigs = stride_manager(case, engine_opt)
    if case == "stride:M64":
        spans = contigs[0][:, 0]
        assert int((spans > 64).sum()) == 543 and int(spans.max()) == 100_000
        assert stride_waves(case, contigs[0]) == (1264, 848_896)
    refs = oracle(case, im, contigs)
    xis = im.xisums
    worst = {"scale": 0.0, "large": 0.0, "sum": 0.0, "stat": 0.0}
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        spans = ob[:, 0]
        v = stride_rows(case, im, contigs, c)
        w = check_rows(v, refs[c], spans, label)
        w["stat"] = check_statistic(v, xis[c], label)
        for k in worst:
            worst[k] = max(worst[k], w[k])
        W, total = 100, int(spans.sum())
        got = im.posterior_transition_windows(c, W)
        assert im.describe()["transition_waves"] == stride_waves(case, ob)[0]
        want, covered = transref.transition_windows(v, spans, W)
        assert got.dtype == np.float64 and got.shape == want.shape == (3, -(-total // W)), (label, got.shape)
        tol = (W + 8) * EPS
        err = np.abs(got - want)
        assert not (err > tol * np.abs(want)).any(), f"{label}: windows off, worst {np.max(err / np.maximum(want, 1e-300)) / EPS:.1f} eps"
        serr = np.abs(got.sum(axis=0) - covered) / covered
        assert np.all(serr <= tol), f"{label}: a window's three rows miss its base pairs by {serr.max() / EPS:.1f} eps (bar {W + 8})"
    print(f"{case}: WORST scale {worst['scale']:.2e} large {worst['large']:.2e} sum {worst['sum']:.2e} stat {worst['stat']:.2e}")


@pytest.mark.parametrize("case", ["stride:M64", "stride:M300", "stride:M520"])
def test_second_row_gives_the_same_bits(engine_opt, case):
    """Repetition, the other posterior products in between, poisoned allocations: the same bits - a second row that reads what the
    first left in the wavefront's scratch shows here."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = stride_manager(case, engine_opt)
    nc = len(contigs)

    def all_products(im):
        out = []
        for c in range(nc):
            out.append({"rows": stride_rows(case, im, contigs, c), "w100": im.posterior_transition_windows(c, 100)})
        return out

    first = all_products(im)
    for a, b in zip(all_products(im), first):
        same_bits(a, b)
    for c in reversed(range(nc)):
        im.posterior_windows(c, 100)
        im.posterior_summary(nc - 1 - c)
        im.posterior_sample_rows(c, 2, 5)
        im.posterior_columns(0, normalize=False)
        assert np.array_equal(im.posterior_transition_windows(c, 100), first[c]["w100"])
        assert np.array_equal(trans(im, c), first[c]["rows"])
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im, contigs = stride_manager(case, engine_opt)
    poisoned = all_products(im)
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(first, poisoned):
        same_bits(b, a)


def test_unstructured_transition_matrix_is_refused(engine_opt):
    """set_raw with a T of no structure: both calls raise with a message that names the reason; the manager is still usable."""
    im, contigs = tg.run_case("eig_big:M96:unstructured", engine_opt)
    gam = im.gammas[0]
    for call in (lambda: im.posterior_transitions(0), lambda: im.posterior_transitions(1, 0, 1, 1),
                 lambda: im.posterior_transition_windows(0, 100)):
        with pytest.raises(RuntimeError, match="semiseparable structure"):
            call()
    assert np.array_equal(im.posterior_columns(0, normalize=False), gam)
    im.E_step()
    assert np.array_equal(im.gammas[0], gam)
    with pytest.raises(RuntimeError, match="semiseparable structure"):
        im.posterior_transitions(0)


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100", "unbinned:M32"])
def test_argument_errors(engine_opt, case):
    """Every argument error raises RuntimeError with a message before anything is launched, and a following valid call still gives
    the same bits."""
    im, contigs = manager(case, engine_opt)
    L = len(contigs[0])
    nc = len(contigs)
    good = products(im, 0)

    def raises(call, match=None):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip(), "an error without a message"
        same_bits(products(im, 0), good)

    for c in (-1, nc, nc + 5):
        raises(lambda: im.posterior_transitions(c), "contig")
        raises(lambda: im.posterior_transition_windows(c, 100), "contig")
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(start=4, stop=2), dict(step=0), dict(step=-1),
               dict(start=L + 1)):
        raises(lambda: im.posterior_transitions(0, **kw))
    for W in (0, -5):
        raises(lambda: im.posterior_transition_windows(0, W), "window_bp")
    # the last E-step ran without save_gamma
    im.save_gamma = False
    im.E_step()
    for call in (lambda: im.posterior_transitions(0), lambda: im.posterior_transition_windows(0, 100)):
        with pytest.raises(RuntimeError, match="save_gamma"):
            call()
    assert np.all(np.isfinite(im.logliks()))
    im.save_gamma = True
    im.E_step()
    same_bits(products(im, 0), good)
    # no E-step yet
    fresh, _ = manager(case, engine_opt, estep=False)
    fresh.save_gamma = True
    for call in (lambda: fresh.posterior_transitions(0), lambda: fresh.posterior_transition_windows(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    fresh.E_step()
    same_bits(products(fresh, 0), good)


def test_cython_manager_gives_the_same_bits(engine_opt):
    """The compiled Cython manager (set-up as in tests/test_cython_binding.py) against the ctypes one on scan:M64."""
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    im, contigs = tg.run_case("scan:M64", engine_opt)
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(tg.N, contigs, synth.hidden_states(im.M), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1", differentiable=[])
    im2.theta = tg.TH_B; im2.rho = tg.RH_B; im2.alpha = 1.0
    im2.save_gamma = True
    im2.E_step()
    for c in range(len(contigs)):
        same_bits(products(im2, c), products(im, c))
        for start, stop, step in _selections(len(contigs[c])):
            assert np.array_equal(trans(im2, c, start, stop, step), trans(im, c, start, stop, step))
    with pytest.raises(RuntimeError):
        im2.posterior_transitions(0, start=-1)
    with pytest.raises(RuntimeError):
        im2.posterior_transition_windows(len(contigs), 100)


@pytest.mark.parametrize("pops", [1, 2])
def test_posterior_products_with_transitions(tmp_path, pops):
    """posterior_products(transitions=True, window=W): the arrays of the manager calls; the default key set is today's; the file
    round-trips the new keys."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    from smcpp_amd.posterior import posterior_products, save_products_npz
    a, s = synth.model_pieces()
    M, W = 16, 1000
    if pops == 1:
        model = PiecewiseModel(a, s, 1e4, "pop1")
        raw = [synth.synth_posterior_contig(200, tg.N, seed=21), synth.synth_posterior_contig(90, tg.N, seed=22)]
        args, kw = (model, raw, M, tg.N, tg.TH_U, tg.RH_U), {}
    else:
        a8, s8 = synth.model_pieces(8)
        m1 = PiecewiseModel(a8, s8, 1e4, pid="pop1")
        m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(4)), s8[:4], 1e4, pid="pop2")
        model = TwoPopulationModel(m1, m2, 0.4)
        raw = [synth.synth_contig_twopop(3, 300_000, 4, 3), synth.synth_contig_twopop(4, 150_000, 4, 3)]
        args, kw = (model, raw, M, (4, 3), synth.THETA, synth.RHO), dict(a=(2, 0))
    hs, prods, im = posterior_products(*args, window=W, transitions=True, return_manager=True, **kw)
    today = ["mean_tmrca", "path", "qstate", "sites", "windows"]
    for c, pr in enumerate(prods):
        assert sorted(pr) == sorted(today + ["transitions", "transition_windows"])
        ncol = len(pr["sites"]) + 1
        assert pr["transitions"].shape == (3, ncol) and pr["transitions"].dtype == np.float64
        assert np.array_equal(pr["transitions"], trans(im, c))
        assert np.array_equal(pr["transition_windows"], im.posterior_transition_windows(c, W))
        assert pr["transition_windows"].shape == (3, pr["windows"].shape[1])
        spans = pr["sites"].astype(float)
        assert np.all(pr["transitions"][:, 0] == 0.0)
        assert np.max(np.abs(pr["transitions"][:, 1:].sum(axis=0) - spans) / spans) <= GAMMA_SUM_RTOL
    hs2, plain = posterior_products(*args, window=W, **kw)
    assert all(sorted(pr) == today for pr in plain)
    for pr, pl in zip(prods, plain):
        for k in today:
            assert pr[k].dtype == pl[k].dtype and np.array_equal(pr[k], pl[k]), k
    _, no_windows = posterior_products(*args, transitions=True, **kw)
    assert all(sorted(pr) == ["mean_tmrca", "path", "qstate", "sites", "transitions"] for pr in no_windows)
    _, bare = posterior_products(*args, **kw)
    assert all(sorted(pr) == ["mean_tmrca", "path", "qstate", "sites"] for pr in bare)
    names = ["chr1.smc.gz", "chr2.smc.gz"]
    path = tmp_path / "products.npz"
    save_products_npz(str(path), hs, prods, names)
    z = np.load(str(path))
    keys = today + ["transitions", "transition_windows"]
    assert sorted(z.files) == sorted(["hidden_states"] + [f"{nm}_{k}" for nm in names for k in keys])
    for nm, pr in zip(names, prods):
        for k in keys:
            assert z[f"{nm}_{k}"].dtype == pr[k].dtype and np.array_equal(z[f"{nm}_{k}"], pr[k]), (nm, k)
    path2 = tmp_path / "plain.npz"
    save_products_npz(str(path2), hs2, plain, names)
    assert sorted(np.load(str(path2)).files) == sorted(["hidden_states"] + [f"{nm}_{k}" for nm in names for k in today])
