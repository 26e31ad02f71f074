"""The log-likelihood track on the device (smcpp_loglik_rows / _positions / _windows; smcpp_amd/csrc/loglik_track_dev.hpp): its exact
identities, tests/llref.py (the float64 position-level reference over the pure hidden Markov model of the manager's getters), its
refusals, posterior_products(loglik_windows=True) and poisoned memory.  Every test calls a new entry.

Exact identities.  Their tolerance is that of fp64 summation, fp(n, S) = n 2^-53 S with n the number of addends of both sides (the
engine's rows twice - its own total and the prefix scan - and the outputs added here) and S the sum of |log c| over the rows:
  1. windows sum to logliks()[c]; rows sum to it; positions at the row ends are the running sum of the rows; l(0) = 0;
  2. windows ARE the differences of loglik_positions at their boundaries, bit for bit;
  3. the same bits under SMCPP_LL_WAVES = 1, 3 and unset, on grids that share positions, after other products ran, after a
     save_gamma E-step instead of a plain one, on poisoned allocations (SMCPP_DEBUG_POISON=255), from the Cython manager;
  4. l does not increase along a contig whose rows all have log c <= 0.
Against llref (5.): per row |log c - llref| <= 4 d_row and per window <= 4 d_win(W), d_row / d_win(W) being the reference's own float
noise ON THAT INPUT - oracle/oracle.py's restatement of the reference (float alpha, 1e-10 floor, eigen-power steps) against llref,
measured here by llref.noise, never against the engine.  Both sides also round in fp64: fp(s_l + 64, |log c_l|) per row,
fp(W + 64, |window|) per window is added to the bar (1e-13 and less: it decides nothing below).
The tightest case is M = 1, contig 1: 1.13e-7 on the row of 129 positions against a bar of 1.15e-7.  At M = 1 a float holds
alpha = 1 exactly and the walk plays no part; the noise is NOT zero there because the oracle forms d^129 of a long row in its
eigen-power step, and what the engine adds is the float rounding of the E-step's own stored-pass scans in log c (SMCPP_SS_MIXED) -
the per-row evidence as it was before this product existed.  The case is deterministic, but a change of one rounding in the
EXISTING chains can move it past the bar: look there first, not at the track, if it ever fails.

Shapes (one-population cases at n = 4): M = 1, 2, 64, 65 (the first two states per lane), 150, 300 on two contigs (contig_base != 0)
(and M = 200, 600: four and sixteen states per lane, the other two instantiations of the walk) with rows of span 1, 2 (window 3 puts a boundary between its two positions), 63, 64, 65 and 500 (window 7 cuts it 71 times; cut into
pieces of 64 positions beyond 64 states: a caller's row is several engine rows), a boundary on a row end, a window wider than the
contig, a last partial window, step 1 over a whole row, one position inside a row; two populations at M = 24; rows of span 1 only; an
un-binned contig at M = 64 (hybrid rows above SMCPP_HYB_TH, one of them behind heterozygous sites that put alpha on the 1e-10 floor);
contigs of 255 / 256 / 257 and 65 535 / 65 536 / 65 537 rows (one block of the prefix scan, and one thread of its second level
holding one or two block sums: LL_SCAN_BLOCK = 256); more items than SMCPP_LL_WAVES allows; 4300 items on the default launch of
4096 wavefronts; a contig of 3 10^9 positions (three un-binned rows of 10^9) for the cap of 2^31 - 1 outputs and the 64-bit position
arithmetic above 2^31.

Measured on one MI355X (the tests print "WORST" lines; rows / windows as measured | bar): see DESIGN.md, "Log-likelihood track"."""
import numpy as np
import pytest

import llref
import test_gpu_gamma as tg

pytestmark = pytest.mark.gpu

N4 = 4
WIDTHS = (3, 7, 100)


def fp(n, S):
    return n * 2.0 ** -53 * S


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def site(rng, het=None):
    a = int(rng.integers(0, 2)) if het is None else int(het)
    b = int(rng.integers(0, N4 + 1)) if a == 1 else int(rng.integers(1, N4 + 1))
    return [1, a, b, N4]


def contig(spans, seed, missing=()):
    """Rows of the given spans: span 1 = a segregating or heterozygous site, longer = a monomorphic run (`missing`: indices of
    missing runs)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, s in enumerate(spans):
        rows.append(site(rng) if s == 1 else [s, -1, 0, 0] if i in missing else [s, 0, 0, N4])
    return np.ascontiguousarray(rows, dtype=np.int32)


SPANS_A = [1, 1, 2, 1, 63, 64, 65, 1, 1, 500, 1, 7, 1, 30, 1]        # P: 1 2 4 5 68 132 197 198 199 699 700 707 708 738 739
SPANS_B = [1, 40, 1, 1, 129, 1, 12]


def two_contigs():
    return [contig(SPANS_A, 1, missing=(13,)), contig(SPANS_B, 2)]


def many_rows(L, seed):
    """L rows: sites, a row of span 5 every 97 rows and as the last row."""
    spans = np.ones(L, dtype=np.int64)
    spans[96::97] = 5
    spans[-1] = 5
    return contig(spans.tolist(), seed)


_INPUTS = {}


def inputs(case):
    """-> (M, contigs, theta, rho)"""
    if case not in _INPUTS:
        if case.startswith("M"):
            r = (int(case[1:]), two_contigs(), tg.TH_B, tg.RH_B)
        elif case == "twopop:M24":
            r = (24, tg.twopop_contigs(60_000), None, None)
        elif case == "span1":
            r = (64, [contig([1] * 300, 3), contig([1] * 7, 4)], tg.TH_B, tg.RH_B)
        elif case == "hybrid:M64":
            rng = np.random.default_rng(5)
            rows = [site(rng), [3000, 0, 0, N4], site(rng), site(rng, 1), site(rng, 1), site(rng, 1), [700, 0, 0, N4], site(rng),
                    [5, 0, 0, N4], site(rng), [900, -1, 0, 0], site(rng)]
            r = (64, [np.ascontiguousarray(rows, dtype=np.int32), contig([1, 600, 1], 6)], tg.TH_U, tg.RH_U)
        elif case == "scan:block":
            r = (2, [many_rows(L, L) for L in (255, 256, 257)], tg.TH_B, tg.RH_B)
        elif case == "scan:level2":
            r = (2, [many_rows(L, L) for L in (65_535, 65_536, 65_537)], tg.TH_B, tg.RH_B)
        elif case == "huge":
            # three un-binned rows of 10^9 positions (eigen-power steps on the hybrid plan), a short row and a site behind them
            rows = [[10**9, 0, 0, N4]] * 3 + [[50, 0, 0, N4], [1, 1, 2, N4]]
            r = (64, [np.ascontiguousarray(rows, dtype=np.int32)], tg.TH_U, tg.RH_U)
        elif case == "items:4300":
            r = (2, [contig([2, 1, 3] * 2150, 7)], tg.TH_B, tg.RH_B)
        else:
            raise AssertionError(case)
        _INPUTS[case] = r
    return _INPUTS[case]


def manager(case, save_gamma=False, estep=True):
    M, contigs, theta, rho = inputs(case)
    im = tg._twopop(M, contigs) if case.startswith("twopop") else tg._onepop(M, contigs, theta, rho, n=N4)
    im.save_gamma = save_gamma
    if estep:
        im.E_step()
    return im, contigs


_REF = {}


def reference(case, im, contigs):
    """Per contig (l, d_row, {W: d_win}): llref and the reference's own noise on this input, once per case and process."""
    if case not in _REF:
        pi, T, keys, E = im.pi, im.transition, im.keys, llref.emission_table(im)
        _REF[case] = [llref.noise(pi, T, keys, E, ob, WIDTHS)[:3] for ob in contigs]
    return _REF[case]


def engine_rows(im):
    return int(im.describe()["plan"]["rows"])


def track(im, c):
    """What the same-bits tests compare."""
    return {"rows": im.loglik_rows(c), "pos": im.loglik_positions(c), "w3": im.loglik_windows(c, 3), "w7": im.loglik_windows(c, 7),
            "w100": im.loglik_windows(c, 100)}


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.float64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def check_identities(im, c, ob, label):
    """1., 2. and 4. on contig c; -> (rows, positions)."""
    P = llref.prefix(ob)
    L, N = len(ob), int(P[-1])
    ll = float(im.logliks()[c])
    rows = im.loglik_rows(c)
    pos = im.loglik_positions(c)
    assert rows.shape == (L + 1,) and pos.shape == (N + 1,) and rows.dtype == pos.dtype == np.float64, label
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(pos)), label
    assert rows[0] == 0.0 and pos[0] == 0.0, label
    S, Le = float(np.abs(rows).sum()), engine_rows(im)
    assert abs(rows.sum() - ll) <= fp(2 * Le + L, S), (label, rows.sum(), ll)
    assert abs(pos[N] - ll) <= fp(2 * Le, S), (label, pos[N], ll)
    assert np.max(np.abs(pos[P] - np.cumsum(rows))) <= fp(2 * Le + L, S), label
    for W in sorted(set(WIDTHS + (1, N - 1, N, N + 5, int(P[5]) if L > 5 else 2))):
        if W < 1:
            continue
        w = im.loglik_windows(c, W)
        b = np.minimum(np.arange(0, N + W, W, dtype=np.int64), N)[:-(-N // W) + 1]
        assert w.shape == (-(-N // W),) and w.dtype == np.float64, (label, W)
        assert np.array_equal(w, np.diff(pos[b])), (label, W)
        assert abs(w.sum() - ll) <= fp(2 * Le + len(w), S), (label, W, w.sum(), ll)
    # 4.: a row whose emission vector stays below one in every state has z < 1 at every position, so its log c is negative beyond
    # any rounding: asserted, and l must not increase inside it.  (A missing row has e = 1 and log c = 0 up to the engine's rounding,
    # either sign: l is held there only where its log c came out <= 0.)
    E = llref.emission_table(im)[llref.row_key_ids(ob, im.keys)]
    loud = E.max(axis=1) < 1.0 - 1e-6
    assert loud.any() and np.all(rows[1:][loud] < 0.0), (label, rows[1:][loud].max())
    down = np.repeat(rows[1:] <= 0.0, ob[:, 0].astype(np.int64))               # per position 1 .. N: its row has log c <= 0
    up = np.diff(pos) > 0.0
    assert not np.any(up & down), f"{label}: l increases at position {int(np.argmax(up & down)) + 1}"
    return rows, pos


def sub_grids(ob):
    """Grids that share positions with the full one: step 1 over the longest row, one position inside it, strides, the ends."""
    P, N = llref.prefix(ob), int(ob[:, 0].sum())
    l = int(np.argmax(ob[:, 0]))
    q0, s = int(P[l]), int(ob[l, 0])
    grids = [(0, 1, 1), (N, N + 1, 1), (0, N + 1, 7), (1, N + 1, 64), (max(0, N - 5), N + 1, 2), (q0 + 1, q0 + s + 1, 1), (q0, q0 + s + 1, s)]
    if s >= 3:
        grids += [(q0 + 1, q0 + 2, 1), (q0 + s - 1, q0 + s, 1), (q0 + 2, q0 + 3, 5), (q0 + 1, q0 + s, 3)]
    return grids


def check_against_llref(case, im, contigs):
    """5.: rows and windows against llref at 4 x the reference's own noise; -> worst (measured / bar)."""
    refs = reference(case, im, contigs)
    worst = 0.0
    for c, ob in enumerate(contigs):
        ell, d_row, d_win = refs[c]
        spans = ob[:, 0].astype(np.int64)
        rows = im.loglik_rows(c)
        want = llref.rows(ell, ob)
        d = np.abs(rows - want)[1:]
        bar = 4.0 * d_row + fp(spans + 64, np.abs(want[1:]))
        line = f"{case} contig {c}: WORST rows {d.max():.2e} | bar {4 * d_row:.2e}"
        ratio = float((d / bar).max())
        for W in WIDTHS:
            w, ww = im.loglik_windows(c, W), llref.windows(ell, W)
            assert w.shape == ww.shape, (case, c, W)
            dw = np.abs(w - ww)
            bw = 4.0 * d_win[W] + fp(W + 64, np.abs(ww))
            line += f"; W = {W}: {dw.max():.2e} | {4 * d_win[W]:.2e}"
            ratio = max(ratio, float((dw / bw).max()))
        print(line + f"; walk ratio {im.describe()['ll_walk_worst_ratio']:.2e}")
        worst = max(worst, ratio)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = ["M1", "M2", "M64", "M65", "M150", "M200", "M300", "M600", "twopop:M24", "span1", "hybrid:M64", "scan:block"]


@pytest.mark.parametrize("case", SHAPES)
def test_identities_and_reference(engine_opt, case):
    """1., 2., 4. and 5. on every contig of the case after a PLAIN E-step; the sub-grids of 3."""
    engine_opt("SMCPP_LL_WAVES", None)
    im, contigs = manager(case)
    plan = im.describe()["plan"]
    if case in ("M150", "M200", "M300", "M600"):
        assert plan["long_rows_cut"] and engine_rows(im) > sum(len(ob) for ob in contigs), plan
    if case in ("M65", "M200", "M600"):
        assert plan["states_per_lane"] == {"M65": 2, "M200": 4, "M600": 16}[case], plan
    if case == "hybrid:M64":
        assert plan["hybrid_rows"], plan
        # the rows in front of the walked row of 700 positions sit on the 1e-10 floor in the reference's own float alpha
        from oracle import oracle
        o = oracle.estep(im.pi, im.transition, im.keys, llref.emission_table(im), contigs[0])
        assert np.min(o["alpha_hat"][6]) == np.float32(1e-10) and contigs[0][6, 0] == 700
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        rows, pos = check_identities(im, c, ob, label)
        for pos0, pos1, step in sub_grids(ob):
            got = im.loglik_positions(c, pos0, pos1, step)
            assert np.array_equal(got, pos[pos0:pos1:step]), (label, pos0, pos1, step)
        L = len(ob)
        for start, stop, step in ((0, L + 1, 1), (0, 1, 1), (L, L + 1, 1), (1, L + 1, 3), (1, max(2, L), 2)):
            assert np.array_equal(im.loglik_rows(c, start, stop, step), rows[start:stop:step]), (label, start, stop, step)
    if case == "M64":
        im.loglik_windows(0, 7)
        d = im.describe()
        P = llref.prefix(contigs[0])
        inside = [int(np.sum((np.arange(7, P[-1], 7) > P[l]) & (np.arange(7, P[-1], 7) < P[l + 1]))) for l in range(len(contigs[0]))]
        assert inside[9] == 71                                     # (window 7 cuts the row of 500 positions 71 times)
        cut = sum(1 for k in inside if k > 0)
        assert d["ll_items"] == cut == d["ll_waves"] and cut >= 4, (d["ll_items"], cut)
        assert np.isfinite(d["ll_walk_worst_ratio"]) and d["ll_walk_worst_ratio"] >= 0.0, d
    worst = check_against_llref(case, im, contigs)
    assert worst <= 1.0, f"{case}: {worst:.2f} of the bar (4 x the reference's own noise)"


def test_prefix_scan_second_level(engine_opt):
    """Contigs of 65 535 / 65 536 / 65 537 rows: 256 and 257 block sums, so a thread of the scan's second level holds one or two."""
    case = "scan:level2"
    im, contigs = manager(case)
    refs = reference(case, im, contigs)
    for c, ob in enumerate(contigs):
        P = llref.prefix(ob)
        L = len(ob)
        rows = im.loglik_rows(c)
        S = float(np.abs(rows).sum())
        ll = float(im.logliks()[c])
        ends = im.loglik_positions(c, 0, int(P[-1]) + 1, 1)[P]
        assert abs(rows.sum() - ll) <= fp(3 * L, S) and abs(ends[-1] - ll) <= fp(2 * L, S), (c, rows.sum(), ends[-1], ll)
        assert np.max(np.abs(ends - np.cumsum(rows))) <= fp(3 * L, S), c
        w = im.loglik_windows(c, 1000)
        assert abs(w.sum() - ll) <= fp(2 * L + len(w), S), c
        ell, d_row, _ = refs[c]
        want = llref.rows(ell, ob)
        d = np.abs(rows - want)[1:]
        print(f"{case} contig {c}: WORST rows {d.max():.2e} | bar {4 * d_row:.2e}")
        assert np.all(d <= 4.0 * d_row + fp(ob[:, 0] + 64, np.abs(want[1:]))), c


def test_same_bits(engine_opt):
    """3.: SMCPP_LL_WAVES = 1, 3 and unset (more items than wavefronts: a wavefront's second item), repetition, the posterior
    products in between, a save_gamma E-step, poisoned allocations."""
    from smcpp_amd import _engine
    engine_opt("SMCPP_LL_WAVES", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    for case in ("M64", "M150", "hybrid:M64"):
        im, contigs = manager(case)
        good = [track(im, c) for c in range(len(contigs))]
        ll = im.logliks().copy()
        im.loglik_windows(0, 7)
        items = im.describe()["ll_items"]
        assert items >= 4
        for waves in ("1", "3", None):
            engine_opt("SMCPP_LL_WAVES", waves)
            for c in range(len(contigs)):
                same_bits(track(im, c), good[c])
            im.loglik_windows(0, 7)
            d = im.describe()
            assert d["ll_items"] == items and d["ll_waves"] == (items if waves is None else int(waves)), d
        # a save_gamma E-step on the same parameters, the posterior products in between
        im2, _ = manager(case, save_gamma=True)
        for c in range(len(contigs)):
            same_bits(track(im2, c), good[c])
            gam = im2.posterior_columns(c, normalize=False)
            im2.posterior_windows_exact(c, 7)
            im2.posterior_transitions(c)
            same_bits(track(im2, c), good[c])
            assert np.array_equal(im2.posterior_columns(c, normalize=False), gam)         # (the posterior buffers are not disturbed)
        assert np.array_equal(im2.logliks(), ll)
        # poisoned allocations: a fresh manager, every fresh device buffer filled with 0xFF bytes
        _engine.set_option("SMCPP_DEBUG_POISON", "255")
        try:
            im3, _ = manager(case)
            for c in range(len(contigs)):
                same_bits(track(im3, c), good[c])
        finally:
            _engine.set_option("SMCPP_DEBUG_POISON", None)


def test_more_items_than_wavefronts_on_the_default_launch(engine_opt):
    """4300 items on 4096 wavefronts: the same numbers as with one wavefront, the identities, llref."""
    engine_opt("SMCPP_LL_WAVES", None)
    case = "items:4300"
    im, contigs = manager(case)
    ob = contigs[0]
    rows, pos = check_identities(im, 0, ob, case)
    assert np.array_equal(im.loglik_positions(0), pos)
    d = im.describe()
    assert d["ll_items"] == 4300 and d["ll_waves"] == 4096, d
    engine_opt("SMCPP_LL_WAVES", "1")
    assert np.array_equal(im.loglik_positions(0), pos) and im.describe()["ll_waves"] == 1
    engine_opt("SMCPP_LL_WAVES", None)
    assert check_against_llref(case, im, contigs) <= 1.0


def test_refusals(engine_opt):
    """Every refusal raises RuntimeError with a message before anything is launched; loglik() is unchanged and the manager usable."""
    case = "M64"
    im, contigs = manager(case)
    L, nc = len(contigs[0]), len(contigs)
    N = int(contigs[0][:, 0].sum())
    good, ll = track(im, 0), im.logliks().copy()

    def raises(call, match=None):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip(), "an error without a message"
        assert np.array_equal(im.logliks(), ll)
        same_bits(track(im, 0), good)

    for c in (-1, nc, nc + 5):
        for call in (lambda: im.loglik_rows(c), lambda: im.loglik_positions(c), lambda: im.loglik_windows(c, 100)):
            raises(call, "contig")
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(start=4, stop=2), dict(step=0), dict(step=-1), dict(start=L + 1)):
        raises(lambda: im.loglik_rows(0, **kw))
    for kw in (dict(pos0=-1), dict(pos1=N + 2), dict(pos0=3, pos1=3), dict(pos0=4, pos1=2), dict(step=0), dict(step=-1), dict(pos0=N + 1)):
        raises(lambda: im.loglik_positions(0, **kw))
    for W in (0, -5):
        raises(lambda: im.loglik_windows(0, W), "window_bp")
    # no E-step yet
    fresh, _ = manager(case, estep=False)
    for call in (lambda: fresh.loglik_rows(0), lambda: fresh.loglik_positions(0), lambda: fresh.loglik_windows(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    fresh.E_step()
    same_bits(track(fresh, 0), good)
    # parameters set again without an E-step: the stored values belong to the earlier ones
    fresh.theta = 2 * tg.TH_B
    for call in (lambda: fresh.loglik_rows(0), lambda: fresh.loglik_positions(0), lambda: fresh.loglik_windows(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    fresh.theta = tg.TH_B
    fresh.E_step()
    same_bits(track(fresh, 0), good)
    # a transition matrix without the scan structure: the rows need none, the walk is refused
    M, cs, theta, rho = inputs("M64")
    raw = tg._unstructured(8, cs, theta, rho, n=N4)
    raw.E_step()
    llr = raw.logliks().copy()
    for call in (lambda: raw.loglik_positions(0), lambda: raw.loglik_windows(0, 100)):
        with pytest.raises(RuntimeError, match="semiseparable structure"):
            call()
    assert np.array_equal(raw.logliks(), llr)
    r = raw.loglik_rows(0)
    assert abs(r.sum() - llr[0]) <= fp(3 * L, float(np.abs(r).sum()))
    raw.E_step()
    assert np.array_equal(raw.logliks(), llr) and np.array_equal(raw.loglik_rows(0), r)


def test_output_cap_and_positions_above_2_31(engine_opt):
    """A contig of 3 10^9 + 51 positions: more than 2^31 - 1 grid positions or windows are refused before anything is launched or
    allocated (the bindings make the checks-only call first), logliks() is unchanged and the manager usable; positions and
    boundaries above 2^31 - row ends at 10^9, 2 10^9, 3 10^9 and the inside of the short row behind them - come out right.
    (Windows narrower than 10^9 would put boundaries inside the rows of 10^9 positions, each of them 10^9 dependent steps of one
    wavefront: minutes.  They are left out for their time.)"""
    engine_opt("SMCPP_LL_WAVES", None)
    im, contigs = manager("huge")
    ob = contigs[0]
    P = llref.prefix(ob)
    N, G = int(P[-1]), 10**9
    assert N == 3 * G + 51 and N > 2**31 and im.describe()["plan"]["hybrid_rows"]
    ll = im.logliks().copy()
    assert np.all(np.isfinite(ll))
    rows = im.loglik_rows(0)
    S = float(np.abs(rows).sum())
    assert abs(rows.sum() - ll[0]) <= fp(16, S)

    def usable():
        assert np.array_equal(im.logliks(), ll)
        w = im.loglik_windows(0, G)                                             # boundaries on the row ends G, 2 G, 3 G
        assert w.shape == (4,) and abs(w.sum() - ll[0]) <= fp(16, S)
        assert np.max(np.abs(w - np.array([rows[1], rows[2], rows[3], rows[4] + rows[5]]))) <= fp(16, S)
        return w

    good = usable()
    for call in (lambda: im.loglik_positions(0), lambda: im.loglik_positions(0, 0, 2**31, 1), lambda: im.loglik_windows(0, 1)):
        with pytest.raises(RuntimeError, match="cap of 2\\^31 - 1"):
            call()
        assert np.array_equal(usable(), good)
    ends = im.loglik_positions(0, 0, N + 1, G)                                  # 0, G, 2 G, 3 G: k_ll_ends above 2^31
    assert ends.shape == (4,) and ends[0] == 0.0 and np.max(np.abs(ends - np.cumsum(rows)[:4])) <= fp(16, S)
    # the inside of the row of 50 positions behind 3 G: the walk's table and slots at positions above 2^31
    q0 = 3 * G
    inner = im.loglik_positions(0, q0, q0 + 52, 1)
    assert inner.shape == (52,) and abs(inner[0] - ends[3]) <= fp(16, S) and abs(inner[51] - ll[0]) <= fp(16, S)
    assert abs(inner[50] - (ends[3] + rows[4])) <= fp(16, S) and np.all(np.diff(inner) < 0.0)
    assert np.array_equal(im.loglik_positions(0, q0 + 7, q0 + 40, 3), inner[7:40:3])
    assert im.describe()["ll_items"] == 1
    # the row is 50 identical steps from a vector that has long forgotten its start: nearly uniform in q
    assert np.max(np.abs(np.diff(inner[:51]) - rows[4] / 50)) <= 1e-3 * abs(rows[4] / 50)
    assert np.array_equal(usable(), good)


def test_cython_manager_gives_the_same_bits(engine_opt):
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    engine_opt("SMCPP_LL_WAVES", None)
    im, contigs = manager("M65")
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(N4, contigs, synth.hidden_states(65), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1", differentiable=[])
    im2.theta = tg.TH_B; im2.rho = tg.RH_B; im2.alpha = 1.0
    im2.E_step()
    for c in range(len(contigs)):
        same_bits(track(im2, c), track(im, c))
        assert np.array_equal(im2.loglik_positions(c, 3, 150, 7), im.loglik_positions(c, 3, 150, 7))
        assert np.array_equal(im2.loglik_rows(c, 1, 5, 2), im.loglik_rows(c, 1, 5, 2))
    with pytest.raises(RuntimeError):
        im2.loglik_rows(0, start=-1)
    with pytest.raises(RuntimeError):
        im2.loglik_windows(len(contigs), 100)
    with pytest.raises(RuntimeError):
        im2.loglik_positions(0, pos0=5, pos1=5)


@pytest.mark.parametrize("pops", [1, 2])
def test_posterior_products_and_evidence(pops):
    """posterior_products(loglik_windows=True, window=W): the arrays of im.loglik_windows; without the flag the key set is today's;
    evidence.loglik_track gives the same track from a plain E-step, and two models compare through compare_tracks."""
    from smcpp_amd import synth
    from smcpp_amd.evidence import compare_tracks, loglik_track, surprisal
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    from smcpp_amd.posterior import posterior_products
    a, s = synth.model_pieces()
    M, W = 16, 1000
    if pops == 1:
        model = PiecewiseModel(a, s, 1e4, "pop1")
        other = PiecewiseModel(a * 1.3, s, 1e4, "pop1")
        raw = [synth.synth_posterior_contig(200, tg.N, seed=21), synth.synth_posterior_contig(90, tg.N, seed=22)]
        args, kw = (raw, M, tg.N, tg.TH_U, tg.RH_U), {}
    else:
        a8, s8 = synth.model_pieces(8)
        m1 = PiecewiseModel(a8, s8, 1e4, pid="pop1")
        m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(4)), s8[:4], 1e4, pid="pop2")
        model, other = TwoPopulationModel(m1, m2, 0.4), TwoPopulationModel(m1, m2, 0.8)
        raw = [synth.synth_contig_twopop(3, 300_000, 4, 3), synth.synth_contig_twopop(4, 150_000, 4, 3)]
        args, kw = (raw, M, (4, 3), synth.THETA, synth.RHO), dict(a=(2, 0))
    hs, prods, im = posterior_products(model, *args, window=W, loglik_windows=True, return_manager=True, **kw)
    _, plain = posterior_products(model, *args, window=W, **kw)
    today = ["mean_tmrca", "path", "qstate", "sites", "windows"]
    hs_t, tr, im_t = loglik_track(model, raw, hs, *args[2:], W, return_manager=True, **kw)
    assert np.array_equal(hs_t, hs) and not im_t.save_gamma
    for c, pr in enumerate(prods):
        assert sorted(plain[c]) == sorted(today) and sorted(pr) == sorted(today + ["loglik_windows"])
        assert np.array_equal(pr["loglik_windows"], im.loglik_windows(c, W))
        assert pr["loglik_windows"].shape == (pr["windows"].shape[1],) and pr["loglik_windows"].dtype == np.float64
        assert np.array_equal(tr[c], pr["loglik_windows"])
        ll = float(im.logliks()[c])
        assert abs(pr["loglik_windows"].sum() - ll) <= fp(3 * len(pr["sites"]) + len(tr[c]), float(np.abs(im.loglik_rows(c)).sum()))
    _, tr_b = loglik_track(other, raw, hs, *args[2:], W, **kw)
    cmp_ = compare_tracks(tr, tr_b, block=5)
    D = sum(float(t.sum()) for t in tr) - sum(float(t.sum()) for t in tr_b)
    assert abs(cmp_["delta"] - D) <= 1e-9 * abs(D) and cmp_["se"] > 0.0 and np.isfinite(cmp_["z"])
    sp = surprisal(tr, W, [int(pr["sites"].sum()) for pr in prods])
    assert all(np.all(x > 0.0) for x in sp)
