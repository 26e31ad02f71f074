"""The per-position posterior products on the device (smcpp_posterior_positions / _position_summary / _windows_exact;
smcpp_amd/csrc/posterior_pos_dev.hpp) against tests/posref.py, the float64 position-level oracle over the pure hidden Markov model
of the manager's getters, and against the engine's own per-row products.

Bounds (tests/test_gpu_parity.py's bars for what is built from the same stored vectors):
  1. every position of every contig: |gamma - oracle| <= GAMMA_TOL (2e-5), entries >= 1e-3 within GAMMA_LARGE_TOL (1e-4) relative, a
     column sums to one within (M + 8) eps, position 0 is column 0 of posterior_columns within 4 eps;
  2. sum over the positions of row l = s_l p[:, l] of posterior_columns within GAMMA_TOL s_l; the position of a row of span 1 IS the
     row's column, bit for bit (the stored alpha_l o beta_l has no getter: the longer rows' last position is held by 1. alone);
  3. argmax / qstate / mean against the device's own columns on the same grid, mean against the oracle within GAMMA_TOL sum |w|;
  4. exact windows at W = 100, 10^4 and window_widths': GAMMA_TOL against the oracle, a window sums to one within (W + M + 8) eps,
     W = 1 equals the columns within 4 eps, one window equals posterior_windows within (L + 8) eps relative;
  5. on unbinned:M64 the window of the 10^5-position row that posterior_windows misses most (2.5e-2 in the oracle alone, computed on
     the host from smcpp_host_prep_onepop before this assert was kept) is missed by the exact product by at most GAMMA_TOL;
  6. rows walked: at most n_windows - 1 on binned rows; a grid inside one row walks its pieces;
  7. the same bits for sub-grids, repetition, other call orders, another E-step and back, poisoned allocations, the Cython manager;
  8. a wavefront's second row (more items than wavefronts): 1., 2. and 7. again;
  9. every argument error before anything is launched; 10. posterior_products(grid=, exact_windows=True).
The caps of 2^31 - 1 output elements and of 1 GiB of scratch need contigs of 3 10^7 positions and more: no test reaches them.

Measured on one MI355X, worst over the contigs of a case (the tests print these as "WORST" lines): entry / entries >= 1e-3 relative /
column sum - 1 / row sums per position / mean per unit of sum |w| / exact windows:
  scan:M64           3.15e-7  1.65e-6  4.0 eps  1.62e-8   5.85e-10  3.15e-7
  scan:M100:chunk37  3.00e-7  3.87e-6  3.0 eps  8.34e-9   1.93e-10  3.00e-7
  scan:M300          1.74e-8  1.00e-6  5.0 eps  8.75e-9   4.43e-11  1.74e-8
  scan:M520          1.18e-8  7.94e-7  8.0 eps  1.02e-9   2.85e-11  1.18e-8
  cut:M100           2.70e-7  7.57e-5  5.0 eps  1.03e-9   1.64e-8   2.70e-7
  cut:M300           8.60e-8  2.29e-6  5.0 eps  2.57e-9   2.55e-10  8.60e-8
  twopop:M130        6.48e-8  1.01e-6  4.0 eps  5.27e-9   1.39e-10  6.48e-8
  unbinned:M32       2.86e-7  4.36e-5  3.5 eps  7.95e-9   2.64e-8   2.86e-7
  unbinned:M64       5.82e-7  4.21e-5  4.0 eps  3.50e-9   2.89e-8   5.82e-7
  G4                 5.50e-7  3.42e-6  3.5 eps  1.59e-8   9.69e-10  5.50e-7
  stride:M100        1.70e-7  1.73e-6  4.0 eps  9.03e-9   2.34e-10
  stride:M300        9.51e-8  1.87e-6  6.0 eps  3.03e-9   5.42e-11
  stride:M520        6.02e-8  2.18e-6  8.0 eps  2.11e-9   2.95e-11
  stride:M64         2.52e-7  1.16e-5  4.0 eps  1.36e-7   1.63e-8
5.: window 1 of row 92 of unbinned:M64: posterior_windows misses the oracle by 2.518e-2, posterior_windows_exact by 5.05e-8.

stride:M64 is the case that shows the 1e-10 floor of the stored alpha: behind two heterozygous sites alpha(0) is 1.2e-11, stored as
1e-10, and b_p(0) is 1600 times the other states' inside the monomorphic row that follows - 1.40e-4 relative where gamma_p(0)
crosses 1e-3 when the walk starts from the floored entry, 1.16e-5 with the entry restored (pq_start)."""
import numpy as np
import pytest

import posref
import postref
import test_gpu_gamma as tg
import test_gpu_posterior_transitions as pt
from test_gpu_parity import GAMMA_LARGE_TOL, GAMMA_TOL
from test_gpu_posterior_products import window_widths

pytestmark = pytest.mark.gpu

EPS = posref.EPS
CASES = pt.ROUTES + pt.OWN
QUANTILES = (0.025, 0.5, 0.975)

_ORACLE = {}                # case -> per contig [M x (N + 1)]; the last three cases of the process


def oracle(case, im, contigs):
    """tests/posref.py on every position of every contig, from the manager's getters; once per case while it stays cached."""
    if case not in _ORACLE:
        while len(_ORACLE) >= 3:
            del _ORACLE[next(iter(_ORACLE))]
        pi, T, keys, E = im.pi, im.transition, im.keys, posref.emission_table(im)
        _ORACLE[case] = [posref.positions(pi, T, keys, E, ob) for ob in contigs]
    return _ORACLE[case]


def weights_of(M):
    return np.cumsum(0.05 + 0.02 * np.arange(M))              # ascending, like average coalescence times


def prefix(ob):
    return np.concatenate([[0], np.cumsum(ob[:, 0].astype(np.int64))])


def window_ref(ref, W):
    N = ref.shape[1] - 1
    lo = np.arange(0, N, W, dtype=np.int64)
    return np.add.reduceat(ref[:, 1:], lo, axis=1) / (np.minimum(lo + W, N) - lo)


def check_columns(g, ref, label, slab=1 << 15):
    """1.: every entry against the oracle, the column sums; -> worst (absolute, relative on large entries, column sum)."""
    M = g.shape[0]
    assert g.shape == ref.shape and g.dtype == np.float64, (label, g.shape, ref.shape)
    worst, where = [0.0, 0.0, 0.0], [0, 0, 0]
    for j in range(0, g.shape[1], slab):
        a, r = g[:, j:j + slab], ref[:, j:j + slab]
        assert np.all(np.isfinite(a)) and np.all(a >= 0.0), label
        d = np.abs(a - r)
        large = r >= 1e-3
        rel = np.where(large, d / np.where(large, r, 1.0), 0.0)
        cs = np.abs(a.sum(axis=0) - 1.0)
        for k, v in enumerate((d.max(axis=0), rel.max(axis=0), cs)):
            if v.max() > worst[k]:
                worst[k], where[k] = float(v.max()), j + int(v.argmax())
    print(f"{label}: {g.shape[1]} positions, worst entry {worst[0]:.3e} (position {where[0]}), large entries rel {worst[1]:.3e} "
          f"(position {where[1]}), column sum {worst[2] / EPS:.1f} eps")
    assert worst[0] <= GAMMA_TOL, f"{label}: position {where[0]} off by {worst[0]:.2e}"
    assert worst[1] <= GAMMA_LARGE_TOL, f"{label}: position {where[1]}: a large entry off by {worst[1]:.2e} relative"
    assert worst[2] <= (M + 8) * EPS, f"{label}: column {where[2]} misses one by {worst[2] / EPS:.1f} eps"
    return worst


def check_rows(im, c, g, ob, label):
    """2.: the sums over the rows against s_l p[:, l]; span-1 rows and position 0 against the stored columns."""
    spans, P = ob[:, 0].astype(np.int64), prefix(ob)
    p = im.posterior_columns(c)
    assert np.max(np.abs(g[:, 0] - p[:, 0])) <= 4 * EPS, label
    sums = np.add.reduceat(g[:, 1:], P[:-1], axis=1)
    d = np.abs(sums - p[:, 1:] * spans) / spans
    assert d.max() <= GAMMA_TOL, f"{label}: row {int(d.max(axis=0).argmax()) + 1} sums off by {d.max():.2e} of its span"
    one = np.nonzero(spans == 1)[0]
    assert np.array_equal(g[:, P[one + 1]], p[:, one + 1]), label
    return float(d.max())


def check_summary(im, c, g, ref, label, **grid):
    """3.: the summary on a grid against the device's own columns `g` of that grid and the oracle's `ref`."""
    M = g.shape[0]
    w = weights_of(M)
    sm = im.posterior_position_summary(c, weights=w, quantiles=QUANTILES, **grid)
    assert sorted(sm) == ["argmax", "mean", "qstate"]
    n = g.shape[1]
    assert sm["argmax"].shape == (n,) and sm["argmax"].dtype == np.int32 and sm["mean"].shape == (n,) and sm["mean"].dtype == np.float64
    assert sm["qstate"].shape == (len(QUANTILES), n) and sm["qstate"].dtype == np.int32
    cols = np.arange(n)
    assert np.all((sm["argmax"] >= 0) & (sm["argmax"] < M)) and np.all((sm["qstate"] >= 0) & (sm["qstate"] < M)), label
    assert np.array_equal(g[sm["argmax"], cols], g.max(axis=0)), label
    first = np.argmax(g, axis=0)                                            # the lowest state that attains it
    assert np.array_equal(sm["argmax"], first), label
    for k, q in enumerate(QUANTILES):
        ok = postref.quantile_ok(g, sm["qstate"][k], q, 2 * M * EPS)
        assert ok.all(), f"{label}: level {q}: {int((~ok).sum())} positions off, e.g. {np.nonzero(~ok)[0][:5]}"
    own = (w[:, None] * g).sum(axis=0)
    assert np.max(np.abs(sm["mean"] - own)) <= (M + 8) * EPS * np.abs(w).max(), label
    dm = float(np.max(np.abs(sm["mean"] - (w[:, None] * ref).sum(axis=0))))
    assert dm <= GAMMA_TOL * np.abs(w).sum(), (label, dm)
    no_w = im.posterior_position_summary(c, quantiles=QUANTILES[:1], **grid)
    assert sorted(no_w) == ["argmax", "qstate"] and np.array_equal(no_w["argmax"], sm["argmax"])
    assert np.array_equal(no_w["qstate"][0], sm["qstate"][0])
    return dm / np.abs(w).sum()


def check_windows(im, c, g, ref, ob, short, label):
    """4.: the exact windows against the oracle's, their sums, W = 1 and one window."""
    M, N, L = g.shape[0], g.shape[1] - 1, len(ob)
    worst = 0.0
    for W in sorted(set([100, 10_000, 1] + window_widths(N, short))):
        got = im.posterior_windows_exact(c, W)
        want = window_ref(ref, W)
        assert got.dtype == np.float64 and got.shape == want.shape == (M, -(-N // W)), (label, W, got.shape)
        d = float(np.abs(got - want).max())
        worst = max(worst, d)
        assert d <= GAMMA_TOL, f"{label}, W = {W}: a window off by {d:.2e}"
        cs = np.abs(got.sum(axis=0) - 1.0).max()
        assert cs <= (W + M + 8) * EPS, f"{label}, W = {W}: a window misses one by {cs / EPS:.1f} eps"
        if W == 1:
            assert np.max(np.abs(got - g[:, 1:])) <= 4 * EPS, label
        if W >= N:
            uni = im.posterior_windows(c, W)
            assert np.all(np.abs(got - uni) <= (L + 8) * EPS * np.abs(uni)), (label, W)
    return worst


def check_all(case, im, contigs, refs, short=False, windows=True):
    worst = {"abs": 0.0, "large": 0.0, "colsum": 0.0, "rows": 0.0, "mean": 0.0, "windows": 0.0}
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        g = im.posterior_positions(c)
        a, r, s = check_columns(g, refs[c], label)
        got = {"abs": a, "large": r, "colsum": s, "rows": check_rows(im, c, g, ob, label),
               "mean": check_summary(im, c, g, refs[c], label)}
        if windows:
            got["windows"] = check_windows(im, c, g, refs[c], ob, short, label)
        for k in got:
            worst[k] = max(worst[k], got[k])
    print(f"{case}: WORST abs {worst['abs']:.2e} large rel {worst['large']:.2e} colsum {worst['colsum'] / EPS:.1f} eps "
          f"rows {worst['rows']:.2e} mean {worst['mean']:.2e} windows {worst['windows']:.2e}")
    return worst


def products(im, c, M=None):
    """What the same-bits tests compare: every position, a summary on a coarse grid, two window widths."""
    sm = im.posterior_position_summary(c, weights=weights_of(im.M if M is None else M), quantiles=QUANTILES, pos0=0, step=3)
    return {"pos": im.posterior_positions(c), "argmax": sm["argmax"].astype(np.float64), "mean": sm["mean"],
            "qstate": sm["qstate"].astype(np.float64), "w100": im.posterior_windows_exact(c, 100), "w7": im.posterior_windows_exact(c, 7)}


def sub_grids(ob):
    """Grids of positions: inside one block of the longest row, across its checkpoints at 64 / 65 / 128 / 129, a stride that the stop
    misses, the ends."""
    P, N = prefix(ob), int(ob[:, 0].sum())
    l = int(np.argmax(ob[:, 0]))
    q0, s = int(P[l]), int(ob[l, 0])
    grids = [(0, 1, 1), (N, N + 1, 1), (0, N + 1, 7), (1, N + 1, 64), (max(0, N - 5), N + 1, 2)]
    if s >= 8:
        grids += [(q0 + 3, q0 + 7, 1), (q0 + 2, q0 + s, 3)]
    if s >= 130:
        grids += [(q0 + 62, q0 + 132, 1), (q0 + 64, q0 + 130, 65), (q0 + 65, q0 + 66, 1), (q0 + 128, q0 + 131, 2)]
    return grids


def check_sub_grids(im, c, g, ob, label):
    for pos0, pos1, step in sub_grids(ob):
        got = im.posterior_positions(c, pos0, pos1, step)
        assert np.array_equal(got, g[:, pos0:pos1:step]), (label, pos0, pos1, step)
        sm = im.posterior_position_summary(c, weights=weights_of(im.M), quantiles=QUANTILES, pos0=pos0, pos1=pos1, step=step)
        assert np.array_equal(sm["argmax"], np.argmax(got, axis=0)), (label, pos0, pos1, step)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_position_against_the_oracle(engine_opt, case):
    """1. - 4. on every contig of the case, and the sub-grids of 7."""
    im, contigs = pt.manager(case, engine_opt)
    refs = oracle(case, im, contigs)
    check_all(case, im, contigs, refs, case in pt.SHORT)
    for c, ob in enumerate(contigs):
        check_sub_grids(im, c, im.posterior_positions(c), ob, f"{case} contig {c}")


def test_exact_windows_close_the_gap_on_a_long_row(engine_opt):
    """5.: the 10 kbp windows of the row of 10^5 positions, un-binned rows at M = 64."""
    case = "unbinned:M64"
    im, contigs = pt.manager(case, engine_opt)
    refs = oracle(case, im, contigs)
    W, ob = 10_000, contigs[0]
    P, l = prefix(ob), int(np.argmax(ob[:, 0]))
    assert ob[l, 0] == 100_000
    want = window_ref(refs[0], W)
    uni, exact = im.posterior_windows(0, W), im.posterior_windows_exact(0, W)
    w0, w1 = int(P[l] // W), int((P[l + 1] - 1) // W)
    miss_uni = np.abs(uni - want).max(axis=0)[w0:w1 + 1]
    miss_exact = np.abs(exact - want).max(axis=0)[w0:w1 + 1]
    w = int(miss_uni.argmax())
    print(f"{case}: window {w0 + w} of row {l + 1}: posterior_windows misses the oracle by {miss_uni[w]:.3e}, "
          f"posterior_windows_exact by {miss_exact[w]:.3e} (worst over the row's windows {miss_exact.max():.3e})")
    assert miss_exact[w] <= GAMMA_TOL
    assert miss_uni[w] > 10 * GAMMA_TOL


def test_rows_walked(engine_opt):
    """6.: binned rows under 10 kbp windows walk at most one row per window boundary; a grid inside one row walks that row."""
    im, contigs = pt.manager("scan:M64", engine_opt)
    ob = contigs[0]
    N, P = int(ob[:, 0].sum()), prefix(ob)
    for width in (10_000, 100, 7):
        out = im.posterior_windows_exact(0, width)
        d = im.describe()
        cut = sum(1 for l in range(len(ob)) if P[l] // width != (P[l + 1] - 1) // width)
        assert d["position_rows_walked"] == cut and cut <= out.shape[1] - 1, (width, d["position_rows_walked"], cut, out.shape)
        assert d["position_waves"] == min(cut, 4096)
    l = int(np.argmax(ob[:, 0]))
    im.posterior_positions(0, int(P[l]) + 1, int(P[l + 1]) + 1)
    d = im.describe()
    assert (d["position_rows_walked"], d["position_waves"]) == (1, 1), d
    # rows cut into pieces: the pieces of the row
    im, contigs = pt.manager("cut:M100", engine_opt)
    ob = contigs[0]
    P, l = prefix(ob), int(np.argmax(ob[:, 0]))
    assert ob[l, 0] > 64
    im.posterior_positions(0, int(P[l]) + 1, int(P[l + 1]) + 1)
    assert im.describe()["position_rows_walked"] == -(-int(ob[l, 0]) // 64)
    one = int(np.nonzero(ob[:, 0] == 1)[0][3])
    im.posterior_positions(0, int(P[one + 1]), int(P[one + 1]) + 1)            # a row of one position: its stored column, no walk
    assert im.describe()["position_rows_walked"] == 0


@pytest.mark.parametrize("case", ["scan:M64", "cut:M300", "twopop:M130", "unbinned:M64"])
def test_order_and_repetition(engine_opt, case):
    """7.: repeated calls, another call order, the other posterior products in between, another E-step with the same parameters."""
    im, contigs = pt.manager(case, engine_opt)
    nc = len(contigs)
    first = [products(im, c) for c in range(nc)]
    for c in range(nc):
        pt.same_bits(products(im, c), first[c])
    for c in reversed(range(nc)):
        assert np.array_equal(im.posterior_windows_exact(c, 7), first[c]["w7"])            # (windows before columns, contigs descending)
        im.posterior_windows(c, 100)
        im.posterior_transitions(c)
        im.posterior_sample_positions(c, 2, 5)
        im.posterior_summary(nc - 1 - c)
        assert np.array_equal(im.posterior_positions(c), first[c]["pos"])
    gam = im.gammas
    for c in range(nc):
        pt.same_bits(products(im, c), first[c])
    assert all(np.array_equal(a, b) for a, b in zip(gam, im.gammas))
    im.E_step()
    for c in (1, 0) + tuple(range(2, nc)):
        pt.same_bits(products(im, c), first[c])


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100"])
def test_second_estep_with_other_parameters_and_back(engine_opt, case):
    """7.: other parameters without an E-step are refused; after the E-step the products follow (checked against the oracle again);
    the first parameters and an E-step give the first bits back."""
    im, contigs = pt.manager(case, engine_opt)
    nc = len(contigs)
    before = [products(im, c) for c in range(nc)]
    rho = im.rho
    im.rho = rho * 1.7
    for call in (lambda: im.posterior_positions(0), lambda: im.posterior_position_summary(0), lambda: im.posterior_windows_exact(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    im.E_step()
    assert not np.array_equal(im.posterior_positions(0), before[0]["pos"])
    pi, T, keys, E = im.pi, im.transition, im.keys, posref.emission_table(im)
    check_all(case + " (rho x 1.7)", im, contigs, [posref.positions(pi, T, keys, E, ob) for ob in contigs], case in pt.SHORT)
    im.rho = rho
    im.E_step()
    for c in range(nc):
        pt.same_bits(products(im, c), before[c])


@pytest.mark.parametrize("case", ["scan:M100:chunk37", "unbinned:M64"])
def test_poisoned_allocations(engine_opt, case):
    """7.: every fresh allocation filled with 0xFF bytes: no NaN and the same bits as without."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = pt.manager(case, engine_opt)
    clean = [products(im, c) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im, contigs = pt.manager(case, engine_opt)
    poisoned = [products(im, c) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(clean, poisoned):
        pt.same_bits(b, a)


def test_cython_manager_gives_the_same_bits(engine_opt):
    """7.: the compiled Cython manager against the ctypes one on scan:M64."""
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
    for c, ob in enumerate(contigs):
        pt.same_bits(products(im2, c, im.M), products(im, c))
        for pos0, pos1, step in sub_grids(ob):
            assert np.array_equal(im2.posterior_positions(c, pos0, pos1, step), im.posterior_positions(c, pos0, pos1, step))
    with pytest.raises(RuntimeError):
        im2.posterior_positions(0, pos0=-1)
    with pytest.raises(RuntimeError):
        im2.posterior_position_summary(0, quantiles=(1.5,))
    with pytest.raises(RuntimeError):
        im2.posterior_windows_exact(len(contigs), 100)


# ---------------------------------------------------------------------------------------------------------------------------------
# more items than wavefronts: a wavefront's second row
# ---------------------------------------------------------------------------------------------------------------------------------
def stride_waves(case, ob):
    """The wavefronts the launch rule gives every position of the contig: its items (rows + position 0), the slots, or what fits
    1 GiB of scratch (the checkpoints of the longest walked row)."""
    M, npl, slots, _, _ = pt.STRIDE[case]
    walked = ob[:, 0][ob[:, 0] > 1]
    nck = (int(walked.max()) + 63) // 64 - 1 if len(walked) else 0
    per_wave = 64 * 64 * npl * 4 + nck * 64 * npl * 8
    return min(len(ob) + 1, slots, (1 << 30) // per_wave)


def stride_columns(case, im, contigs, c):
    g = im.posterior_positions(c)
    waves, L = im.describe()["position_waves"], len(contigs[c])
    print(f"{case} contig {c}: {L} rows on {waves} wavefronts")
    assert waves == stride_waves(case, contigs[c]), (case, c, waves)
    if c == 0:
        assert waves < L, (case, waves, L)
    return g


@pytest.mark.parametrize("case", sorted(pt.STRIDE))
def test_second_row_of_a_wavefront(engine_opt, case):
    """8.: more rows than wavefronts - by the 1 GiB cap at one state per lane, by the slots at 2, 8 and 16: 1. - 3. on every contig."""
    im, contigs = pt.stride_manager(case, engine_opt)
    refs = oracle(case, im, contigs)
    for c in range(len(contigs)):
        stride_columns(case, im, contigs, c)
    check_all(case, im, contigs, refs, windows=False)
    got = im.posterior_windows_exact(0, 100)
    assert np.abs(got - window_ref(refs[0], 100)).max() <= GAMMA_TOL


@pytest.mark.parametrize("case", ["stride:M64", "stride:M300", "stride:M520"])
def test_second_row_gives_the_same_bits(engine_opt, case):
    """8.: repetition, the other posterior products in between, poisoned allocations: the same bits - a second row that reads what
    the first left in the wavefront's scratch shows here."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = pt.stride_manager(case, engine_opt)
    nc = len(contigs)

    def all_products(im):
        return [{"pos": stride_columns(case, im, contigs, c), "w100": im.posterior_windows_exact(c, 100)} for c in range(nc)]

    first = all_products(im)
    for a, b in zip(all_products(im), first):
        pt.same_bits(a, b)
    for c in reversed(range(nc)):
        im.posterior_windows(c, 100)
        im.posterior_transitions(nc - 1 - c)
        im.posterior_sample_rows(c, 2, 5)
        assert np.array_equal(im.posterior_windows_exact(c, 100), first[c]["w100"])
        assert np.array_equal(im.posterior_positions(c), first[c]["pos"])
    ob = contigs[0]
    check_sub_grids(im, 0, first[0]["pos"], ob, f"{case} contig 0")
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im, contigs = pt.stride_manager(case, engine_opt)
    poisoned = all_products(im)
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(first, poisoned):
        pt.same_bits(b, a)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals, the Python layer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_unstructured_transition_matrix_is_refused(engine_opt):
    """9.: set_raw with a T of no structure: every call raises with a message that names the reason; the manager stays usable."""
    im, contigs = tg.run_case("eig_big:M96:unstructured", engine_opt)
    gam = im.gammas[0]
    for call in (lambda: im.posterior_positions(0), lambda: im.posterior_positions(1, 0, 1, 1),
                 lambda: im.posterior_position_summary(0, quantiles=(0.5,)), lambda: im.posterior_windows_exact(0, 100)):
        with pytest.raises(RuntimeError, match="semiseparable structure"):
            call()
    assert np.array_equal(im.posterior_columns(0, normalize=False), gam)


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100", "unbinned:M32"])
def test_argument_errors(engine_opt, case):
    """9.: every argument error raises RuntimeError with a message before anything is launched (position_waves of the last good call
    stays), and a following valid call still gives the same bits."""
    im, contigs = pt.manager(case, engine_opt)
    N, nc, M = int(contigs[0][:, 0].sum()), len(contigs), im.M
    good = products(im, 0)
    shape = (im.describe()["position_waves"], im.describe()["position_rows_walked"])

    def raises(call, match=None):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip(), "an error without a message"

    for c in (-1, nc, nc + 5):
        raises(lambda: im.posterior_positions(c), "contig")
        raises(lambda: im.posterior_position_summary(c), "contig")
        raises(lambda: im.posterior_windows_exact(c, 100), "contig")
    for kw in (dict(pos0=-1), dict(pos1=N + 2), dict(pos0=3, pos1=3), dict(pos0=4, pos1=2), dict(step=0), dict(step=-1), dict(pos0=N + 1)):
        raises(lambda: im.posterior_positions(0, **kw), "posterior positions")
        raises(lambda: im.posterior_position_summary(0, **kw), "posterior positions")
    for W in (0, -5):
        raises(lambda: im.posterior_windows_exact(0, W), "window_bp")
    raises(lambda: im.posterior_position_summary(0, quantiles=np.linspace(0.1, 0.9, 9)), "quantile")
    for q in (0.0, 1.0, -0.5, 1.5, np.nan):
        raises(lambda: im.posterior_position_summary(0, quantiles=(0.5, q)), "quantile")
    for bad in (np.inf, -np.inf, np.nan):
        w = weights_of(M)
        w[M // 2] = bad
        raises(lambda: im.posterior_position_summary(0, weights=w), "finite")
    raises(lambda: im.posterior_position_summary(0, weights=np.ones(M + 1)), "weights")
    assert (im.describe()["position_waves"], im.describe()["position_rows_walked"]) == shape
    pt.same_bits(products(im, 0), good)
    # the last E-step ran without save_gamma
    im.save_gamma = False
    im.E_step()
    for call in (lambda: im.posterior_positions(0), lambda: im.posterior_position_summary(0), lambda: im.posterior_windows_exact(0, 100)):
        with pytest.raises(RuntimeError, match="save_gamma"):
            call()
    im.save_gamma = True
    im.E_step()
    pt.same_bits(products(im, 0), good)
    # no E-step yet
    fresh, _ = pt.manager(case, engine_opt, estep=False)
    fresh.save_gamma = True
    for call in (lambda: fresh.posterior_positions(0), lambda: fresh.posterior_position_summary(0),
                 lambda: fresh.posterior_windows_exact(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    fresh.E_step()
    pt.same_bits(products(fresh, 0), good)


@pytest.mark.parametrize("pops", [1, 2])
def test_posterior_products_with_a_grid(tmp_path, pops):
    """10.: posterior_products(grid=step, exact_windows=True): the arrays of the manager calls; the default key set is today's; the
    file round-trips the new keys."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    from smcpp_amd.posterior import average_coal_times, posterior_products, save_products_npz
    a, s = synth.model_pieces()
    M, W, step = 16, 1000, 250
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
    hs, prods, im = posterior_products(*args, window=W, grid=step, exact_windows=True, return_manager=True, **kw)
    today = ["mean_tmrca", "path", "qstate", "sites", "windows"]
    new = ["grid_mean_tmrca", "grid_path", "grid_positions", "grid_qstate"]
    w = average_coal_times(model.model1 if pops == 2 else model, hs)
    for c, pr in enumerate(prods):
        assert sorted(pr) == sorted(today + new)
        total = int(pr["sites"].sum())
        npos = -(-(total + 1) // step)
        assert pr["grid_positions"].dtype == np.int64 and np.array_equal(pr["grid_positions"], np.arange(0, total + 1, step))
        assert pr["grid_path"].shape == (npos,) and pr["grid_path"].dtype == np.int32
        assert pr["grid_mean_tmrca"].shape == (npos,) and pr["grid_mean_tmrca"].dtype == np.float64
        assert pr["grid_qstate"].shape == (3, npos) and pr["grid_qstate"].dtype == np.int32
        sm = im.posterior_position_summary(c, weights=w, quantiles=(0.025, 0.5, 0.975), step=step)
        assert np.array_equal(pr["grid_path"], sm["argmax"]) and np.array_equal(pr["grid_mean_tmrca"], sm["mean"])
        assert np.array_equal(pr["grid_qstate"], sm["qstate"])
        assert np.array_equal(pr["windows"], im.posterior_windows_exact(c, W)) and pr["windows"].dtype == np.float64
        assert pr["windows"].shape == (M, -(-total // W))
        cols = im.posterior_positions(c, step=step)
        assert np.array_equal(pr["grid_path"], np.argmax(cols, axis=0))
    hs2, plain = posterior_products(*args, window=W, **kw)
    assert all(sorted(pr) == today for pr in plain)
    for c, (pr, pl) in enumerate(zip(prods, plain)):
        for k in ("mean_tmrca", "path", "qstate", "sites"):
            assert np.array_equal(pr[k], pl[k]), k
        assert np.array_equal(pl["windows"], im.posterior_windows(c, W))
    path = str(tmp_path / "products.npz")
    save_products_npz(path, hs, prods, ["a", "b"])
    z = np.load(path)
    for nm, pr in zip(("a", "b"), prods):
        for k in today + new:
            assert np.array_equal(z[f"{nm}_{k}"], pr[k]), (nm, k)
