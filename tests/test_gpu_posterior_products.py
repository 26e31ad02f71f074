"""The device-side posterior products - `posterior_columns`, `posterior_summary`, `posterior_windows` (smcpp_amd/csrc/posterior_dev.hpp)
and `posterior.posterior_products` - on every column of every contig of the per-row posterior routes of tests/test_gpu_gamma.py.

The truth is `gamma = im.gammas[c]`, which the existing suite pins against the reference's restatement, pushed through the numpy
oracles of tests/postref.py.  Managers come from `test_gpu_gamma.run_case`, which asserts the route each case runs; every case but
the `eig_b:*` ones (six contigs of 9 to 230 rows, ragged batches per key) holds contigs of one and of two rows.  Bounds (eps = 2^-52):

  un-normalised columns   bitwise equal to gamma[:, start:stop:step]
  normalised columns      fp64: relative 2 M eps (both sides add M non-negative terms in some order and divide once), zero where gamma
                          is zero; fp32: relative 2^-23, absolute float32 tiny
  argmax                  equal to np.argmax(gamma, axis=0) and to im.gamma_argmax(c)
  colsum                  relative M eps;  mean: relative 4 M eps
  quantile states         with F = cumsum(p) and t = 2 M eps: F[m] >= q - t and (m == 0 or F[m - 1] < q + t), no column skipped
  windows                 relative (W + 2 M + 8) eps against the per-base-pair oracle (sums of at most W non-negative terms on either
                          side); every window column sums to 1 within the same bound
"""
import numpy as np
import pytest

import postref
import test_gpu_gamma as tg

pytestmark = pytest.mark.gpu

EPS = postref.EPS
CASES = ["eig_b:M1", "eig_b:M13", "scan:M64", "scan:M300", "eig_big:M96:unstructured", "cut:M100", "pieces:M65", "twopop:M48"]
SHORT = {"eig_b:M1", "eig_b:M13", "cut:M100"}                  # contigs short enough for one window per base pair
Q3 = (0.025, 0.5, 0.975)
Q8 = (0.01, 0.025, 0.1, 0.25, 0.5, 0.75, 0.9, 0.975)


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _coal_weights(M):
    """The average coalescence time of each hidden state under the synthetic one-population model (finite in the last state too)."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    from smcpp_amd.posterior import average_coal_times
    a, s = synth.model_pieces()
    w = average_coal_times(PiecewiseModel(a, s, 1e4, "pop1"), synth.hidden_states(M))
    assert w.shape == (M,) and np.all(np.isfinite(w)) and np.all(w > 0)
    return w


def _selections(L):
    """Column selections over 0 .. L: all; [0, 1); [L, L + 1); start > 0 with step 7; a stop that the step does not hit."""
    miss = next(s for s in range(2, 12) if (L + 1) % s)
    return [(0, None, 1), (0, 1, 1), (L, L + 1, 1), (1, None, 7), (0, L + 1, miss)]


def _rel_ok(got, want, rel, absolute=0.0):
    got = np.asarray(got, dtype=np.float64)
    return np.abs(got - want) <= rel * np.abs(want) + absolute


def check_columns(im, c, gamma):
    M, ncol = gamma.shape
    L = ncol - 1
    p = gamma / gamma.sum(axis=0)
    full = im.posterior_columns(c)
    full32 = im.posterior_columns(c, dtype=np.float32)
    raw = im.posterior_columns(c, normalize=False)
    assert full.dtype == np.float64 and full32.dtype == np.float32 and raw.dtype == np.float64
    assert full.shape == full32.shape == raw.shape == (M, L + 1)
    assert np.array_equal(raw, gamma), f"contig {c}: un-normalised columns differ from gammas in {int(np.sum(raw != gamma))} entries"
    bad = ~_rel_ok(full, p, 2 * M * EPS)
    assert not bad.any(), f"contig {c}: {int(bad.sum())} normalised entries off, worst {np.max(np.abs(full - p) / np.maximum(p, 1e-300)) / EPS:.1f} eps"
    assert np.all(full[gamma == 0.0] == 0.0)
    bad = ~_rel_ok(full32, p, 2.0 ** -23, float(np.finfo(np.float32).tiny))
    assert not bad.any(), f"contig {c}: {int(bad.sum())} fp32 entries off"
    raw32 = im.posterior_columns(c, dtype=np.float32, normalize=False)
    assert raw32.dtype == np.float32 and _rel_ok(raw32, gamma, 2.0 ** -23, float(np.finfo(np.float32).tiny)).all()
    for start, stop, step in _selections(L):
        sl = slice(start, stop, step)
        assert np.array_equal(im.posterior_columns(c, start, stop, step, normalize=False), gamma[:, sl]), (c, start, stop, step)
        assert np.array_equal(im.posterior_columns(c, start, stop, step), full[:, sl]), (c, start, stop, step)
        assert np.array_equal(im.posterior_columns(c, start, stop, step, dtype=np.float32), full32[:, sl]), (c, start, stop, step)


def check_summary(im, c, gamma, weights):
    M, ncol = gamma.shape
    L = ncol - 1
    fulls = []
    for w in weights:
        ref = postref.summary(gamma, weights=w, quantiles=Q3)
        s = im.posterior_summary(c, weights=w, quantiles=Q3)
        assert sorted(s) == ["argmax", "colsum", "mean", "qstate"]
        assert s["argmax"].shape == s["colsum"].shape == s["mean"].shape == (L + 1,) and s["qstate"].shape == (3, L + 1)
        assert np.array_equal(s["argmax"], ref["argmax"]), f"contig {c}: argmax differs on {int(np.sum(s['argmax'] != ref['argmax']))} columns"
        assert np.array_equal(s["argmax"], im.gamma_argmax(c))
        assert _rel_ok(s["colsum"], ref["colsum"], M * EPS).all()
        bad = ~_rel_ok(s["mean"], ref["mean"], 4 * M * EPS)
        assert not bad.any(), f"contig {c}: {int(bad.sum())} means off, worst {np.max(np.abs(s['mean'] - ref['mean']) / ref['mean']) / EPS:.1f} eps"
        for k, q in enumerate(Q3):
            ok = postref.quantile_ok(gamma, s["qstate"][k], q, 2 * M * EPS)
            assert ok.all(), f"contig {c}: level {q}: {int((~ok).sum())} columns off"
        fulls.append(s)
    # eight levels at once; the three levels are rows of it; no weights: no mean
    s8 = im.posterior_summary(c, quantiles=Q8)
    assert sorted(s8) == ["argmax", "colsum", "qstate"] and s8["qstate"].shape == (8, L + 1)
    for k, q in enumerate(Q8):
        assert postref.quantile_ok(gamma, s8["qstate"][k], q, 2 * M * EPS).all(), (c, q)
    for k, q in enumerate(Q3):
        assert np.array_equal(s8["qstate"][Q8.index(q)], fulls[0]["qstate"][k])
    assert np.all((s8["qstate"] >= 0) & (s8["qstate"] < M)) and np.all(np.diff(s8["qstate"], axis=0) >= 0)
    s0 = im.posterior_summary(c)
    assert s0["qstate"].shape == (0, L + 1) and np.array_equal(s0["colsum"], fulls[0]["colsum"])
    # the column sums of the columns product are the same numbers
    for start, stop, step in _selections(L):
        sl = slice(start, stop, step)
        s = im.posterior_summary(c, weights=weights[0], quantiles=Q3, start=start, stop=stop, step=step)
        for key in ("colsum", "argmax", "mean"):
            assert np.array_equal(s[key], fulls[0][key][sl]), (c, key, start, stop, step)
        assert np.array_equal(s["qstate"], fulls[0]["qstate"][:, sl]), (c, start, stop, step)


def window_widths(total, short):
    """W = 7, 100, wider than the contig, one that leaves a partial last window (a contig of one or two base pairs has none), and 1
    on the short cases."""
    ws = [7, 100, total + 13]
    if total > 53:
        ws.append(next(w for w in (50, 51, 52, 53) if total % w))
    elif total > 2:
        ws.append(total - 1)
    if short:
        ws.append(1)
    return ws


def check_windows(im, c, gamma, spans, short):
    M = gamma.shape[0]
    total = int(np.sum(spans))
    for W in window_widths(total, short):
        got = im.posterior_windows(c, W)
        want = postref.windows_repeat(gamma, spans, W)
        assert got.shape == want.shape == (M, -(-total // W)), (c, W, got.shape)
        tol = (W + 2 * M + 8) * EPS
        bad = ~_rel_ok(got, want, tol)
        assert not bad.any(), f"contig {c}, W = {W}: {int(bad.sum())} entries off, worst {np.max(np.abs(got - want) / np.maximum(want, 1e-300)) / EPS:.1f} eps"
        assert np.all(np.abs(got.sum(axis=0) - 1.0) <= tol), (c, W, float(np.max(np.abs(got.sum(axis=0) - 1.0))))
        if W == 1:
            assert got.shape[1] == total


def check_all(im, contigs, short, weights):
    gams = im.gammas
    assert len(gams) == len(contigs)
    for c, ob in enumerate(contigs):
        assert gams[c].shape == (im.M, len(ob) + 1)
        check_columns(im, c, gams[c])
        check_summary(im, c, gams[c], weights)
        check_windows(im, c, gams[c], ob[:, 0], short)


def products(im, c, w):
    """Every product of contig c, flattened into one dict of arrays (for bit comparisons)."""
    out = {"p": im.posterior_columns(c), "p32": im.posterior_columns(c, dtype=np.float32), "raw": im.posterior_columns(c, normalize=False),
           "w100": im.posterior_windows(c, 100), "w7": im.posterior_windows(c, 7)}
    out.update({"s_" + k: v for k, v in im.posterior_summary(c, weights=w, quantiles=Q8).items()})
    return out


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        assert np.all(np.isfinite(a[k])), k


def _weights(M):
    return [np.random.default_rng(1000 + M).random(M) + 0.1, _coal_weights(M)]


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_products_on_every_column(engine_opt, case):
    """Columns, summaries and windows of every contig of one per-row posterior route against the oracles."""
    im, contigs = tg.run_case(case, engine_opt)
    if tg.CASES[case][0] != "batches":
        assert any(len(ob) == 1 for ob in contigs) and any(len(ob) == 2 for ob in contigs)
    check_all(im, contigs, case in SHORT, _weights(im.M))


@pytest.mark.parametrize("case", CASES)
def test_order_and_reuse(engine_opt, case):
    """Contig 0, contig 1, contig 0 again (rows cut into pieces share one merge buffer between contigs); products, im.gammas, products;
    a second E-step with other parameters; an E-step without save_gamma: every call raises and the process goes on."""
    im, contigs = tg.run_case(case, engine_opt)
    M = im.M
    w = _weights(M)[0]
    a0 = products(im, 0, w)
    a1 = products(im, 1, w)
    same_bits(products(im, 0, w), a0)
    g_old = im.gammas
    same_bits(products(im, 0, w), a0)
    same_bits(products(im, 1, w), a1)
    assert np.array_equal(a0["raw"], g_old[0]) and np.array_equal(a1["raw"], g_old[1])
    # other parameters
    if tg.CASES[case][0] == "unstructured":
        keys = im.keys
        ep = im.emission_probs
        T = 0.9 * im.transition + 0.1 * np.eye(M)               # (same eigenvectors: still a real spectrum)
        im.set_raw(im.pi, T, keys, np.array([ep[tuple(k)] for k in keys.tolist()]))
    else:
        im.rho = im.rho * 1.7
    im.E_step()
    g_new = im.gammas
    assert M == 1 or not np.array_equal(g_new[0], g_old[0])         # (one state: gamma is the span whatever the parameters)
    check_all(im, contigs, False, _weights(M))
    # without save_gamma
    im.save_gamma = False
    im.E_step()
    for call in (lambda: im.posterior_columns(0), lambda: im.posterior_summary(0, weights=w, quantiles=Q3),
                 lambda: im.posterior_windows(0, 100)):
        with pytest.raises(RuntimeError, match="save_gamma"):
            call()
    assert np.all(np.isfinite(im.logliks())) and im.gammas[0].shape == (M, 1)
    im.save_gamma = True
    im.E_step()
    again = products(im, 0, w)
    same_bits(products(im, 0, w), again)
    assert np.array_equal(again["raw"], im.gammas[0]) and np.array_equal(im.posterior_columns(1, normalize=False), im.gammas[1])
    check_all(im, contigs, False, _weights(M))


@pytest.mark.parametrize("case", ["eig_b:M13", "cut:M100"])
def test_argument_errors(engine_opt, case):
    """Every argument error raises RuntimeError with a message before anything is launched, and a following valid call still works."""
    im, contigs = tg.run_case(case, engine_opt)
    M = im.M
    L = len(contigs[0])
    nc = len(contigs)
    w = np.ones(M)
    good = products(im, 0, w)

    def raises(call):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value).strip(), "an error without a message"
        same_bits(products(im, 0, w), good)

    for c in (-1, nc, nc + 5):
        raises(lambda: im.posterior_columns(c))
        raises(lambda: im.posterior_summary(c))
        raises(lambda: im.posterior_windows(c, 100))
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(start=4, stop=2), dict(step=0), dict(step=-1),
               dict(start=L + 1)):
        raises(lambda: im.posterior_columns(0, **kw))
        raises(lambda: im.posterior_summary(0, **kw))
    for W in (0, -5):
        raises(lambda: im.posterior_windows(0, W))
    raises(lambda: im.posterior_summary(0, quantiles=np.linspace(0.1, 0.9, 9)))
    for q in (0.0, 1.0, 1.5, -0.1, np.nan):
        raises(lambda: im.posterior_summary(0, quantiles=(0.5, q)))
    for bad in (np.inf, -np.inf, np.nan):
        wb = np.ones(M); wb[M // 2] = bad
        raises(lambda: im.posterior_summary(0, weights=wb))
    # no E-step yet
    kind, Mc, switches, _, _ = tg.CASES[case]
    cont, theta, rho = tg.case_inputs(kind, Mc)
    fresh = tg._onepop(Mc, cont, theta, rho)
    fresh.save_gamma = True
    for call in (lambda: fresh.posterior_columns(0), lambda: fresh.posterior_summary(0), lambda: fresh.posterior_windows(0, 100)):
        with pytest.raises(RuntimeError, match="E-step"):
            call()
    fresh.E_step()
    assert np.array_equal(fresh.posterior_columns(0, normalize=False), fresh.gammas[0])


def test_poisoned_allocations(engine_opt):
    """scan:M64 with every fresh allocation filled with 0xFF bytes: no NaN and the same bits as without - no output or scratch
    buffer of the products is read before it is written."""
    case = "scan:M64"
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = tg.run_case(case, engine_opt)
    w = _weights(im.M)[1]
    clean = [products(im, c, w) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    im, contigs = tg.run_case(case, engine_opt)
    poisoned = [products(im, c, w) for c in range(len(contigs))]
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(clean, poisoned):
        same_bits(b, a)


def test_cython_manager_gives_the_same_bits(engine_opt):
    """The compiled Cython manager (set-up as in tests/test_cython_binding.py) against the ctypes one on scan:M64."""
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    im, contigs = tg.run_case("scan:M64", engine_opt)
    M = im.M
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(tg.N, contigs, synth.hidden_states(M), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1", differentiable=[])
    im2.theta = tg.TH_B; im2.rho = tg.RH_B; im2.alpha = 1.0
    im2.save_gamma = True
    im2.E_step()
    w = _weights(M)[1]
    for c in range(len(contigs)):
        assert np.array_equal(im2.gammas[c], im.gammas[c])
        same_bits(products(im2, c, w), products(im, c, w))
        for start, stop, step in _selections(len(contigs[c])):
            assert np.array_equal(im2.posterior_columns(c, start, stop, step), im.posterior_columns(c, start, stop, step))
            sa = im.posterior_summary(c, weights=w, quantiles=Q3, start=start, stop=stop, step=step)
            sb = im2.posterior_summary(c, weights=w, quantiles=Q3, start=start, stop=stop, step=step)
            same_bits({k: np.asarray(v) for k, v in sb.items()}, sa)
    assert sorted(im2.posterior_summary(0)) == ["argmax", "colsum", "qstate"]
    with pytest.raises(RuntimeError):
        im2.posterior_columns(0, start=-1)
    with pytest.raises(RuntimeError):
        im2.posterior_windows(len(contigs), 100)


@pytest.mark.parametrize("pops", [1, 2])
def test_posterior_products(tmp_path, pops):
    """posterior_products on the two synthetic contigs of test_gpu_gamma.test_save_npz_product against posterior()'s matrix."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    from smcpp_amd.posterior import average_coal_times, posterior, posterior_products, save_products_npz
    a, s = synth.model_pieces()
    M, W = 16, 1000
    if pops == 1:
        model = PiecewiseModel(a, s, 1e4, "pop1")
        raw = [synth.synth_posterior_contig(200, tg.N, seed=21), synth.synth_posterior_contig(90, tg.N, seed=22)]
        args, kw = (model, raw, M, tg.N, tg.TH_U, tg.RH_U), {}
        dist = model
    else:
        a8, s8 = synth.model_pieces(8)                                # (the set-up of test_gpu_parity's two-population posterior)
        m1 = PiecewiseModel(a8, s8, 1e4, pid="pop1")
        m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(4)), s8[:4], 1e4, pid="pop2")
        model = TwoPopulationModel(m1, m2, 0.4)
        raw = [synth.synth_contig_twopop(3, 300_000, 4, 3), synth.synth_contig_twopop(4, 150_000, 4, 3)]
        args, kw = (model, raw, M, (4, 3), synth.THETA, synth.RHO), dict(a=(2, 0))
        dist = m1
    hs, gammas, sites, paths = posterior(*args, **kw)
    hs2, prods = posterior_products(*args, window=W, **kw)
    assert np.array_equal(hs, hs2) and len(prods) == len(raw)
    w = average_coal_times(dist, hs)
    assert np.all(np.isfinite(w)) and np.all(np.diff(w) > 0)
    for g, st, path, pr in zip(gammas, sites, paths, prods):
        assert sorted(pr) == ["mean_tmrca", "path", "qstate", "sites", "windows"]
        ncol = g.shape[1]
        assert np.array_equal(pr["sites"], st) and np.array_equal(pr["path"], np.asarray(path))
        ref = postref.summary(g, weights=w, quantiles=Q3)
        assert pr["mean_tmrca"].shape == (ncol,) and _rel_ok(pr["mean_tmrca"], ref["mean"], 4 * M * EPS).all()
        assert pr["qstate"].shape == (3, ncol)
        for k, q in enumerate(Q3):
            assert postref.quantile_ok(g, pr["qstate"][k], q, 2 * M * EPS).all()
        want = postref.windows_repeat(g, st, W)                      # (position 0 of the window axis: the prepended missing row)
        assert pr["windows"].shape == want.shape and _rel_ok(pr["windows"], want, (W + 2 * M + 8) * EPS).all()
    _, no_windows = posterior_products(*args, quantiles=(0.5,), **kw)
    assert all("windows" not in pr and pr["qstate"].shape[0] == 1 for pr in no_windows)
    names = ["chr1.smc.gz", "chr2.smc.gz"]
    path = tmp_path / "products.npz"
    save_products_npz(str(path), hs, prods, names)
    z = np.load(str(path))
    keys = ["sites", "path", "mean_tmrca", "qstate", "windows"]
    assert sorted(z.files) == sorted(["hidden_states"] + [f"{nm}_{k}" for nm in names for k in keys])
    assert np.array_equal(z["hidden_states"], hs)
    for nm, pr in zip(names, prods):
        for k in keys:
            assert z[f"{nm}_{k}"].dtype == pr[k].dtype and np.array_equal(z[f"{nm}_{k}"], pr[k]), (nm, k)
        assert z[nm + "_path"].dtype == np.int32 and z[nm + "_qstate"].dtype == np.int32
        assert z[nm + "_mean_tmrca"].dtype == np.float64 and z[nm + "_windows"].dtype == np.float64
