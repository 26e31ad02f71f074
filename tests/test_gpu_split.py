"""`smc++ split` on the GPU: two-population managers at ONE hidden state against the C restatement, the reference's CI flow
end to end (vcf2smc -> estimate x 2 -> split -> posterior), and recovery of a known split from data drawn from the model."""
import json
import os
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCF = os.path.join(ROOT, "tests", "golden", "example.vcf.gz")


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _ci_files(d):
    """The four data sets of the reference's conda/run_test.sh, written as .smc.gz."""
    from smcpp_amd import vcf2smc as V
    specs = {"example.1": dict(pop1=("msp1", ["msp_0"])),
             "example.11": dict(pop1=("msp1", ["msp_1"])),
             "example.2": dict(pop1=("msp2", ["msp_0", "msp_3", "msp_4"]), d=["msp_0", "msp_0"]),
             "example.12": dict(pop1=("msp1", ["msp_1", "msp_2"]), pop2=("msp2", ["msp_3", "msp_4", "msp_0"]),
                                d=["msp_1", "msp_1"])}
    out = {}
    for nm, kw in specs.items():
        c, hdr = V.vcf2smc(VCF, "1", **kw)
        out[nm] = os.path.join(d, nm + ".smc.gz")
        V.write_smc(out[nm], c, hdr)
    return out


def _fixed_models(pids=("msp1", "msp2")):
    from smcpp_amd.analysis import SMCModel
    m1 = SMCModel([0.01, 0.08, 0.5, 2.0], 4000.0, pids[0])
    m2 = SMCModel([0.02, 0.15, 1.2], 4000.0, pids[1])
    m1[:] = np.log([1.5, 0.7, 1.1, 2.0])
    m2[:] = np.log([0.4, 0.9, 1.3])
    return m1, m2


def _pipeline(path):
    """base.py's pipeline without thinning / binning (what every split E-step sees)."""
    from smcpp_amd import data as D
    c = D.load_smc(path)
    c.data = D.compress_repeated_obs(c.data)
    return D.drop_small_contigs(D.break_long_spans(c, 100000), 100000)


@pytest.mark.gpu
def test_two_population_manager_at_one_hidden_state_matches_the_oracle(tmp_path):
    """A two-population manager (a = (2, 0)) at hidden states [0, inf] on the un-binned rows of the CI's example.12 (spans up to
    1e5): loglik, gamma sums, xi sums and Q against oracle/ on the manager's own pi / transition / emission to 1e-9; the
    emission of every fully observed key against the joint CSFS (`host_joint_csfs`) at two splits."""
    from oracle import oracle
    from smcpp_amd import _engine as E, _smcpp
    from smcpp_amd.analysis import SMCTwoPopulationModel
    cs = _pipeline(_ci_files(str(tmp_path))["example.12"])
    c = cs[0]
    assert tuple(c.a) == (2, 0) and tuple(c.pid) == ("msp1", "msp2")
    assert c.data[:, 0].max() > 1000
    obs = [np.ascontiguousarray(x.data, dtype=np.int32) for x in cs]
    n1, n2 = c.n
    m1, m2 = _fixed_models()
    theta = 1e-4
    for pol, split in ((0.5, 0.3), (0.0, 0.3), (0.0, 0.9)):
        model = SMCTwoPopulationModel(m1, m2, split)
        im = _smcpp.PyTwoPopInferenceManager(n1, n2, 2, 0, obs, [0.0, np.inf], ("msp1", "msp2"), pol)
        im.model = model
        im.theta = theta; im.rho = theta; im.alpha = 1
        im.E_step()
        assert im.M == 1
        keys = im.keys
        ep = im.emission_probs
        Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
        q = np.zeros(4)
        ll = 0.0
        for ci, ob in enumerate(obs):
            o = oracle.estep(im.pi, im.transition, keys, Etab, ob)
            ll += o["loglik"]
            q += o["q"]
            assert _rel(im.xisums[ci], o["xisum"]) <= 1e-9
            gs = im.gamma_sums[ci]
            assert sorted(gs) == sorted(o["gamma_sums"])
            for k, v in o["gamma_sums"].items():
                assert _rel(gs[k], v) <= 1e-9, k
        assert abs(im.loglik() - ll) <= 1e-9 * abs(ll), (im.loglik(), ll)
        qs = np.array(im.Q(separate=True))
        assert np.all(np.abs(qs - q) <= 1e-9 * np.maximum(np.abs(q), 1e-300)), (qs, q)
        if pol == 0.5:
            # the compiled Cython binding reads the same model through the same for_pop / stepwise_values / s
            from smcpp_amd import _smcpp_cy
            imc = _smcpp_cy.PyTwoPopInferenceManager(n1, n2, 2, 0, obs, [0.0, np.inf], ("msp1", "msp2"), pol)
            imc.model = model
            imc.theta = theta; imc.rho = theta; imc.alpha = 1
            imc.E_step()
            assert abs(float(imc.loglik()) - im.loglik()) <= 1e-12 * abs(im.loglik())
            del imc
        if pol == 0.0:
            # emission of a fully observed key = f * J[a1, b1, a2, b2], f = -expm1(-theta tau) / tau, tau = sum of J
            # (incorporate_theta, inference_manager.cpp); J = the joint CSFS of the model's two populations at this split
            p1, p2 = model.for_pop("msp1"), model.for_pop("msp2")
            J = E.host_joint_csfs(n1, n2, 2, 0, np.array([0.0, np.inf]), (p1.stepwise_values(), p1.s),
                                  (p2.stepwise_values(), p2.s), split)[0]
            tau = J.sum()
            f = -np.expm1(-theta * tau) / tau
            checked = 0
            for k in keys.tolist():
                a1, b1, nb1, a2, b2, nb2 = k
                if a1 < 0 or nb1 != n1 or nb2 != n2 or a1 + b1 + b2 == 0 or (a1 == 2 and b1 == n1 and b2 == n2):
                    continue
                want = f * J[a1, b1, a2, b2]
                if want < 1e-9:
                    continue
                assert abs(ep[tuple(k)][0] - want) <= 1e-9 * want, (k, ep[tuple(k)], want)
                checked += 1
            assert checked >= 5


def _estimate(path, outdir, base, **kw):
    from smcpp_amd.analysis import Analysis, EstimateArgs
    args = EstimateArgs(multi=True, em_iterations=1, knots=3, mu=1.25e-8, outdir=outdir, base=base, **kw)
    an = Analysis([path], args)
    an.run()
    return os.path.join(outdir, base + ".final.json")


@pytest.mark.gpu
def test_split_reproduces_the_reference_ci_flow(tmp_path):
    """conda/run_test.sh: vcf2smc (four files) -> estimate pop 1 (--unfold --knots 3 --timepoints 33 1000) and pop 2 (-p 0.01
    -r 1e-8 --knots 3) -> split on all four files -> posterior of example.12 under the split model."""
    from smcpp_amd import data as D
    from smcpp_amd.analysis import SplitAnalysis, SplitArgs, SMCTwoPopulationModel, model_from_dict
    from smcpp_amd.posterior import posterior
    f = _ci_files(str(tmp_path))
    np.random.seed(0)
    for d in ("out1", "out2", "split"):
        os.makedirs(tmp_path / d)
    j1p = _estimate(f["example.1"], str(tmp_path / "out1"), "model", unfold=True, timepoints=(33, 1000))
    j2p = _estimate(f["example.2"], str(tmp_path / "out2"), "pop2", polarization_error=0.01, r=1e-8)
    j1, j2 = json.load(open(j1p)), json.load(open(j2p))
    t0 = time.perf_counter()
    an = SplitAnalysis([f[k] for k in ("example.1", "example.11", "example.12", "example.2")],
                       SplitArgs(pop1=j1p, pop2=j2p, outdir=str(tmp_path / "split")))
    t_init = time.perf_counter() - t0
    ims = an.inference_managers
    assert sorted(ims) == [("msp1",), ("msp1", "msp2"), ("msp2",)]
    assert all(im.M == 1 for im in ims.values())
    max_split = j2["model"]["knots"][-1]
    assert an.max_split == max_split and an.model.split == max_split / 2
    ncalls = [0]
    q_orig = an.Q

    def counted():
        ncalls[0] += 1
        return q_orig()
    an.Q = counted
    t0 = time.perf_counter()
    an.run()
    t_run = time.perf_counter() - t0
    an.Q = q_orig
    out = json.load(open(tmp_path / "split" / "model.final.json"))
    # ---- the file, field by field ----
    assert sorted(out) == ["alpha", "hidden_states", "model", "rho", "theta"]
    assert out["alpha"] == 1 and out["theta"] == j1["theta"] == j2["theta"] and out["rho"] == j1["rho"]
    assert out["hidden_states"] == {**j1["hidden_states"], **j2["hidden_states"]}
    mo = out["model"]
    assert sorted(mo) == ["class", "model1", "model2", "split"] and mo["class"] == "SMCTwoPopulationModel"
    s_hat = mo["split"]
    assert 0 < s_hat < max_split
    # model1 / model2 are the inputs up to ScaleOptimizer's common shift of every log size, |shift| <= 1
    shifts = []
    for mk, jin in (("model1", j1), ("model2", j2)):
        mi = jin["model"]
        assert {k: v for k, v in mo[mk].items() if k != "y"} == {k: v for k, v in mi.items() if k != "y"}
        shifts.append(np.asarray(mo[mk]["y"]) - np.asarray(mi["y"]))
    sh = np.concatenate(shifts)
    assert np.all(np.abs(sh - sh[0]) <= 1e-12) and abs(sh[0]) <= 1.0
    # ---- the split search: with the E-step statistics of the run held fixed and the models as the search saw them ----
    m = an.model
    m[:] = np.r_[j1["model"]["y"], j2["model"]["y"]]
    m.split = s_hat
    q_hat = an.Q()
    t0 = time.perf_counter()
    grid = []
    for s in np.linspace(0, max_split, 27)[1:-1]:
        m.split = s
        grid.append(-an.Q())
    t_q = (time.perf_counter() - t0) / 25
    assert -q_hat <= min(grid) + 1e-6 * abs(q_hat), (q_hat, grid)
    # ---- posterior of example.12 under the dumped model (commands/posterior.py:60-111) ----
    sm = model_from_dict(out["model"])
    assert isinstance(sm, SMCTwoPopulationModel)
    c12 = D.load_smc(f["example.12"])
    M = 8
    hs, gammas, sites, paths = posterior(sm, [c12.data], M, tuple(c12.n), out["theta"], out["rho"], alpha=out["alpha"],
                                         a=tuple(c12.a))
    assert hs.shape == (M + 1,) and hs[0] == 0 and np.isinf(hs[-1])
    # the manager's rows are the contig's with one missing row in front; gammas carry one column more than rows
    assert sites[0].shape == (len(c12.data) + 1,) and gammas[0].shape == (M, len(c12.data) + 2)
    assert paths[0].shape == (len(c12.data) + 2,) and np.all((paths[0] >= 0) & (paths[0] < M))
    assert np.allclose(gammas[0].sum(axis=0), 1.0, atol=1e-9)
    assert sites[0][0] == 1 and np.array_equal(sites[0][1:], c12.data[:, 0])
    rows = {p: sum(len(o) for o in im.observations) for p, im in ims.items()}
    print(f"\n[split timing] init {t_init * 1e3:.1f} ms, run (E-step of 3 managers + split search + scale search, "
          f"{ncalls[0]} Q evaluations) {t_run * 1e3:.1f} ms, one Q(split) over 3 managers {t_q * 1e3:.2f} ms; rows {rows}; "
          f"split {s_hat:.6g} of max {max_split:.6g}")


def _draw(im, catalog, N, rng):
    """N positions drawn i.i.d. from the M = 1 emission distribution over the fully observed keys of `catalog`, laid out as
    un-binned rows: the drawn non-monomorphic sites at random positions, monomorphic runs between them."""
    ep = im.emission_probs
    p = np.array([ep[tuple(int(x) for x in k)][0] for k in catalog])
    # (the all-derived key folds into the monomorphic one or not - take the reading under which the table is a distribution)
    na = np.array([k[0] == 2 and all(k[1 + 3 * j] == k[2 + 3 * j] for j in range(len(k) // 3)) for k in catalog])
    total_all, total_rest = p.sum(), p[~na].sum()
    use = np.ones(len(p), bool) if abs(total_all - 1) <= abs(total_rest - 1) else ~na
    assert abs(p[use].sum() - 1) <= 1e-6, (total_all, total_rest)
    p = np.where(use, p, 0.0)
    p /= p.sum()
    counts = rng.multinomial(N, p)
    mono = [i for i, k in enumerate(catalog) if k[0] == 0 and all(k[1 + 3 * j] == 0 for j in range(len(k) // 3))][0]
    site_keys = np.repeat(np.arange(len(catalog)), np.where(np.arange(len(catalog)) == mono, 0, counts))
    rng.shuffle(site_keys)
    gaps = rng.multinomial(counts[mono], np.full(len(site_keys) + 1, 1.0 / (len(site_keys) + 1)))
    rows = []
    mrow = list(catalog[mono])
    for g, k in zip(gaps, site_keys):
        if g > 0:
            rows.append([int(g)] + mrow)
        rows.append([1] + list(catalog[k]))
    if gaps[-1] > 0:
        rows.append([int(gaps[-1])] + mrow)
    out = np.array(rows, dtype=np.int32)
    assert out[:, 0].sum() == N
    return out


@pytest.mark.gpu
def test_split_recovers_a_known_split():
    """Data drawn i.i.d. per position from the M = 1 emission distributions of the three managers (pop 1, pop 2, the joint
    spectrum with a = (2, 0)) at a known split s*, 2e7 positions each; the split search must return s* within

        tol = 5 / sqrt(I) + 2e-5,   I = -d2Q/ds2 at s*

    At M = 1 the HMM has a single state (pi = T = 1), so Q(s) with the E-step statistics held fixed IS the log-likelihood
    of the i.i.d. data; its observed information I gives the asymptotic standard error 1 / sqrt(I) of the maximum-likelihood
    split (central second difference with step 1e-3 s*); 5 standard errors plus the bounded search's xatol (1e-5) twice."""
    from smcpp_amd import _smcpp, data as D
    from smcpp_amd.analysis import SMCTwoPopulationModel, SplitAnalysis, SplitArgs
    rng = np.random.default_rng(2026)
    m1, m2 = _fixed_models(("p1", "p2"))
    s_true, theta, N = 0.35, 1e-3, 20_000_000
    model = SMCTwoPopulationModel(m1, m2, s_true)
    n, n1, n2 = 4, 2, 4
    specs = [(("p1",), [n], [2]), (("p2",), [n], [2]), (("p1", "p2"), [n1, n2], [2, 0])]
    contigs = []
    for pid, nn, aa in specs:
        if len(pid) == 1:
            catalog = [(a, b, nn[0]) for a in range(3) for b in range(nn[0] + 1)]
        else:
            catalog = [(a, b1, nn[0], 0, b2, nn[1]) for a in range(3) for b1 in range(nn[0] + 1) for b2 in range(nn[1] + 1)]
        cat = np.array([[1] + list(k) for k in catalog], dtype=np.int32)
        if len(pid) == 1:
            im = _smcpp.PyOnePopInferenceManager(nn[0], [cat], [0.0, np.inf], pid, 0.0)
        else:
            im = _smcpp.PyTwoPopInferenceManager(nn[0], nn[1], 2, 0, [cat], [0.0, np.inf], pid, 0.0)
        im.model = model
        im.theta = theta; im.rho = theta; im.alpha = 1
        im.E_step()
        contigs.append(D.Contig(data=_draw(im, catalog, N, rng), pid=pid, n=list(nn), a=list(aa)))
        del im
    fits = []
    for mm, pid in ((m1, "p1"), (m2, "p2")):
        fits.append({"theta": theta, "rho": theta, "alpha": 1, "model": mm.to_dict(), "hidden_states": {pid: [0.0, np.inf]}})
    an = SplitAnalysis(contigs, SplitArgs(pop1=fits[0], pop2=fits[1], polarization_error=0.0))
    assert an.max_split == m2.knots[-1] and len(an.inference_managers) == 3
    an.E_step()
    res = an.optimize_split()
    s_hat = float(res.x)
    h = 1e-3 * s_true
    q = []
    for s in (s_true - h, s_true, s_true + h):
        an.model.split = s
        q.append(an.Q())
    info = -(q[0] - 2 * q[1] + q[2]) / h ** 2
    assert info > 0
    se = 1 / np.sqrt(info)
    assert se < 0.1 * s_true, se                       # the data do inform the split
    tol = 5 * se + 2e-5
    print(f"\n[split recovery] s* {s_true}, s_hat {s_hat:.6f}, standard error {se:.3g}, tol {tol:.3g}, rows "
          f"{[len(c.data) for c in an.contigs]}")
    assert abs(s_hat - s_true) <= tol, (s_hat, s_true, tol)
