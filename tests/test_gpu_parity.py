"""Parity of the HIP E-step (through the C ABI) with the golden vectors emitted by the compiled reference and with
the C restatement (oracle/) on the same inputs.

Tolerances (BASELINE.json north_star):
  * log-likelihood: 1e-6 relative (observed ~1e-9: alpha_hat is float in the reference and here);
  * posterior decoding indices argmax_m gamma[m, ell]: identical on every column whose reference top-1/top-2
    relative margin exceeds 1e-5 (columns below it are reported);
  * xisum / gamma_sums / Q: 5e-6 relative — the float-alpha noise floor of the reference itself.
"""
import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

LL_TOL = 1e-6
STAT_TOL = 5e-6


def make_im(g, **kw):
    from smcpp_amd import _smcpp
    obs = np.ascontiguousarray(g["obs"], dtype=np.int32)
    if obs.shape[1] == 4:
        im = _smcpp.PyOnePopInferenceManager(int(g["n"]), [obs], g["hs"], ("pop1",), float(g["pol"]))
    else:
        im = _smcpp.PyTwoPopInferenceManager(10, 10, 2, 0, [obs], g["hs"], ("pop1", "pop2"), float(g["pol"]))
    im.theta = float(g["theta"]); im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
    im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
    return im


GAMMA_TOL = 2e-5          # per entry of a per-row posterior, times the row's span
GAMMA_LARGE_TOL = 1e-4    # relative, on the entries that hold 1e-3 of their column's mass or more
GAMMA_SUM_RTOL = 1e-9     # a column sums to its row's span (hmm.cpp:113-121 normalises to it)
GAMMA_MARGIN = 1e-5       # decoded index identical where top-1 minus top-2 exceeds this times the span

_ORACLE = {}              # (parameters, contig, save_gamma) -> the restatement's E-step, shared by every test of the process


def oracle_estep(pi, T, keys, E, obs, save_gamma=True):
    """oracle.estep, run once per (parameters, contig) in a process: cases that share a setup reuse it."""
    import hashlib
    from oracle import oracle
    h = hashlib.sha1(b"gamma" if save_gamma else b"")
    for x in (pi, T, keys, E, obs):
        x = np.ascontiguousarray(x)
        h.update(str((x.dtype, x.shape)).encode())
        h.update(x.tobytes())
    key = h.hexdigest()
    if key not in _ORACLE:
        _ORACLE[key] = oracle.estep(pi, T, keys, E, obs, save_gamma=save_gamma)
    return _ORACLE[key]


def check_gamma_columns(gam, ref, obs, arg_dev=None, label=""):
    """Every column of a per-row posterior matrix `gam` ([M, L + 1], column l >= 1 the row of span s_l) against the restatement's
    `ref`, each at the scale of its own row's span:
      * max_i |gam - ref| <= 2e-5 s_l (column 0, alpha_0 o beta_0, which is not normalised: 2e-5 of its largest entry);
      * the column sums to s_l to 1e-9 relative;
      * entries with ref >= 1e-3 s_l to 1e-4 relative;
      * the decoded index equals the reference's wherever its top-1 / top-2 gap exceeds 1e-5 s_l, and `arg_dev` (the device's
        decode, when given) equals gam.argmax(0) on every column.
    Returns the worst value of each measure (printed with `label`)."""
    obs = np.asarray(obs)
    M, ncol = ref.shape
    assert gam.shape == ref.shape == (M, len(obs) + 1), (gam.shape, ref.shape, len(obs))
    assert np.all(np.isfinite(gam)), f"{label}: {int(np.sum(~np.isfinite(gam)))} non-finite entries"
    spans = np.concatenate([[1.0], obs[:, 0].astype(float)])
    d = np.abs(gam - ref)
    c0 = float(d[:, 0].max() / max(np.abs(ref[:, 0]).max(), 1e-300))
    assert c0 <= GAMMA_TOL, (label, c0)
    scale = d[:, 1:].max(axis=0) / spans[1:]
    sums = np.abs(gam[:, 1:].sum(axis=0) - spans[1:]) / spans[1:]
    large = ref[:, 1:] >= 1e-3 * spans[1:]
    rel = np.where(large, d[:, 1:] / np.where(large, ref[:, 1:], 1.0), 0.0)
    worst = {"scale": float(scale.max(initial=0.0)), "sum": float(sums.max(initial=0.0)), "large": float(rel.max(initial=0.0)),
             "col0": c0}
    print(f"{label}: {ncol - 1} rows, worst column of its span {worst['scale']:.2e}, column sum vs span {worst['sum']:.2e}, "
          f"large entries rel {worst['large']:.2e}, column 0 {c0:.2e}")
    bad = np.nonzero(scale > GAMMA_TOL)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} columns off by more than {GAMMA_TOL} of their span, e.g. rows {bad[:8] + 1} " \
                          f"(spans {spans[1:][bad[:8]]}, errors {scale[bad[:8]]})"
    bad = np.nonzero(sums > GAMMA_SUM_RTOL)[0]
    assert len(bad) == 0, f"{label}: {len(bad)} columns do not sum to their span, e.g. rows {bad[:8] + 1} (spans {spans[1:][bad[:8]]}, " \
                          f"sums {gam[:, 1:].sum(axis=0)[bad[:8]]})"
    assert worst["large"] <= GAMMA_LARGE_TOL, (label, worst["large"])
    arg = gam.argmax(axis=0)
    if M > 1:
        top2 = np.sort(ref, axis=0)[-2:]
        strong = (top2[1] - top2[0]) > GAMMA_MARGIN * np.concatenate([[max(np.abs(ref[:, 0]).max(), 1e-300)], spans[1:]])
        mism = np.nonzero(strong & (arg != ref.argmax(axis=0)))[0]
        assert len(mism) == 0, f"{label}: decoded index differs on columns {mism[:10]}"
    if arg_dev is not None:
        arg_dev = np.asarray(arg_dev)
        assert arg_dev.shape == arg.shape and np.array_equal(arg_dev, arg), \
            f"{label}: device decode differs from argmax of its own gamma on columns {np.nonzero(arg_dev != arg)[0][:10]}"
    return worst


def check_against(g, im, save_gamma):
    ll = im.loglik()
    assert abs(ll - float(g["loglik"])) <= LL_TOL * abs(float(g["loglik"])), (ll, float(g["loglik"]))
    xs = im.xisums[0]
    assert rel_err(xs, g["xisum"]) <= STAT_TOL
    gs = im.gamma_sums[0]
    ref_keys = [tuple(int(x) for x in k) for k in g["gs_keys"]]
    assert sorted(gs.keys()) == sorted(ref_keys)
    for k, v in zip(ref_keys, g["gs_vals"]):
        scale = max(np.abs(v).max(), 1e-300)
        assert np.max(np.abs(gs[k] - v)) <= STAT_TOL * scale, k
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"]) <= STAT_TOL * np.maximum(np.abs(g["q"]), 1e-12)), (q, g["q"])
    gam = im.gammas[0]
    if not save_gamma:
        assert gam.shape == (len(g["pi"]), 1)
        assert rel_err(gam[:, 0], g["gamma0"]) <= STAT_TOL
        return
    L = len(g["obs"])
    assert gam.shape == (len(g["pi"]), L + 1)
    st = int(g["gamma_stride"])
    sub = gam[:, ::st]
    assert np.max(np.abs(sub - g["gamma_sub"])) <= 2e-5 * max(1.0, float(np.abs(g["gamma_sub"]).max()))
    # the compiled reference's strided columns, each at the scale of its own row's span (column 0: of its largest entry)
    sub_spans = np.concatenate([[max(float(np.abs(g["gamma_sub"][:, 0]).max()), 1e-300)], g["obs"][:, 0].astype(float)])[::st]
    sub_err = np.max(np.abs(sub - g["gamma_sub"]), axis=0) / sub_spans
    assert sub_err.max() <= GAMMA_TOL, f"strided columns {np.nonzero(sub_err > GAMMA_TOL)[0][:10] * st} off their span's scale"
    # every column against the C restatement run on the golden's own parameters
    o = oracle_estep(g["pi"], g["T"], g["keys"], g["E"], g["obs"])
    check_gamma_columns(gam, o["gamma"], g["obs"], arg_dev=im.gamma_argmax(0), label=str(g.get("name", "golden")))
    arg = gam.argmax(axis=0)
    strong = g["gamma_margin"] > 1e-5
    mism = np.nonzero(arg != g["gamma_argmax"])[0]
    assert not np.any(strong[mism]), f"posterior argmax differs on columns {mism[strong[mism]][:10]}"
    # north_star: "bit-exact posterior indices".  On every golden the decoded index is identical on EVERY column, also those
    # whose top-1 / top-2 margin is below 1e-5 (the rule above is what SURVEY.md 8(c) can promise in general; this is what holds)
    assert len(mism) == 0, f"posterior argmax differs on {len(mism)} low-margin columns {mism[:10]} (margins {g['gamma_margin'][mism][:10]})"
    arg_dev = im.gamma_argmax(0)
    assert np.array_equal(arg_dev, arg.astype(np.int32))


@pytest.fixture(params=["default", "dense", "lock"])
def chain_family(request, engine_opt):
    """Every golden vector is checked with the chain kernels the engine picks by itself (the scans over the semiseparable
    structure of T when the spans are short, else cooperative / streamed operands), with the scans switched off (the dense
    kernels every manager falls back to) and with the lock-step kernels on the matrix cores forced (M <= 64)."""
    if request.param == "lock":
        engine_opt("SMCPP_CHAIN", "lock")
    if request.param == "dense":
        engine_opt("SMCPP_SS", "0")
    return request.param


def test_golden_stats(golden, chain_family):
    im = make_im(golden)
    if chain_family == "lock" and len(golden["pi"]) <= 64:
        assert im.chain_mode() == 4
    if chain_family == "default" and int(np.max(golden["obs"][:, 0])) <= 512:
        assert im.chain_mode() == 5
    if chain_family == "dense":
        assert im.chain_mode() != 5
    im.E_step()
    check_against(golden, im, save_gamma=False)


def test_golden_posterior(golden, chain_family):
    im = make_im(golden)
    im.save_gamma = True
    im.E_step()
    check_against(golden, im, save_gamma=True)


def test_per_row_gamma_from_scan_steps_vs_eigensystems(engine_opt):
    """Round 6: with save_gamma the engine keeps its eigen-free path on binned data - the per-row posterior of a span > 1 row is the sum
    over its positions of forward x backward scan vectors (`k_gamma_rows_scan`, 2 span - 1 O(M) steps) instead of the reference's
    eigensystem formula (hmm.cpp:113-121: `k_gamma_rows_b` / `k_gamma_rows_eig`, 2 M^3 flop; SMCPP_GAMMA_SCAN=0).  Both against the
    compiled reference's goldens (every check of `check_against`, the decoded index on EVERY column) and against each other."""
    res = {}
    for scan in ("0", "1"):
        engine_opt("SMCPP_GAMMA_SCAN", scan)
        for name in ("G4_M64_n20_2Mbp", "G3_M32_n10_2Mbp", "G1_M16_n4", "G5_M48_twopop_layout"):
            g = load_golden(name)
            im = make_im(g)
            im.save_gamma = True
            im.E_step()
            plan = im.describe()["plan"]
            # (G1 holds spans up to 199: beyond the eigen-free statistics' 64, it keeps the eigensystems in either setting)
            eigen_free = scan == "1" and int(g["obs"][:, 0].max()) <= 64
            assert plan["per_row_gamma"] == ("scan steps" if eigen_free else "eigensystem"), (name, plan)
            check_against(g, im, save_gamma=True)
            res[(scan, name)] = im.gammas[0]
    for (scan, name), gam in res.items():
        if scan == "1":
            d = np.max(np.abs(gam - res[("0", name)]))
            print(f"{name}: per-row gamma, scan steps vs eigensystems: max abs difference {d:.2e}")
            assert d <= 2e-6


@pytest.mark.parametrize("rows_per_chunk", [37, 100, 1000000])
def test_chunking_invariance(rows_per_chunk):
    """The chunk-parallel chains must reproduce the single-chunk (purely sequential) run."""
    g = load_golden("G4_M64_n20_2Mbp")
    im = make_im(g)
    im.set_chunking(rows_per_chunk)
    im.E_step()
    check_against(g, im, save_gamma=False)
    t = im.last_timing()
    if rows_per_chunk >= 1000000:
        assert t["fwd_passes"] == 1 and t["bwd_passes"] == 1


def test_vs_oracle_random_small():
    """Seeded random inputs at a size the C restatement finishes in a second, several contigs of ragged length."""
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    g = load_golden("G3_M32_n10_2Mbp")
    contigs = [synth.synth_contig(10 + i, L, 10) for i, L in enumerate([300_000, 100, 70_000, 1_000_000])]
    contigs[1] = contigs[1][:1]                      # a one-row contig
    im = _smcpp.PyOnePopInferenceManager(10, contigs, g["hs"], ("pop1",), 0.5)
    im.theta = float(g["theta"]); im.rho = float(g["rho"])
    im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
    im.E_step()
    lls = im.logliks()
    xs = im.xisums
    gss = im.gamma_sums
    qtot = np.zeros(4)
    for c, ob in enumerate(contigs):
        o = oracle.estep(g["pi"], g["T"], g["keys"], g["E"], ob)
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"])
        assert rel_err(xs[c], o["xisum"]) <= STAT_TOL
        assert sorted(gss[c].keys()) == sorted(o["gamma_sums"].keys())
        for k, v in o["gamma_sums"].items():
            assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300)
        qtot += o["q"]
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - qtot) <= STAT_TOL * np.abs(qtot))


def test_errors():
    from smcpp_amd import _smcpp
    g = load_golden("G1_M16_n4")
    with pytest.raises(RuntimeError, match="empty"):
        _smcpp.PyOnePopInferenceManager(4, [], g["hs"], ("p",), 0.5)
    with pytest.raises(RuntimeError, match="ascending"):
        _smcpp.PyOnePopInferenceManager(4, [g["obs"]], g["hs"][::-1].copy(), ("p",), 0.5)
    bad = g["obs"].copy(); bad[5, 0] = 0
    with pytest.raises(RuntimeError, match="span <= 0"):
        _smcpp.PyOnePopInferenceManager(4, [bad], g["hs"], ("p",), 0.5)
    im = _smcpp.PyOnePopInferenceManager(4, [g["obs"]], g["hs"], ("p",), 0.5)
    with pytest.raises(RuntimeError):
        im.E_step()                                   # no parameters yet
    with pytest.raises(RuntimeError, match="same size"):
        im.hidden_states = [0.0, 1.0]


def test_pack_stats_matches_python_layout():
    """smcpp_pack_stats (the buffer that is all-reduced over RCCL) equals smcpp_amd.dist.pack_host on the getters."""
    from smcpp_amd import _smcpp, dist as sd, synth
    g = load_golden("G3_M32_n10_2Mbp")
    contigs = [synth.synth_contig(30 + i, L, 10) for i, L in enumerate([120_000, 50_000])]
    im = _smcpp.PyOnePopInferenceManager(10, contigs, g["hs"], ("pop1",), 0.5)
    im.theta = float(g["theta"]); im.rho = float(g["rho"])
    im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
    im.E_step()
    gkeys = np.array(sorted(set(tuple(int(x) for x in k) for k in im.keys) | {(2, 9, 10)}), dtype=np.int32)
    im.set_global_keys(gkeys)
    buf = im.pack_stats()
    py = sd.pack_host(list(im.logliks()), [x[:, 0] for x in im.gammas], im.xisums, im.gamma_sums, gkeys)
    np.testing.assert_allclose(buf, py, rtol=1e-14, atol=0)
    # device path (what bench.py hands to RCCL): one kernel writes the same layout into a caller-owned device tensor
    import torch
    tbuf = torch.full((im.stats_len(),), -1.0, dtype=torch.float64, device="cuda")
    im.pack_stats_device(tbuf.data_ptr())
    np.testing.assert_allclose(tbuf.cpu().numpy(), buf, rtol=1e-14, atol=0)
    q_before = np.array(im.Q(separate=True))
    im.unpack_stats_device(tbuf.data_ptr(), tbuf.numel())      # "reduced" over a world of one, from the device buffer
    np.testing.assert_allclose(np.array(im.Q(separate=True)), q_before, rtol=1e-12)
    q_local = np.array(im.Q(separate=True))
    im.unpack_stats(buf)                       # "reduced" over a world of one
    q_red = np.array(im.Q(separate=True))
    np.testing.assert_allclose(q_red, q_local, rtol=1e-12)


@pytest.mark.parametrize("name", ["G1_M16_n4", "G4_M64_n20_2Mbp", "G7_M32_n8_chr11"])
def test_model_parameter_path(name):
    """The reference's own entry: im.model = model; im.theta/rho/alpha; E_step().  pi, T and the emission table are
    prepared on the host by the engine (rows A6-A10) instead of being handed in with set_raw."""
    from smcpp_amd import _smcpp
    from smcpp_amd.model import PiecewiseModel
    g = load_golden(name)
    im = _smcpp.PyOnePopInferenceManager(int(g["n"]), [np.ascontiguousarray(g["obs"])], g["hs"], ("pop1",),
                                         float(g["pol"]))
    m = PiecewiseModel(g["a"], g["s"], 1e4, "pop1")
    im.model = m
    im.theta = float(g["theta"]); im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
    im.E_step()
    check_against(g, im, save_gamma=False)
    np.testing.assert_allclose(im.pi, g["pi"], rtol=1e-13)
    np.testing.assert_allclose(im.transition, g["T"], rtol=1e-11, atol=1e-17)
    ll0 = im.loglik()
    m[1] = m[1] * 1.5                      # Observable -> "model update" -> set_params -> dirty
    im.E_step()
    assert abs(im.loglik() - ll0) > 1e-6 * abs(ll0)
    m[1] = g["a"][1]
    im.E_step()
    assert abs(im.loglik() - ll0) <= 1e-12 * abs(ll0)


def test_q_gradient_matches_finite_differences():
    """dQ/da_k by forward-mode duals through the host preparation equals central finite
    differences of Q (statistics of the E-step held fixed), the check the reference's own test_inference.py:61-74 prints."""
    from smcpp_amd import _smcpp
    from smcpp_amd.model import PiecewiseModel
    g = load_golden("G1_M16_n4")
    im = _smcpp.PyOnePopInferenceManager(int(g["n"]), [np.ascontiguousarray(g["obs"])], g["hs"], ("pop1",),
                                         float(g["pol"]))
    m = PiecewiseModel(g["a"], g["s"], 1e4, "pop1")
    m.differentiable = True
    im.model = m
    im.theta = float(g["theta"]); im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
    im.E_step()
    q, jac = im.Q_with_gradient()
    np.testing.assert_allclose(q, g["q"], rtol=5e-6)
    assert jac.shape == (4, len(g["a"]))
    a0 = np.array(g["a"], dtype=float)
    for k in range(len(a0)):
        h = 1e-4 * a0[k]
        m[k] = a0[k] + h; qp = np.array(im.Q(separate=True))
        m[k] = a0[k] - h; qm = np.array(im.Q(separate=True))
        m[k] = a0[k]
        fd = (qp - qm) / (2 * h)
        assert np.all(np.abs(fd - jac[:, k]) <= 1e-4 * np.abs(jac[:, k]) + 1e-5), (k, fd, jac[:, k])


def test_posterior_product_on_reference_test_contig():
    """`smc++ posterior` on the reference's own un-binned test contig (test/bugs/11/chr11_5subjs.smc.gz, fixture G7):
    the decoded path must equal the reference's argmax on every column with a relative top-1/top-2 margin > 1e-5."""
    from smcpp_amd.model import PiecewiseModel
    from smcpp_amd.posterior import posterior
    g = load_golden("G7_M32_n8_chr11")
    m = PiecewiseModel(g["a"], g["s"], 1e4, "pop1")
    hs, gammas, sites, paths = posterior(m, [g["obs"][1:]], 32, int(g["n"]), float(g["theta"]), float(g["rho"]),
                                         float(g["alpha"]), float(g["pol"]), hidden_states=g["hs"])
    L = len(g["obs"])
    assert gammas[0].shape == (32, L + 1) and paths[0].shape == (L + 1,)
    np.testing.assert_allclose(gammas[0].sum(axis=0), 1.0, rtol=1e-12)
    assert np.array_equal(sites[0], g["obs"][:, 0])          # `<file>_sites` = the span column, as smc++ posterior stores it
    strong = g["gamma_margin"] > 1e-5
    mism = np.nonzero(paths[0] != g["gamma_argmax"])[0]
    assert not np.any(strong[mism])
    assert np.array_equal(paths[0], gammas[0].argmax(axis=0))


def test_posterior_product_two_populations():
    """`smc++ posterior` with two populations (commands/posterior.py:88-100): 7-column rows, PyTwoPopInferenceManager, hidden
    states balanced on the distinguished model; the decoded matrix against the C restatement of hmm.cpp run on the SAME prepared
    parameters (pi, T, joint-CSFS emission table as the engine formed them) - every column with a clear winner decodes equally."""
    from oracle import oracle
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    from smcpp_amd.posterior import posterior
    a, s = synth.model_pieces(8)
    model = TwoPopulationModel(PiecewiseModel(a, s, 1e4, pid="pop1"),
                               PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(4)), s[:4], 1e4, pid="pop2"), 0.4)
    raw = synth.synth_contig_twopop(3, 3_000_000, 4, 3)
    hs, gammas, sites, paths, im = posterior(model, [raw], 12, (4, 3), synth.THETA, synth.RHO, a=(2, 0), return_manager=True)
    assert len(hs) == 13 and hs[0] == 0 and np.isinf(hs[-1])
    obs = np.vstack([[1, -1, 0, 0, -1, 0, 0], raw]).astype(np.int32)
    assert gammas[0].shape == (12, len(obs) + 1) and np.array_equal(sites[0], obs[:, 0])
    np.testing.assert_allclose(gammas[0].sum(axis=0), 1.0, rtol=1e-12)
    keys = im.keys
    ep = im.emission_probs
    o = oracle.estep(im.pi, im.transition, keys, np.array([ep[tuple(k)] for k in keys.tolist()]), obs, save_gamma=True)
    g = o["gamma"] / o["gamma"].sum(axis=0, keepdims=True)
    assert np.max(np.abs(gammas[0] - g)) <= 2e-5
    srt = np.sort(g, axis=0)
    strong = (srt[-1] - srt[-2]) / srt[-1] > 1e-5
    assert np.all((paths[0] == g.argmax(axis=0)) | ~strong)
    assert abs(im.loglik() - o["loglik"]) <= 1e-6 * abs(o["loglik"])
    # a window and thinning (posterior.py:76-87) go through the same path
    hs2, g2, s2, p2 = posterior(model, [raw], 12, (4, 3), synth.THETA, synth.RHO, a=(2, 0), start=100_000, end=900_000, thinning=5,
                                hidden_states=hs)
    assert s2[0].sum() <= 800_001 + raw[:, 0].max() and g2[0].shape[1] == len(s2[0]) + 1


def test_em_iterations_increase_the_likelihood():
    """End-to-end property of E-step statistics + Q + gradients: an EM step cannot decrease the log-likelihood
    (up to the float-alpha noise of the E-step).  Data are simulated under a size history that differs from the start."""
    from smcpp_amd import synth
    from smcpp_amd.analysis import em
    g = load_golden("G1_M16_n4")
    contigs = [synth.synth_contig(40 + i, 400_000, 4) for i in range(2)]
    a0 = np.ones(4)
    model, ll = em(contigs, 4, g["hs"], a0, g["s"], float(g["theta"]), float(g["rho"]), iterations=3)
    assert len(ll) == 4
    assert np.all(np.diff(ll) >= -1e-6 * np.abs(ll[:-1])), ll
    assert ll[-1] > ll[0] + 1e-3
    assert np.all(model.a > 0)


@pytest.mark.parametrize("a1,a2,M,split", [(2, 0, 24, 0.3), (1, 1, 24, 0.005), (1, 1, 1, 0.3)])
def test_two_population_model_path(a1, a2, M, split):
    """`PyTwoPopInferenceManager` driven the reference's way (im.model = two-population model; SURVEY.md config C4
    shape): the engine prepares pi / T from the distinguished model and the emission table from its JointCSFS; the
    E-step on those parameters must equal the C restatement of hmm.cpp fed with the same parameters (6-int keys)."""
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    n1, n2 = 6, 5
    a, s = synth.model_pieces()
    m1 = PiecewiseModel(a, s, 1e4, pid="pop1")
    m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(8)), s[:8], 1e4, pid="pop2")
    contigs = []
    for ci, L in enumerate([400_000, 150_000]):
        obs = synth.synth_contig_twopop(3 + ci, L, n1, n2).copy()
        if a1 == 1:                               # one distinguished lineage per population: a2 in {0, 1}, missing together
            nm = obs[:, 1] >= 0
            obs[nm, 4] = (obs[nm, 2] + obs[nm, 6] + obs[nm, 0]) % 2
            obs[~nm, 4] = -1
        contigs.append(np.ascontiguousarray(obs, dtype=np.int32))
    hs = synth.hidden_states(M)
    im = _smcpp.PyTwoPopInferenceManager(n1, n2, a1, a2, contigs, hs, ("pop1", "pop2"), 0.5)
    tm = TwoPopulationModel(m1, m2, split)
    im.model = tm
    im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
    im.E_step()
    pi, T = im.pi, im.transition
    keys = im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    assert np.all(np.isfinite(T)) and np.all(Etab > 0) and np.all(Etab <= 1)
    lls = im.logliks()
    xs, gss = im.xisums, im.gamma_sums
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob)
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"])
        assert rel_err(xs[c], o["xisum"]) <= STAT_TOL
        for k, v in o["gamma_sums"].items():
            assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300)
    # the split is a parameter: moving it changes the likelihood, moving it back restores it bit for bit
    ll0 = im.loglik()
    tm.split = split * 1.5
    im.E_step()
    assert abs(im.loglik() - ll0) > 1e-9 * abs(ll0)
    tm.split = split
    im.E_step()
    assert abs(im.loglik() - ll0) <= 1e-12 * abs(ll0)


@pytest.mark.parametrize("M,n,length,chunk", [(64, 12, 400_000, -1),         # chunk = -1: emission / power tables from global memory
                                               (48, 9, 300_000, -1),         # (the path taken when they do not fit the LDS)
                                               (2, 3, 400_000, 0), (3, 5, 300_000, 50), (15, 4, 300_000, 0),
                                               (17, 6, 300_000, 40), (33, 8, 300_000, 0), (47, 9, 250_000, 64),
                                               (65, 10, 200_000, 0), (100, 12, 150_000, 64), (130, 6, 120_000, 0),
                                               (200, 8, 80_000, 48), (256, 10, 60_000, 0)])
def test_state_count_sweep_vs_oracle(engine_opt, M, n, length, chunk):
    """Every kernel family (cooperative M <= 64 at each padded width, generic 64 < M <= 256, odd widths that need
    padding) against the C restatement, parameters from the engine's own preparation, several ragged contigs, with and
    without forced multi-chunk iteration; posterior rows included."""
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contigs = [synth.synth_contig(100 + M + i, L, n) for i, L in enumerate([length, length // 3, 20_000])]
    im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
    im.model = PiecewiseModel(a, s, 1e4, "pop1")
    im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
    import os
    if chunk > 0:
        im.set_chunking(chunk)
    if chunk < 0:
        engine_opt("SMCPP_COOP_TAB", "0")
    im.save_gamma = True
    try:
        im.E_step()
    finally:
        engine_opt("SMCPP_COOP_TAB", None)
    pi, T, keys = im.pi, im.transition, im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    lls, xs, gss, gams = im.logliks(), im.xisums, im.gamma_sums, im.gammas
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob, save_gamma=True)
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"])
        assert rel_err(xs[c], o["xisum"]) <= STAT_TOL
        for k, v in o["gamma_sums"].items():
            assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300)
        g_ref = o["gamma"]
        assert gams[c].shape == g_ref.shape
        assert np.max(np.abs(gams[c] - g_ref)) <= 2e-5 * max(1.0, float(np.abs(g_ref).max()))
        check_gamma_columns(gams[c], g_ref, ob, arg_dev=im.gamma_argmax(c), label=f"M = {M}, contig {c}")
        if M > 1:
            top2 = np.sort(g_ref, axis=0)[-2:]
            margin = (top2[1] - top2[0]) / np.maximum(top2[1], 1e-300)
            mism = np.nonzero(gams[c].argmax(axis=0) != g_ref.argmax(axis=0))[0]
            assert not np.any(margin[mism] > 1e-5)


@pytest.mark.parametrize("M,n", [(64, 20), (32, 10), (48, 7), (16, 4), (130, 6), (256, 8)])
def test_eigen_free_prepass_on_and_off_vs_oracle(engine_opt, M, n):
    """The two ways the cooperative chains run on binned data (spans < 32): eigensystem kernels only
    (SMCPP_POWER_PREPASS=0) and eigen-free pre-pass + a full eigensystem pass (the default; cooperative kernels for
    M <= 64, streamed-operand kernels with device-built powers above).  Each against the C restatement at the stated tolerances, and against each other far below them (every stored row comes from the
    eigensystem kernels either way; the pre-pass only changes the start vectors of the chunks)."""
    import os
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contigs = [synth.synth_contig(300 + M, 3_000_000 if M <= 64 else 1_200_000, n), synth.synth_contig(301 + M, 150_000, n)]
    res = {}
    for mode in (0, 1):
        engine_opt("SMCPP_POWER_PREPASS", str(mode))
        try:
            im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
            im.model = PiecewiseModel(a, s, 1e4, "pop1")
            im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
            for _ in range(2):            # the second E-step pre-queues as many passes as the first one needed
                im.E_step()
            res[mode] = (np.array(im.logliks()), im.xisums, im.gamma_sums, np.array(im.Q(separate=True)))
        finally:
            engine_opt("SMCPP_POWER_PREPASS", None)
    pi, T, keys = im.pi, im.transition, im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob)
        for mode, (lls, xs, gss, q) in res.items():
            assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"]), mode
            assert rel_err(xs[c], o["xisum"]) <= STAT_TOL, mode
            for k, v in o["gamma_sums"].items():
                assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), (mode, k)
    for mode in (1,):
        assert np.all(np.abs(res[mode][0] - res[0][0]) <= 1e-8 * np.abs(res[0][0])), mode
        assert np.all(np.abs(res[mode][3] - res[0][3]) <= 1e-6 * np.maximum(np.abs(res[0][3]), 1e-12)), mode


@pytest.mark.parametrize("M,n,max_span", [(64, 20, 4000), (32, 6, 700), (48, 9, 100), (130, 5, 3000), (256, 6, 500)])
def test_eigen_free_prepass_with_long_spans_vs_oracle(engine_opt, M, n, max_span):
    """Spans of 32 .. 4095 positions: the pre-pass applies rescaled powers A^32 .. A^2048 from L2 on the rows that need them;
    every stored row still comes from the eigensystem kernels.  Pre-pass on / off against the C restatement."""
    import os
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    rng = np.random.RandomState(M + n)
    contigs = []
    for ci, L in enumerate([2_000_000 if M <= 64 else 900_000, 200_000]):
        c = synth.synth_contig(500 + M + ci, L, n).copy()
        long_rows = np.nonzero(c[:, 0] > 1)[0]
        pick = rng.choice(long_rows, size=len(long_rows) // 12, replace=False)
        c[pick, 0] = rng.randint(32, max_span + 1, size=len(pick))         # a twelfth of the runs becomes long
        c[pick[0], 0] = max_span
        contigs.append(np.ascontiguousarray(c))
    res = {}
    for mode in (0, 1):
        engine_opt("SMCPP_POWER_PREPASS", str(mode))
        try:
            im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
            im.model = PiecewiseModel(a, s, 1e4, "pop1")
            im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
            im.E_step(); im.E_step()
            res[mode] = (np.array(im.logliks()), im.xisums, im.gamma_sums)
        finally:
            engine_opt("SMCPP_POWER_PREPASS", None)
    pi, T, keys = im.pi, im.transition, im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob)
        for mode, (lls, xs, gss) in res.items():
            assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"]), mode
            assert rel_err(xs[c], o["xisum"]) <= STAT_TOL, mode
            for k, v in o["gamma_sums"].items():
                assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), (mode, k)
    assert np.all(np.abs(res[1][0] - res[0][0]) <= 1e-8 * np.abs(res[0][0]))


@pytest.mark.parametrize("M,n,chunk", [(64, 20, 0), (64, 12, 37), (50, 6, 150), (64, 8, 400), (32, 10, 0), (33, 5, 90), (16, 4, 60),
                                       (7, 3, 0)])
def test_lock_step_chains_vs_oracle(engine_opt, M, n, chunk):
    """The lock-step chains (16 chunks per workgroup on the matrix cores, chains_lock.hpp) forced on small inputs: ragged
    contigs (so the 16 columns of a workgroup have different lengths and some do not exist), chunks far shorter than the
    chains' memory (many passes, per-column merge exits and skip tests), three eigen keys (one register-resident), against the
    C restatement and against the cooperative kernels."""
    import os
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contigs = [synth.synth_contig(700 + M + i, L, n) for i, L in enumerate([1_500_000, 40_000, 600_000, 900, 250_000])]
    res = {}
    for mode in ("coop", "lock"):
        engine_opt("SMCPP_CHAIN", mode)
        try:
            im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
            im.model = PiecewiseModel(a, s, 1e4, "pop1")
            im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
            if chunk > 0:
                im.set_chunking(chunk)
            im.save_gamma = True
            im.E_step(); im.E_step()
            res[mode] = (np.array(im.logliks()), im.xisums, im.gamma_sums, im.gammas)
        finally:
            engine_opt("SMCPP_CHAIN", None)
    pi, T, keys = im.pi, im.transition, im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob, save_gamma=True)
        for mode, (lls, xs, gss, gams) in res.items():
            assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"]), mode
            assert rel_err(xs[c], o["xisum"]) <= STAT_TOL, mode
            for k, v in o["gamma_sums"].items():
                assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), (mode, k)
            g_ref = o["gamma"]
            assert np.max(np.abs(gams[c] - g_ref)) <= 2e-5 * max(1.0, float(np.abs(g_ref).max())), mode
            top2 = np.sort(g_ref, axis=0)[-2:]
            margin = (top2[1] - top2[0]) / np.maximum(top2[1], 1e-300)
            mism = np.nonzero(gams[c].argmax(axis=0) != g_ref.argmax(axis=0))[0]
            assert not np.any(margin[mism] > 1e-5), mode
    # (the span-1 product is rounded differently - fp64 MFMA then float vs float FMAs - so the two agree at float noise level)
    assert np.all(np.abs(res["lock"][0] - res["coop"][0]) <= 2 * LL_TOL * np.abs(res["coop"][0]))


def test_many_tiny_contigs():
    """300 contigs of 1-40 rows each (ragged, most shorter than any chunk): per-contig results against the oracle."""
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    g = load_golden("G3_M32_n10_2Mbp")
    rng = np.random.default_rng(7)
    big = synth.synth_contig(77, 3_000_000, 10)
    contigs = []
    pos = 0
    for _ in range(300):
        L = int(rng.integers(1, 41))
        contigs.append(np.ascontiguousarray(big[pos:pos + L]))
        pos += L
    im = _smcpp.PyOnePopInferenceManager(10, contigs, g["hs"], ("pop1",), 0.5)
    im.theta = float(g["theta"]); im.rho = float(g["rho"])
    im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
    im.E_step()
    lls, xs, gss = im.logliks(), im.xisums, im.gamma_sums
    tot = 0.0
    for c in range(0, 300, 7):
        o = oracle.estep(g["pi"], g["T"], g["keys"], g["E"], contigs[c])
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * max(1.0, abs(o["loglik"]))
        assert rel_err(xs[c], o["xisum"]) <= STAT_TOL
        assert sorted(gss[c].keys()) == sorted(o["gamma_sums"].keys())
    assert np.isfinite(im.loglik())


@pytest.mark.parametrize("rows_per_chunk", [300, 800, 1200])
def test_warm_start_matches_cold_start(rows_per_chunk):
    """Opt-in extension: an E-step that starts its chunk-parallel chains from the previous E-step's boundary vectors
    must give what a cold manager gives on the same (perturbed) parameters, in fewer / shorter passes.
    300 rows per chunk: several light passes; 800 (3 400 positions): one forward light pass cold, so the warm start's first
    launched forward pass is the FULL pass; 1200 (5 100 positions): no forward light pass at all (a full pass
    must never take the idle exit on the never-written flag of the pass before it)."""
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    g = load_golden("G4_M64_n20_2Mbp")
    obs = synth.synth_contig(0, 30_000_000, 20)
    a0 = np.array(g["a"], dtype=float)

    def manager(warm):
        im = _smcpp.PyOnePopInferenceManager(20, [obs], g["hs"], ("pop1",), float(g["pol"]))
        im.theta = float(g["theta"]); im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
        im.set_chunking(rows_per_chunk)            # many chunks so that the iteration matters at this size
        if warm:
            im.set_warm_start(True)
        return im

    warm, cold = manager(True), manager(False)
    mw, mc = PiecewiseModel(a0, g["s"], 1e4, "pop1"), PiecewiseModel(a0, g["s"], 1e4, "pop1")
    warm.model = mw; cold.model = mc
    warm.E_step(); cold.E_step()
    assert abs(warm.loglik() - cold.loglik()) <= 1e-12 * abs(cold.loglik())       # first call: nothing to reuse
    rng = np.random.default_rng(3)
    for it in range(3):
        a1 = a0 * (1.0 + 0.02 * rng.standard_normal(len(a0)) / (it + 1))
        mw[:] = a1; mc[:] = a1
        warm.E_step(); cold.E_step()
        lw, lc = warm.loglik(), cold.loglik()
        assert abs(lw - lc) <= 1e-8 * abs(lc)
        assert rel_err(warm.xisums[0], cold.xisums[0]) <= STAT_TOL
        gw, gc = warm.gamma_sums[0], cold.gamma_sums[0]
        for k, v in gc.items():
            assert np.max(np.abs(gw[k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300)
        tw, tc = warm.last_timing(), cold.last_timing()
        if rows_per_chunk == 300:
            assert tw["fwd_passes"] <= tc["fwd_passes"] and tw["bwd_passes"] <= tc["bwd_passes"]
    # a JUMP in parameter space: the stale boundary vectors are then no better than pi, the iteration has to absorb it
    a2 = a0[::-1] * 2.5
    mw[:] = a2; mc[:] = a2
    warm.E_step(); cold.E_step()
    assert abs(warm.loglik() - cold.loglik()) <= 1e-8 * abs(cold.loglik())
    assert rel_err(warm.xisums[0], cold.xisums[0]) <= STAT_TOL


@pytest.mark.parametrize("name", ["G1_M16_n4", "G3_M32_n10_2Mbp", "G4_M64_n20_2Mbp", "G7_M32_n8_chr11"])
def test_q_gradient_matches_reference_autodiff(name):
    """SURVEY.md §8(f) row f-1, golden G10: dQ/da_k from the engine (duals through the host preparation, linear in the
    GPU E-step statistics) against the gradients the reference's own AD gives on the same contig."""
    from smcpp_amd import _smcpp
    from smcpp_amd.model import PiecewiseModel
    import os
    g = load_golden(name)
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G10_q_gradients.npz"))
    im = _smcpp.PyOnePopInferenceManager(int(g["n"]), [np.ascontiguousarray(g["obs"])], g["hs"], ("pop1",),
                                         float(g["pol"]))
    m = PiecewiseModel(g["a"], g["s"], 1e4, "pop1")
    m.differentiable = True
    im.model = m
    im.theta = float(g["theta"]); im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
    im.E_step()
    q, jac = im.Q_with_gradient()
    qr, jr = G[name + "_q"], G[name + "_jac"]
    assert np.all(np.abs(q - qr) <= STAT_TOL * np.maximum(np.abs(qr), 1e-12))
    # every row of the Jacobian is linear in one family of statistics: same relative tolerance against its largest entry
    for r in range(4):
        scale = max(np.abs(jr[r]).max(), 1e-300)
        assert np.max(np.abs(jac[r] - jr[r])) <= 2 * STAT_TOL * scale, (r, jac[r], jr[r])


def test_config_c1_reference_example_end_to_end():
    """Config C1 (BASELINE.json configs[0]): the reference's example VCF -> rows (smcpp_amd.vcf2smc) -> the E-step on the
    un-binned contig with the missing row `estimate` prepends, and on the thinned / binned / compressed contig the main
    EM loop sees; GPU against the C restatement on the same rows, parameters from the engine's own preparation."""
    import os
    from oracle import oracle
    from smcpp_amd import _smcpp, data as D, synth, vcf2smc as V
    from smcpp_amd.model import PiecewiseModel
    vcf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example.vcf.gz")
    c, _ = V.vcf2smc(vcf, "1", ("pop1", ["msp_0", "msp_1", "msp_2"]))
    n = c.n[0]
    raw = np.ascontiguousarray(np.vstack([[1, -1, 0, 0], c.data]), dtype=np.int32)
    assert raw.shape == (1850, 4)                                  # what the reference's bootstrap sees
    piece = D.break_long_spans(D.Contig(D.compress_repeated_obs(c.data), c.pid, c.n, c.a), 100000)[0]
    binned = D.recode_monomorphic(D.Contig(D.bin_observations(D.thin_data(piece.data, 895), 100, [2]), c.pid, c.n, c.a))
    thin = np.ascontiguousarray(D.compress_repeated_obs(binned.data), dtype=np.int32)
    assert thin.shape == (2727, 4)                                 # what the reference's main EM loop sees
    a, s = synth.model_pieces()
    for rows, M in ((raw, 1), (raw, 16), (thin, 15)):
        hs = synth.hidden_states(M)
        im = _smcpp.PyOnePopInferenceManager(n, [rows], hs, ("pop1",), 0.5)
        im.model = PiecewiseModel(a, s, 1e4, "pop1")
        # mutation rate per row unit from Watterson's estimator of this contig (4.02e-4 per bp; bins of 100 bp)
        im.theta = 4.02e-4 if rows is raw else 4.02e-2; im.rho = 1e-4 if rows is raw else 1e-2; im.alpha = 1.0
        im.E_step()
        ep = im.emission_probs
        Etab = np.array([ep[tuple(k)] for k in im.keys.tolist()])
        o = oracle.estep(im.pi, im.transition, im.keys, Etab, rows)
        assert abs(im.loglik() - o["loglik"]) <= LL_TOL * abs(o["loglik"])
        assert rel_err(im.xisums[0], o["xisum"]) <= STAT_TOL
        for k, v in o["gamma_sums"].items():
            assert np.max(np.abs(im.gamma_sums[0][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300)
        q = np.array(im.Q(separate=True))
        assert np.all(np.abs(q - o["q"]) <= STAT_TOL * np.maximum(np.abs(o["q"]), 1e-12))


def test_em_on_the_reference_example_pipeline():
    """VCF -> rows -> the reference's shaping pipeline -> balanced hidden states -> three EM iterations on the GPU
    (the whole C1 flow of SURVEY.md §8d, with this repository's callers of the path): the log-likelihood must rise."""
    import os
    from smcpp_amd import data as D, posterior as PO, vcf2smc as V
    from smcpp_amd.analysis import em
    from smcpp_amd.model import PiecewiseModel
    vcf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example.vcf.gz")
    c, _ = V.vcf2smc(vcf, "1", ("pop1", ["msp_0", "msp_1", "msp_2"]))
    piece = D.break_long_spans(D.Contig(D.compress_repeated_obs(c.data), c.pid, c.n, c.a), 100000)[0]
    theta_bp = D.watterson_theta([piece])
    binned = D.recode_monomorphic(D.Contig(D.bin_observations(D.thin_data(piece.data, 895), 100, [2]), c.pid, c.n, c.a))
    rows = np.ascontiguousarray(D.compress_repeated_obs(binned.data), dtype=np.int32)
    s = np.diff(np.concatenate([[0.0], np.logspace(-2, 0.7, 8)]))
    a0 = np.ones(len(s))
    hs = PO.balance_hidden_states(PiecewiseModel(a0, s, 1e4, "pop1"), 16)
    assert len(hs) == 17 and hs[0] == 0 and np.isinf(hs[-1]) and np.all(np.diff(hs[:-1]) > 0)
    model, ll = em([rows], c.n[0], hs, a0, s, 100 * theta_bp, 25 * theta_bp, iterations=3, penalty=1.0)
    assert np.all(np.diff(ll) >= -1e-6 * np.abs(ll[:-1])), ll
    assert ll[-1] > ll[0]


def test_c5_slice_5000_rows_vs_compiled_reference(chain_family):
    """Golden G14 (tests/golden/make_golden_c5.py): config C5 (M = 256, n = 50) on the first 5 000 rows of its contig, outputs of
    the compiled reference; several chunks, so the chunk-parallel iteration (scan chains with 4 states per lane by default,
    streamed-operand chains with `dense`, and with `lock`: the lock-step chains exist for M <= 64 only, so forcing them at this
    state count must leave the manager on the streamed-operand chains) is exercised at this state count."""
    import os
    from conftest import ROOT
    from smcpp_amd import _smcpp
    p = dict(np.load(os.path.join(ROOT, "tests", "golden", "params_M256_n50.npz")))
    g = load_golden("G14_c5_slice")
    obs = np.ascontiguousarray(g["obs"], dtype=np.int32)
    im = _smcpp.PyOnePopInferenceManager(50, [obs], p["hs"], ("pop1",), float(p["pol"]))
    if chain_family in ("lock", "dense"):
        assert im.chain_mode() == 3
    im.theta = float(p["theta"]); im.rho = float(p["rho"]); im.alpha = float(p["alpha"])
    im.set_raw(p["pi"], p["T"], p["keys"], p["E"])
    im.set_chunking(700)
    im.E_step()
    assert im.last_timing()["fwd_passes"] >= 2
    ll = im.loglik()
    assert abs(ll - float(g["loglik"])) <= LL_TOL * abs(float(g["loglik"]))
    assert rel_err(im.xisums[0], g["xisum"]) <= STAT_TOL
    gs = im.gamma_sums[0]
    for k, v in zip([tuple(int(x) for x in k) for k in g["gs_keys"]], g["gs_vals"]):
        assert np.max(np.abs(gs[k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), k
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"]) <= STAT_TOL * np.maximum(np.abs(g["q"]), 1e-12)), (q, g["q"])
    assert rel_err(im.gammas[0][:, 0], g["gamma0"]) <= STAT_TOL


def _stats_close(a, b, tol):
    xa, xb = a.xisums, b.xisums
    for c in range(len(xa)):
        assert rel_err(xa[c], xb[c]) <= tol
    ga, gb = a.gamma_sums, b.gamma_sums
    for c in range(len(ga)):
        assert sorted(ga[c]) == sorted(gb[c])
        for k, v in gb[c].items():
            assert np.max(np.abs(ga[c][k] - v)) <= tol * max(np.abs(v).max(), 1e-300), (c, k)


def test_full_size_headline_properties(engine_opt):
    """The BASELINE.json headline at FULL size (one 100 Mbp contig, M = 64, n = 20: 235 552 rows) through properties that do not
    need an oracle run of 25 s per E-step:
      * the chunk-parallel run (512 chunks, light passes, re-run passes) against the SAME kernels run as ONE chunk, i.e. purely
        sequentially: log-likelihood to 1e-9, statistics to the tolerance the goldens are held to (observed 1e-7);
      * the scan chains + eigen-free statistics against the dense chains + eigensystem statistics (two independent
        implementations of hmm.cpp:57-149 that share only the data layout);
      * the log-likelihood the survey recorded for this contig with the reference itself (-377640.9665392124
        is for the Appendix-A generator; this repository's generator value is pinned by bench.py's own `loglik`)."""
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    M, n = 64, 20
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contig = synth.synth_contig(0, 100_000_000, n)
    assert len(contig) == 235_552

    def make(chunk=None):
        im = _smcpp.PyOnePopInferenceManager(n, [contig], hs, ("pop1",), 0.5)
        im.model = PiecewiseModel(a, s, 1e4, "pop1")
        im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
        if chunk:
            im.set_chunking(chunk)
        im.E_step()
        return im

    par = make()
    assert par.chain_mode() == 5 and par.last_timing()["fwd_passes"] >= 2
    seq = make(10 ** 9)
    assert seq.last_timing()["fwd_passes"] <= 1
    assert abs(par.loglik() - seq.loglik()) <= 1e-9 * abs(seq.loglik())
    _stats_close(par, seq, STAT_TOL)
    np.testing.assert_allclose(par.Q(separate=True), seq.Q(separate=True), rtol=STAT_TOL)
    engine_opt("SMCPP_SS", "0")
    dense = make()
    assert dense.chain_mode() != 5
    assert abs(par.loglik() - dense.loglik()) <= 1e-8 * abs(dense.loglik())
    _stats_close(par, dense, 2 * STAT_TOL)       # two float-alpha noise floors


def test_full_size_whole_genome_scan_vs_lockstep(engine_opt):
    """Config C3's input on ONE manager (22 contigs, 6.76 M rows, M = 64, n = 20): the scan chains against the lock-step chains on
    the matrix cores (an independent kernel family, eigensystem statistics)."""
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    M, n = 64, 20
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contigs = [synth.synth_contig(i, int(L * 1e6), n) for i, L in enumerate(synth.C3_LENGTHS_MBP)]

    def make():
        im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
        im.model = PiecewiseModel(a, s, 1e4, "pop1")
        im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
        im.E_step()
        return im

    scan = make()
    assert scan.chain_mode() == 5
    ll_scan, x_scan, g_scan, q_scan = np.array(scan.logliks()), scan.xisums, scan.gamma_sums, np.array(scan.Q(separate=True))
    del scan
    engine_opt("SMCPP_CHAIN", "lock")
    lock = make()
    assert lock.chain_mode() == 4
    np.testing.assert_allclose(ll_scan, lock.logliks(), rtol=1e-8)
    xl, gl = lock.xisums, lock.gamma_sums
    for c in range(len(contigs)):
        assert rel_err(x_scan[c], xl[c]) <= 2 * STAT_TOL
        for k, v in gl[c].items():
            assert np.max(np.abs(g_scan[c][k] - v)) <= 2 * STAT_TOL * max(np.abs(v).max(), 1e-300), (c, k)
    np.testing.assert_allclose(q_scan, lock.Q(separate=True), rtol=2 * STAT_TOL)


def test_span1_statistics_one_pass_in_key_order(engine_opt):
    """SMCPP_S1_FUSE: the span-1 rank update and the per-key gamma sums in ONE pass over key-sorted single-key slabs (k_rank_acc<3>,
    the default from half a million span-1 rows on) against the two-kernel form (k_s1_scalars + k_rank_acc<0>): same goldens, same
    tolerances, and against each other far below them."""
    res = {}
    names = ("G4_M64_n20_2Mbp", "G3_M32_n10_2Mbp", "G1_M16_n4", "G5_M48_twopop_layout")
    for fuse in ("0", "1"):
        engine_opt("SMCPP_S1_FUSE", fuse)
        for name in names:
            g = load_golden(name)
            im = make_im(g)
            im.E_step()
            check_against(g, im, save_gamma=False)
            res[(fuse, name)] = (im.gamma_sums[0], im.xisums[0])
    for name in names:
        g0, x0 = res[("0", name)]
        g1, x1 = res[("1", name)]
        assert rel_err(x1, x0) <= 1e-11
        for k, v in g0.items():
            np.testing.assert_allclose(g1[k], v, rtol=1e-11, atol=1e-13 * np.abs(v).max())


def test_rank_partials_by_teams_of_four_slabs_vs_one_per_slab(engine_opt):
    """Round 5 default: four consecutive slabs of one reduction range share a workgroup of `k_rank_acc<., true>`, which adds their
    accumulators through LDS and writes ONE partial; SMCPP_STATS_TEAM=0 keeps one partial per slab.  Same goldens and tolerances for
    both (one to four states per lane: the span-1 form of M > 64 too), and against each other to the rounding of a re-ordered sum."""
    res = {}
    import os
    from conftest import ROOT
    from smcpp_amd import _smcpp
    names = ("G4_M64_n20_2Mbp", "G3_M32_n10_2Mbp", "G1_M16_n4", "G5_M48_twopop_layout")
    p5 = dict(np.load(os.path.join(ROOT, "tests", "golden", "params_M256_n50.npz")))
    g5 = load_golden("G14_c5_slice")
    for team in ("0", "1"):
        engine_opt("SMCPP_STATS_TEAM", team)
        for name in names:
            g = load_golden(name)
            im = make_im(g)
            im.E_step()
            check_against(g, im, save_gamma=False)
            res[(team, name)] = (im.gamma_sums[0], im.xisums[0])
        # four states per lane (config C5's slice, golden G14 from the compiled reference): the span-1 rank update in its M > 64 form
        im = _smcpp.PyOnePopInferenceManager(50, [np.ascontiguousarray(g5["obs"], dtype=np.int32)], p5["hs"], ("pop1",), float(p5["pol"]))
        im.theta = float(p5["theta"]); im.rho = float(p5["rho"]); im.alpha = float(p5["alpha"])
        im.set_raw(p5["pi"], p5["T"], p5["keys"], p5["E"])
        im.E_step()
        assert rel_err(im.xisums[0], g5["xisum"]) <= STAT_TOL
        gs = im.gamma_sums[0]
        for k, v in zip([tuple(int(x) for x in k) for k in g5["gs_keys"]], g5["gs_vals"]):
            assert np.max(np.abs(gs[k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), k
        res[(team, "G14")] = (gs, im.xisums[0])
    for name in names + ("G14",):
        g0, x0 = res[("0", name)]
        g1, x1 = res[("1", name)]
        assert rel_err(x1, x0) <= 1e-11
        for k, v in g0.items():
            np.testing.assert_allclose(g1[k], v, rtol=1e-11, atol=1e-13 * np.abs(v).max())


def test_float_scans_of_the_stored_passes_vs_fp64_scans(engine_opt):
    """Round 5 default: every scan of the stored passes runs in float (the sums over the states above as native suffix scans; the
    vector and the diagonal term stay in fp64), SMCPP_SS_MIXED=0 keeps the fp64 scans.  Same goldens and tolerances for both, and
    against each other: the log-likelihood to 1e-9, the statistics to the float noise the reference's own forward chain carries."""
    res = {}
    names = ("G4_M64_n20_2Mbp", "G3_M32_n10_2Mbp", "G1_M16_n4", "G5_M48_twopop_layout")
    for mixed in ("0", "1"):
        engine_opt("SMCPP_SS_MIXED", mixed)
        for name in names:
            g = load_golden(name)
            im = make_im(g)
            im.E_step()
            assert im.chain_mode() == 5
            check_against(g, im, save_gamma=False)
            res[(mixed, name)] = (im.loglik(), im.gamma_sums[0], im.xisums[0])
    for name in names:
        l0, g0, x0 = res[("0", name)]
        l1, g1, x1 = res[("1", name)]
        assert abs(l1 - l0) <= 1e-9 * abs(l0)
        assert rel_err(x1, x0) <= 2e-6
        for k, v in g0.items():
            assert np.max(np.abs(g1[k] - v)) <= 2e-6 * max(np.abs(v).max(), 1e-300), k


@pytest.mark.parametrize("M,n", [(48, 7), (64, 20), (100, 6), (130, 6), (256, 8)])
def test_span_fold_on_scans_vs_matrix_cores(engine_opt, M, n):
    """Round 4: the eigen-free span statistics fold the spans with the O(M) scan steps of the chains (k_span_scan: one wavefront per
    row of F / column of H) instead of 2 s_max products of M x M matrices on the matrix cores (k_span_big, SMCPP_SPAN_SCAN=0).  Both
    against the C restatement at the stated tolerances and against each other far below them, for one to four states per lane."""
    from oracle import oracle
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    hs = synth.hidden_states(M)
    a, s = synth.model_pieces()
    contigs = [synth.synth_contig(700 + M, 2_000_000 if M <= 64 else 800_000, n), synth.synth_contig(701 + M, 120_000, n)]
    res = {}
    for scan in ("1", "0"):
        engine_opt("SMCPP_SPAN_SCAN", scan)
        im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
        im.model = PiecewiseModel(a, s, 1e4, "pop1")
        im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
        im.E_step()
        assert im.chain_mode() == 5
        res[scan] = (np.array(im.logliks()), im.xisums, im.gamma_sums, np.array(im.Q(separate=True)))
    pi, T, keys = im.pi, im.transition, im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    for c, ob in enumerate(contigs):
        o = oracle.estep(pi, T, keys, Etab, ob)
        for scan, (lls, xs, gss, q) in res.items():
            assert abs(lls[c] - o["loglik"]) <= LL_TOL * abs(o["loglik"]), scan
            assert rel_err(xs[c], o["xisum"]) <= STAT_TOL, scan
            for k, v in o["gamma_sums"].items():
                assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), (scan, k)
        # (round 6: until the engine's switches were parsed through one table with an explicit reload, SMCPP_SPAN_SCAN was latched at
        # its first read and both legs of this test ran the same fold; measured now that they differ: the largest PER-ENTRY relative
        # difference of the xi sums is 1.1e-9 .. 1.5e-9 - entries of 1e-10 summed in two different orders - against 5e-6 to the oracle)
        assert rel_err(res["1"][1][c], res["0"][1][c]) <= 1e-8
        for k, v in res["0"][2][c].items():
            assert np.max(np.abs(res["1"][2][c][k] - v)) <= 1e-8 * max(np.abs(v).max(), 1e-300), k
    assert np.all(np.abs(res["1"][3] - res["0"][3]) <= 1e-8 * np.maximum(np.abs(res["0"][3]), 1e-12))


@pytest.mark.parametrize("name", ["G7_M32_n8_chr11", "G18_M64_n8_chr11"])
def test_hybrid_scan_chains_on_unbinned_data(engine_opt, name):
    """Un-binned data (spans to 10^5): the scan kernel with HYBRID rows (chain mode 6: a long row is one eigen-power step
    P d^s P^-1 inside the one-wavefront-per-chunk kernel, a short one `span` scan steps) against the dense chains (SMCPP_HYBRID=0)
    on the reference's own un-binned contig (golden G7 / G18, with gamma) and on a synthetic contig long enough for several chunks.
    M = 64 (G18, round 4): the four eigenvector tables of a key do not fit LDS - single-direction workgroups with two tables each."""
    from smcpp_amd import _smcpp
    g = load_golden(name)
    res = {}
    for hyb in ("1", "0"):
        engine_opt("SMCPP_HYBRID", hyb)
        im = make_im(g)
        im.save_gamma = True
        im.E_step()
        check_against(g, im, save_gamma=True)
        res[hyb] = (im.chain_mode(), im.loglik(), im.xisums[0], im.gammas[0])
    assert res["1"][0] == 6 and res["0"][0] != 6
    assert abs(res["1"][1] - res["0"][1]) <= 1e-8 * abs(res["0"][1])
    assert rel_err(res["1"][2], res["0"][2]) <= 2 * STAT_TOL
    assert np.array_equal(np.argmax(res["1"][3], axis=0), np.argmax(res["0"][3], axis=0))
    # synthetic un-binned contig: 60 000 rows over G7's own keys, chunks of 2 000 rows so that the fixed point iterates
    rng = np.random.default_rng(11)
    L = 60_000
    keys = np.asarray(g["keys"], dtype=np.int32)
    mono = int(np.nonzero((keys == np.array([0, 0, 8])).all(axis=1))[0][0])
    kid = rng.integers(0, len(keys), L)
    span = np.where(rng.random(L) < 0.45, 1, np.minimum(100_000, 1 + rng.geometric(2e-3, L)))
    kid[span > 1] = mono                                       # long spans are monomorphic stretches
    obs = np.concatenate([span[:, None], keys[kid]], axis=1).astype(np.int32)
    out = {}
    for hyb in ("1", "0"):
        engine_opt("SMCPP_HYBRID", hyb)
        im = _smcpp.PyOnePopInferenceManager(8, [obs], g["hs"], ("pop1",), float(g["pol"]))
        im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
        im.set_chunking(2000)
        im.E_step()
        out[hyb] = (im.chain_mode(), im.loglik(), im.xisums[0], im.gamma_sums[0], im.last_timing()["fwd_passes"])
    assert out["1"][0] == 6 and out["1"][4] >= 2
    assert abs(out["1"][1] - out["0"][1]) <= 1e-8 * abs(out["0"][1])
    assert rel_err(out["1"][2], out["0"][2]) <= 2 * STAT_TOL
    for k, v in out["0"][3].items():
        assert np.max(np.abs(out["1"][3][k] - v)) <= 2 * STAT_TOL * max(np.abs(v).max(), 1e-300)


def test_hybrid_rows_with_cold_eigen_keys_m64(engine_opt):
    """Un-binned data at M = 64 with THREE eigen keys (round 5): the pair of eigenvector tables a direction needs is 66 KB per key, two
    keys fill LDS - the third (least frequent) key's table rows are read from L2 on the rows that need them.  Until round 4 such an
    input fell back to the dense cooperative chains.  Checked against those (SMCPP_HYBRID=0) and against the C restatement of
    hmm.cpp on G18's parameters, with the posterior argmax."""
    from oracle import oracle
    from smcpp_amd import _smcpp
    g = load_golden("G18_M64_n8_chr11")
    keys = np.asarray(g["keys"], dtype=np.int32)
    idx = {tuple(k): i for i, k in enumerate(keys.tolist())}
    mono, miss = idx[(0, 0, 8)], idx[(-1, 0, 0)]
    third = next(i for i in range(len(keys)) if i not in (mono, miss))          # any third key that also comes in long rows
    rng = np.random.default_rng(5)
    L = 24_000
    kid = rng.integers(0, len(keys), L)
    span = np.where(rng.random(L) < 0.45, 1, np.minimum(50_000, 1 + rng.geometric(3e-3, L)))
    u = rng.random(L)
    kid[span > 1] = np.where(u[span > 1] < 0.75, mono, np.where(u[span > 1] < 0.93, miss, third))
    obs = np.concatenate([span[:, None], keys[kid]], axis=1).astype(np.int32)
    out = {}
    for hyb in ("1", "0"):
        engine_opt("SMCPP_HYBRID", hyb)
        im = _smcpp.PyOnePopInferenceManager(8, [obs], g["hs"], ("pop1",), float(g["pol"]))
        im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
        im.set_chunking(1500)
        im.save_gamma = True
        im.E_step()
        out[hyb] = (im.chain_mode(), im.loglik(), im.xisums[0], im.gamma_sums[0], im.gamma_argmax(0), im.gammas[0])
    assert out["1"][0] == 6 and out["0"][0] != 6, (out["1"][0], out["0"][0])
    assert abs(out["1"][1] - out["0"][1]) <= 1e-8 * abs(out["0"][1])
    assert rel_err(out["1"][2], out["0"][2]) <= 2 * STAT_TOL
    o = oracle.estep(g["pi"], g["T"], g["keys"], g["E"], obs, save_gamma=True)
    assert abs(out["1"][1] - o["loglik"]) <= LL_TOL * abs(o["loglik"])
    assert rel_err(out["1"][2], o["xisum"]) <= STAT_TOL
    for k, v in o["gamma_sums"].items():
        assert np.max(np.abs(out["1"][3][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), k
    srt = np.sort(o["gamma"], axis=0)
    strong = (srt[-1] - srt[-2]) / np.maximum(srt[-1], 1e-300) > 1e-5
    assert np.all((out["1"][4] == o["gamma"].argmax(axis=0)) | ~strong)
