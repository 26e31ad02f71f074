"""Every kernel family on poisoned memory, and managers that are reused against fresh ones.

`hipMalloc` hands out zeroed pages in a fresh process and recycled ones later, and a manager that has run keeps its buffers with the
previous E-step's values in them: a kernel that reads memory nobody wrote in THIS E-step, or a stream that starts before the copy it
reads has landed, is right by accident everywhere else in the suite.  Two such races were found by hand (the parameter
arena read on a side stream before its copy, `enqueue_stats` `arena_wait`; the row-0 memset of the per-row posteriors queued behind
the chains' fork event).  Here they are deterministic failures:

  * SMCPP_DEBUG_POISON=nan (engine_options.hpp) fills every fresh allocation of float / double data with 0xFF bytes (NaN in both
    widths; integer buffers stay as the allocator returns them, so nothing can become a wild address or an endless wait), and on
    every E-step fills the parameter arena in front of its copy and the per-row posteriors before the chains start, in stream order.
    A read before write or a missing wait then turns an output into NaN.
  * test_kernel_families_on_poisoned_memory: each case runs twice in one process, clean and poisoned (switch set before the manager
    is constructed), two E-steps each; every output must be finite, poisoned must equal clean bit for bit (the engine reduces in a
    fixed order), and the clean run must pass the golden / C-restatement check of the test the setup comes from.
  * test_reused_manager_equals_fresh_managers: one manager walks through parameter sets and save_gamma switches and must give at
    every state what a manager built for that state gives.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, rel_err
from test_gpu_argmax import _check_stats, _load as _load_headline, _manager as _headline_manager, argmax_report
from test_gpu_parity import LL_TOL, STAT_TOL, check_against, check_gamma_columns, make_im

pytestmark = pytest.mark.gpu

STAT_TOL_WIDE = 1e-5          # 512 < M <= 1024: the statistics' tolerance of tests/test_gpu_bigm.py


# ---------------------------------------------------------------------------------------------------------------------------------
# outputs and the two runs of a case
# ---------------------------------------------------------------------------------------------------------------------------------
def _outputs(im, save_gamma, gradient=False, steps=2):
    """Every output of a manager after `steps` E-steps (the second takes the launch counts the first one adapted)."""
    for _ in range(steps):
        im.E_step()
    nc = len(im.logliks())
    out = {"loglik": np.array(im.logliks()), "xisum": np.array(im.xisums)}
    gs = im.gamma_sums
    out["gamma_sums"] = np.array([gs[c][k] for c in range(nc) for k in sorted(gs[c])])
    out["gamma_keys"] = np.array([k for c in range(nc) for k in sorted(gs[c])], dtype=np.int64)
    out["q"] = np.array(im.Q(separate=True))
    out["gammas"] = np.concatenate([g.ravel() for g in im.gammas])
    if save_gamma:
        out["argmax"] = np.concatenate([np.asarray(im.gamma_argmax(c)) for c in range(nc)])
    if gradient:
        q, jac = im.Q_with_gradient()
        out["q_grad"] = np.concatenate([np.asarray(q).ravel(), np.asarray(jac).ravel()])
    return out


def _clean_and_poisoned(engine_opt, build, check, save_gamma, gradient=False):
    """build() -> a configured manager (save_gamma set); check(im) -> the golden / oracle check of the clean run."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    im = build()
    im.save_gamma = save_gamma
    clean = _outputs(im, save_gamma, gradient)
    check(im)
    del im
    engine_opt("SMCPP_DEBUG_POISON", "nan")
    im = build()
    im.save_gamma = save_gamma
    poisoned = _outputs(im, save_gamma, gradient)
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    assert sorted(poisoned) == sorted(clean)
    for k, v in clean.items():
        p = poisoned[k]
        assert np.all(np.isfinite(v)), f"clean run: {k} is not finite"
        assert np.all(np.isfinite(p)), f"poisoned run: {k} holds {int(np.sum(~np.isfinite(p)))} non-finite entries"
        assert p.shape == v.shape and np.array_equal(p, v), \
            f"poisoned run differs from the clean one in {k}: {int(np.sum(p != v))} entries, largest {np.max(np.abs(p - v)):.3e}"
    return clean


# ---------------------------------------------------------------------------------------------------------------------------------
# checks of the clean run against the C restatement (oracle/), fed with the engine's own prepared parameters
# ---------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}      # (parameters, contig) -> the restatement's E-step: cases that share a setup (M = 768 lean / save_gamma) run it once


def _oracle_estep(pi, T, keys, Etab, obs, gamma):
    import hashlib
    from oracle import oracle
    h = hashlib.sha1(b"gamma" if gamma else b"")
    for x in (pi, T, keys, Etab, obs):
        h.update(np.ascontiguousarray(x).tobytes())
    if h.hexdigest() not in _ORACLE:
        _ORACLE[h.hexdigest()] = oracle.estep(pi, T, keys, Etab, obs, save_gamma=gamma)
    return _ORACLE[h.hexdigest()]


def _oracle_check(contigs, every=1, stat_tol=STAT_TOL, gamma=False, xs_entry_tol=None, first=0, oracle_gamma=None):
    def check(im):
        keys = im.keys
        ep = im.emission_probs
        Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
        pi, T = im.pi, im.transition
        lls, xs, gss = im.logliks(), im.xisums, im.gamma_sums
        gams = im.gammas if gamma else None
        for c in range(first, len(contigs), every):
            o = _oracle_estep(pi, T, keys, Etab, contigs[c], gamma if oracle_gamma is None else oracle_gamma)
            assert abs(lls[c] - o["loglik"]) <= LL_TOL * max(1.0, abs(o["loglik"])), (c, lls[c], o["loglik"])
            if xs_entry_tol is None:
                assert rel_err(xs[c], o["xisum"]) <= stat_tol, c
            else:        # (long rows in one eigen-power step: see test_long_rows_of_binned_data_cut_into_pieces)
                assert rel_err(xs[c], o["xisum"]) <= xs_entry_tol, c
                assert np.abs(xs[c] - o["xisum"]).max() <= stat_tol * np.abs(o["xisum"]).max(), c
            assert sorted(gss[c].keys()) == sorted(o["gamma_sums"].keys())
            for k, v in o["gamma_sums"].items():
                assert np.max(np.abs(gss[c][k] - v)) <= stat_tol * max(np.abs(v).max(), 1e-300), (c, k)
            if gamma:
                ob = contigs[c]
                assert gams[c].shape == o["gamma"].shape
                spans = np.concatenate([[1.0], ob[:, 0].astype(float)])
                assert np.max(np.max(np.abs(gams[c] - o["gamma"]), axis=0) / spans) <= 2e-5, c
                if im.M > 1:
                    top2 = np.sort(o["gamma"], axis=0)[-2:]
                    strong = (top2[1] - top2[0]) > 1e-5 * spans
                    assert not np.any(strong & (gams[c].argmax(axis=0) != o["gamma"].argmax(axis=0))), c
                check_gamma_columns(gams[c], o["gamma"], ob, arg_dev=im.gamma_argmax(c), label=f"contig {c}")
    return check


def _model_manager(n, contigs, M=None, hs=None, theta=None, rho=None, pol=0.5, a=None, s=None, chunk=0):
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    if a is None:
        a, s = synth.model_pieces()
    im = _smcpp.PyOnePopInferenceManager(n, contigs, synth.hidden_states(M) if hs is None else hs, ("pop1",), pol)
    im.model = PiecewiseModel(a, s, 1e4, "pop1")
    im.theta = synth.THETA if theta is None else theta
    im.rho = synth.RHO if rho is None else rho
    im.alpha = 1.0
    if chunk:
        im.set_chunking(chunk)
    return im


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (setups of the tests named in each comment)
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDENS = ["G1_M16_n4", "G2_M51_n6_longspans", "G3_M32_n10_2Mbp", "G4_M64_n20_2Mbp", "G5_M48_twopop_layout", "G6_M1_n4",
           "G7_M32_n8_chr11", "G18_M64_n8_chr11"]
CASES = [f"golden:{g}:{fam}:{sg}" for g in GOLDENS for fam in ("default", "dense", "lock") for sg in (0, 1)]
CASES += ["gammaeig:G4_M64_n20_2Mbp", "gammaeig:G5_M48_twopop_layout",        # per-row gammas from the eigensystems
          "hybrid:G7_M32_n8_chr11", "hybrid:G18_M64_n8_chr11",                # hybrid scan chains on un-binned rows
          "model:params_M32_n10", "model:params_M64_n20", "model:params_M256_n50",
          "twopop:2:0", "twopop:1:1", "m1",
          "sweep:33", "sweep:130",                                             # padding columns with save_gamma (G2 above: M = 51)
          "cut:144", "cut:300", "pieces:128:1", "pieces:96:2",
          "pieces:150:2", "pieces:130:2:eig",                                  # three states per lane; k_span_q + k_gamma_rows_eig
          "bigm:512:0", "bigm:768:0", "bigm:768:1", "bigm:1024:0",
          "tiny", "headline:0", "headline:1"]


def _case(case, engine_opt):
    """-> (build, check, save_gamma, gradient)"""
    from smcpp_amd import _smcpp, synth
    kind, *arg = case.split(":")
    if kind == "golden":
        # test_gpu_parity.py: test_golden_stats / test_golden_posterior over the chain_family fixture
        name, fam, sg = arg[0], arg[1], bool(int(arg[2]))
        if fam == "lock":
            engine_opt("SMCPP_CHAIN", "lock")
        if fam == "dense":
            engine_opt("SMCPP_SS", "0")
        g = load_golden(name)

        def build():
            im = make_im(g)
            if fam == "lock":
                assert im.chain_mode() == 4
            if fam == "dense":
                assert im.chain_mode() != 5
            return im
        return build, lambda im: check_against(g, im, save_gamma=sg), sg, False
    if kind == "gammaeig":
        # test_per_row_gamma_from_scan_steps_vs_eigensystems, SMCPP_GAMMA_SCAN=0
        engine_opt("SMCPP_GAMMA_SCAN", "0")
        g = load_golden(arg[0])

        def build():
            im = make_im(g)
            return im

        def check(im):
            assert im.describe()["plan"]["per_row_gamma"] == "eigensystem"
            check_against(g, im, save_gamma=True)
        return build, check, True, False
    if kind == "hybrid":
        # test_hybrid_scan_chains_on_unbinned_data (the golden contig, hybrid rows on)
        g = load_golden(arg[0])

        def check(im):
            assert im.chain_mode() == 6
            check_against(g, im, save_gamma=True)
        return lambda: make_im(g), check, True, False
    if kind == "model":
        # tools/poison_probe.py `model:`: the engine's own cold preparation, two contigs, Q with its gradient
        p = dict(np.load(os.path.join(GOLDEN, arg[0] + ".npz")))
        n = int(p["n"])
        contigs = [synth.synth_contig(1, 3_000_000, n), synth.synth_contig(2, 400_000, n)]

        def build():
            from smcpp_amd.model import PiecewiseModel
            im = _smcpp.PyOnePopInferenceManager(n, contigs, p["hs"], ("pop1",), float(p["pol"]))
            im.theta = float(p["theta"]); im.rho = float(p["rho"]); im.alpha = float(p["alpha"])
            im.model = PiecewiseModel(p["a"], p["s"], 1e4, "pop1")
            return im
        # (the restatement takes 2 M^3 flop per span > 1 row on one core: at M = 256 the short contig only)
        return build, _oracle_check(contigs, first=0 if len(p["hs"]) <= 65 else 1), False, True
    if kind == "twopop":
        # test_two_population_model_path, (a1, a2) = (2, 0) / (1, 1), M = 24
        a1, a2 = int(arg[0]), int(arg[1])
        contigs = _twopop_contigs(a1)

        def build():
            im = _smcpp.PyTwoPopInferenceManager(6, 5, a1, a2, contigs, synth.hidden_states(24), ("pop1", "pop2"), 0.5)
            im.model = _twopop_model(0.3 if a1 == 2 else 0.005)
            im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
            return im
        return build, _oracle_check(contigs), False, False
    if kind == "m1":
        # tools/poison_probe.py `m1:`: ONE hidden state (the bootstrap manager of Analysis)
        p = dict(np.load(os.path.join(GOLDEN, "params_M32_n10.npz")))
        n = int(p["n"])
        contigs = [synth.synth_contig(3, 2_000_000, n)]

        def build():
            from smcpp_amd.model import PiecewiseModel
            im = _smcpp.PyOnePopInferenceManager(n, contigs, np.array([0.0, np.inf]), ("pop1",), float(p["pol"]))
            im.theta = float(p["theta"]); im.rho = float(p["rho"]); im.alpha = 1.0
            im.model = PiecewiseModel(p["a"], p["s"], 1e4, "pop1")
            return im
        return build, _oracle_check(contigs), False, False
    if kind == "sweep":
        # test_state_count_sweep_vs_oracle: (33, 8, 300 000) and (130, 6, 120 000), three ragged contigs, save_gamma
        M = int(arg[0])
        n, length = {33: (8, 300_000), 130: (6, 120_000)}[M]
        contigs = [synth.synth_contig(100 + M + i, L, n) for i, L in enumerate([length, length // 3, 20_000])]
        return lambda: _model_manager(n, contigs, M=M), _oracle_check(contigs, gamma=True), True, False
    if kind == "cut":
        # rows of binned data longer than 64 positions cut into pieces: tools/poison_probe.py `cut:` (M = 144, 1 500 rows of G1) and
        # test_long_rows_of_binned_data_cut_into_pieces (M = 300, 700 rows), save_gamma
        M = int(arg[0])
        g = load_golden("G1_M16_n4")
        obs = [np.ascontiguousarray(g["obs"][:1500 if M == 144 else 700], dtype=np.int32)]

        def build():
            im = _model_manager(4, obs, M=M, theta=float(g["theta"]), rho=float(g["rho"]))
            assert im.describe()["plan"]["long_rows_cut"]
            return im
        return build, _oracle_check(obs, gamma=True, xs_entry_tol=5e-5), True, False
    if kind == "pieces":
        # test_unbinned_rows_gamma_from_eigen_power_pieces: un-binned rows, per-row gammas from eigen-power pieces (k_piece_vectors)
        # ("eig": SMCPP_GAMMA_PIECES=0, the eigensystem kernel of M > 64 on the same rows)
        M, nc, eig = int(arg[0]), int(arg[1]), arg[2:] == ["eig"]
        rows = 400 if M == 128 else 300
        contigs = [np.ascontiguousarray(synth.synth_posterior_contig(rows - 40 * c, 8, seed=11 + c), dtype=np.int32) for c in range(nc)]
        engine_opt("SMCPP_SPLIT_SPANS", "0")
        if eig:
            engine_opt("SMCPP_GAMMA_PIECES", "0")

        def build():
            im = _model_manager(8, contigs, M=M, theta=2e-4, rho=6e-5)
            return im

        def check(im):
            assert im.describe()["plan"]["per_row_gamma"] == ("eigensystem" if eig else "eigen-power pieces + scan steps")
            _oracle_check(contigs, gamma=True)(im)
        return build, check, True, False
    if kind == "bigm":
        # test_more_than_256_states_vs_oracle: M = 512 / 768 / 1024 on 160 / 70 / 40 rows (M = 768 on 70 rows: the arena race's case)
        M, sg = int(arg[0]), bool(int(arg[1]))
        rows, chunk = {512: (160, 60), 768: (70, 30), 1024: (40, 18)}[M]
        obs = [np.ascontiguousarray(synth.synth_contig(0, 100_000_000, 10)[:rows], dtype=np.int32)]

        def build():
            im = _model_manager(10, obs, M=M, chunk=chunk)
            assert im.chain_mode() == 5
            return im
        return build, _oracle_check(obs, stat_tol=STAT_TOL if M <= 512 else STAT_TOL_WIDE, gamma=sg, oracle_gamma=True), sg, False
    if kind == "tiny":
        # test_many_tiny_contigs: 300 contigs of 1 - 40 rows (row 0 of every contig cleared on its own), with save_gamma
        g = load_golden("G3_M32_n10_2Mbp")
        rng = np.random.default_rng(7)
        big = synth.synth_contig(77, 3_000_000, 10)
        contigs, pos = [], 0
        for _ in range(300):
            L = int(rng.integers(1, 41))
            contigs.append(np.ascontiguousarray(big[pos:pos + L]))
            pos += L

        def build():
            im = _smcpp.PyOnePopInferenceManager(10, contigs, g["hs"], ("pop1",), 0.5)
            im.theta = float(g["theta"]); im.rho = float(g["rho"])
            im.set_raw(g["pi"], g["T"], g["keys"], g["E"])
            return im
        return build, _oracle_check(contigs, every=7, gamma=True), True, False
    if kind == "headline":
        # test_gpu_argmax.py: the headline contig (G19, M = 64, 100 Mbp) on the params route - the lean E-step bench.py times (light
        # passes, float scans in the stored passes) against the compiled reference's statistics, and save_gamma against its decode
        sg = bool(int(arg[0]))
        g, obs = _load_headline("G19_headline")

        def check(im):
            assert im.chain_mode() == 5
            if not sg:
                _check_stats(im, g)
                return
            assert abs(im.loglik() - float(g["loglik"])) <= LL_TOL * abs(float(g["loglik"]))
            assert im.describe()["plan"]["float_scans_in_stored_passes"]
            _, strong, _ = argmax_report(im.gamma_argmax(0), g)
            assert len(strong) == 0
            gam = im.gammas[0]
            st = int(g["gamma_stride"])
            assert np.max(np.abs(gam[:, ::st] - g["gamma_sub"])) <= 2e-5 * max(1.0, float(np.abs(g["gamma_sub"]).max()))
        return lambda: _headline_manager(g, obs, "params"), check, sg, False
    raise AssertionError(case)


def _twopop_contigs(a1):
    from smcpp_amd import synth
    contigs = []
    for ci, L in enumerate([400_000, 150_000]):
        obs = synth.synth_contig_twopop(3 + ci, L, 6, 5).copy()
        if a1 == 1:
            nm = obs[:, 1] >= 0
            obs[nm, 4] = (obs[nm, 2] + obs[nm, 6] + obs[nm, 0]) % 2
            obs[~nm, 4] = -1
        contigs.append(np.ascontiguousarray(obs, dtype=np.int32))
    return contigs


def _twopop_model(split, a=None):
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    a0, s = synth.model_pieces()
    m1 = PiecewiseModel(a0 if a is None else a, s, 1e4, pid="pop1")
    m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(8)), s[:8], 1e4, pid="pop2")
    return TwoPopulationModel(m1, m2, split)


@pytest.mark.parametrize("case", CASES)
def test_kernel_families_on_poisoned_memory(engine_opt, case):
    build, check, save_gamma, gradient = _case(case, engine_opt)
    _clean_and_poisoned(engine_opt, build, check, save_gamma, gradient)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. one manager through a sequence of states against a fresh manager per state
# ---------------------------------------------------------------------------------------------------------------------------------
def _setup(kind):
    """-> (make(a, theta) -> manager, model_of(a) -> model, a0, theta0)"""
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    if kind == "scan":
        # test_warm_start_matches_cold_start: 30 Mbp at M = 64, 300 rows per chunk (several passes, light passes)
        g = load_golden("G4_M64_n20_2Mbp")
        obs = synth.synth_contig(0, 30_000_000, 20)

        def model_of(a):
            return PiecewiseModel(a, g["s"], 1e4, "pop1")

        def make(a, theta):
            im = _smcpp.PyOnePopInferenceManager(20, [obs], g["hs"], ("pop1",), float(g["pol"]))
            im.theta = theta; im.rho = float(g["rho"]); im.alpha = float(g["alpha"])
            im.set_chunking(300)
            im.model = model_of(a)
            return im
        return make, model_of, np.array(g["a"], dtype=float), float(g["theta"])
    if kind == "m768":
        # test_more_than_256_states_vs_oracle's M = 768 on 70 rows, 30 rows per chunk
        obs = [np.ascontiguousarray(synth.synth_contig(0, 100_000_000, 10)[:70], dtype=np.int32)]
        a0, s = synth.model_pieces()

        def model_of(a):
            return PiecewiseModel(a, s, 1e4, "pop1")

        def make(a, theta):
            return _model_manager(10, obs, M=768, theta=theta, a=a, s=s, chunk=30)
        return make, model_of, np.array(a0, dtype=float), synth.THETA
    # test_two_population_model_path's (a1, a2) = (2, 0), M = 24: the first population's `a` moves
    contigs = _twopop_contigs(2)
    a0, _ = synth.model_pieces()

    def model_of(a):
        return _twopop_model(0.3, a)

    def make(a, theta):
        im = _smcpp.PyTwoPopInferenceManager(6, 5, 2, 0, contigs, synth.hidden_states(24), ("pop1", "pop2"), 0.5)
        im.model = model_of(a)
        im.theta = theta; im.rho = synth.RHO; im.alpha = 1.0
        return im
    return make, model_of, np.array(a0, dtype=float), synth.THETA


def _state_outputs(im, save_gamma):
    t = im.last_timing()
    out = {"loglik": np.array(im.logliks()), "xisum": np.array(im.xisums)}
    gs = im.gamma_sums
    nc = len(out["loglik"])
    out["gamma_sums"] = np.array([gs[c][k] for c in range(nc) for k in sorted(gs[c])])
    if save_gamma:
        out["argmax"] = np.concatenate([np.asarray(im.gamma_argmax(c)) for c in range(nc)])
        out["gammas"] = np.concatenate([g.ravel() for g in im.gammas])
    return out, (int(t["fwd_passes"]), int(t["bwd_passes"]))


@pytest.mark.parametrize("kind", ["scan", "m768", "twopop"])
def test_reused_manager_equals_fresh_managers(engine_opt, kind):
    """States: P0; P1 = P0's `a` reversed x 2.5 and theta x 1.5; save_gamma on; P2 = P1 perturbed (`a` x 0.6 with a 10 % ripple,
    theta x 0.8: a ripple and theta x 0.85 alone moved the 30 Mbp contig's log-likelihood by 1.7e-4 only); save_gamma off; P0 again.
    At every state the reused manager against a manager built for it: log-likelihood to 1e-10, xi / gamma sums to 1e-9, the same
    decoded index, bit for bit where both ran the same passes; every change of the parameters moves the log-likelihood by 1e-3 or
    more (a kernel that read the previous state's parameters cannot pass by luck).  Clean and under SMCPP_DEBUG_POISON=nan, and the
    two sequences against each other bit for bit."""
    make, model_of, a0, th0 = _setup(kind)
    k = np.arange(len(a0))
    a1, th1 = a0[::-1] * 2.5, th0 * 1.5
    a2, th2 = a1 * 0.6 * (1.0 + 0.1 * np.sin(k)), th1 * 0.8
    states = [(a0, th0, False), (a1, th1, False), (a1, th1, True), (a2, th2, True), (a2, th2, False), (a0, th0, False)]
    seqs = {}
    for mode in (None, "nan"):
        engine_opt("SMCPP_DEBUG_POISON", mode)
        im = make(a0, th0)
        seq = []
        prev_ll = None
        for i, (a, th, sg) in enumerate(states):
            im.model = model_of(a)
            im.theta = th
            im.save_gamma = sg
            im.E_step()
            got, passes = _state_outputs(im, sg)
            fresh = make(a, th)
            fresh.save_gamma = sg
            fresh.E_step()
            want, fpasses = _state_outputs(fresh, sg)
            del fresh
            for key, v in got.items():
                assert np.all(np.isfinite(v)), (mode, i, key)
            ll, llf = got["loglik"].sum(), want["loglik"].sum()
            assert abs(ll - llf) <= 1e-10 * abs(llf), (mode, i, ll, llf)
            assert rel_err(got["xisum"], want["xisum"]) <= 1e-9, (mode, i)
            assert np.max(np.abs(got["gamma_sums"] - want["gamma_sums"])) <= 1e-9 * np.abs(want["gamma_sums"]).max(), (mode, i)
            if sg:
                assert np.array_equal(got["argmax"], want["argmax"]), (mode, i)
            if passes == fpasses:
                for key, v in got.items():
                    assert np.array_equal(v, want[key]), f"state {i} ({mode}): {key} differs from a fresh manager's with the same passes"
            if prev_ll is not None and i in (1, 3, 5):
                assert abs(ll - prev_ll) >= 1e-3 * abs(prev_ll), (i, ll, prev_ll)
            prev_ll = ll
            seq.append((got, passes))
        del im
        seqs[mode] = seq
    engine_opt("SMCPP_DEBUG_POISON", None)
    for i, ((c, pc), (p, pp)) in enumerate(zip(seqs[None], seqs["nan"])):
        if pc == pp:
            for key, v in c.items():
                assert np.array_equal(p[key], v), f"state {i}: the poisoned sequence differs from the clean one in {key}"
