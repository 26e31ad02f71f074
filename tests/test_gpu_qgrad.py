"""The M-step's objective on the device: Q and dQ/da of `smcpp_q` (smcpp_amd/csrc/prep_dev.hpp: k_prep_tables<DN<4>> /
k_prep_csfs<DN<4>>, k_q_stats, k_q_reduce, driven by smcpp_im::q_device) through the C ABI, against the dense evaluation in
extended precision of tests/qref.py on the host preparation and on the statistics the manager hands out.

The statistics come from the engine (one short E-step per case; only Q's arithmetic on them is under test).  As in an M-step,
`smcpp_set_params` with the case's derivative seeds comes after the E-step and `smcpp_q` before any getter; the statistics are read
afterwards.  Every evaluation asserts the route `smcpp_describe` reports for it ("q_route": device / host): a getter of the
emission table (`im.emission_probs`), a sample size the device preparation refuses, or an E-step that needs eigensystems hands Q to
the host loops of engine_capi.hpp without any other sign.  For that reason the Q checks of tests that read `im.emission_probs`
before `im.Q()` cover the HOST route, not these kernels: in tests/test_gpu_bigm.py test_more_than_256_states_vs_oracle,
test_m512_and_m768_vs_compiled_reference and test_long_rows_of_binned_data_cut_into_pieces; and a manager whose parameters came
through `set_raw` has no device route to take (q_device refuses it).  Their assertions stand; they are not device coverage.

Bars (from the project, tests/test_gpu_prep.py::test_q_gradient_with_device_preparation): each of the four values to 1e-10
relative, each Jacobian row to 1e-9 of its largest entry.  A case that misses evaluates the host route (SMCPP_Q=host with the host
preparation) against the same reference and reports both figures.  Observed on an MI355X when written: no case misses; every
evaluation after an E-step is within 5e-16 on the values and 2e-14 of a Jacobian row, device and host route alike; Q before the
first E-step at (64, 20) shows 1.6e-15 / 1.7e-13, consistent with the 2e-9 relative spread of the emission entries next to the
1e-10 floor that tests/test_gpu_prep.py documents: the statistics of a fresh manager weigh every state by the default model's
initial distribution, the posterior of an E-step puts almost no weight on those entries.  No bar was replaced.

Floors: "the derivative of a floored entry is zero" (T at 1e-20, E at 1e-10).  With synth.hidden_states no entry of T sits on its
floor in any sweep case (the uniform mix keeps T above 1e-5 / (M + 1), the floor acts on the unmixed entry); entries of E do in
the cases with n >= 10 (over every key a sample can show, qref.edge_keys: 2 entries at (32, 10), 63 at (64, 20), 1 368 at (256, 50), 314 at (48, 55), 30 at (1024, 10)):
the keys with many derived alleles at the youngest states.  test_floored_entries makes both floors bind on purpose.
"""
import numpy as np
import pytest

import qref

pytestmark = pytest.mark.gpu

VAL_TOL = 1e-10
JAC_TOL = 1e-9


def _contigs(n, count, rows):
    from smcpp_amd import synth
    return [np.ascontiguousarray(synth.synth_contig(c, 2_000_000, n)[:rows], dtype=np.int32) for c in range(count)]


def _manager(p, contigs):
    """As tests/test_gpu_prep.py::_manager builds them, from a dictionary of tests/qref.py::sweep_inputs."""
    from smcpp_amd import _smcpp
    from smcpp_amd.model import PiecewiseModel
    im = _smcpp.PyOnePopInferenceManager(p["n"], contigs, p["hs"], ("pop1",), p["pol"])
    im.theta = p["theta"]; im.rho = p["rho"]; im.alpha = p["alpha"]
    im.model = PiecewiseModel(p["a"], p["s"], 1e4, pid="pop1")
    return im


def _set_params(im, a, da, s):
    from smcpp_amd import _engine
    a = np.ascontiguousarray(a, dtype=np.float64); s = np.ascontiguousarray(s, dtype=np.float64)
    nder = 0 if da is None else da.shape[1]
    da = None if nder == 0 else np.ascontiguousarray(da, dtype=np.float64)
    _engine.check(_engine.lib().smcpp_set_params(im._im, len(a), _engine.dptr(a), _engine.dptr(da), nder, _engine.dptr(s)))


def _q(im, nder):
    """(val [4], jac [4, nder], route) of one smcpp_q call."""
    from smcpp_amd import _engine
    val = np.full(4, np.nan); jac = np.full((4, max(nder, 1)), np.nan)
    _engine.check(_engine.lib().smcpp_q(im._im, _engine.dptr(val), _engine.dptr(jac) if nder else None))
    return val, jac[:, :nder], im.describe()["q_route"]


def _reference(im, p, a, da):
    """Dense longdouble Q and gradient on this moment's statistics and the host preparation of (a, da) under the manager's
    theta / rho / alpha."""
    da = np.zeros((len(a), 0)) if da is None else da
    return qref.host_reference(p["n"], p["hs"], p["pol"], a, da, p["s"], im.theta, im.rho, im.alpha, im.keys, *qref.manager_statistics(im))


def _host_route_errors(im, p, a, da, ref, rj, engine_opt):
    """The same evaluation by the host loops on the host preparation (SMCPP_Q=host, set_prep_mode(True)); the manager is handed back
    on the device preparation."""
    engine_opt("SMCPP_Q", "host")
    im.set_prep_mode(True)
    _set_params(im, a, da, p["s"])
    hv, hj, route = _q(im, 0 if da is None else da.shape[1])
    engine_opt("SMCPP_Q", None)
    im.set_prep_mode(False)
    assert route == "host"
    return qref.errors(hv, hj, ref, rj)


def _check(tag, im, p, a, da, got, want_route, engine_opt, val_tol=VAL_TOL, jac_tol=JAC_TOL):
    """One evaluation `got` = (val, jac, route) against the dense reference; prints the headroom; returns (ref val, ref jac, prep)."""
    val, jac, route = got
    assert route == want_route, f"{tag}: Q ran on the {route} route, expected {want_route}"
    ref, rj, prep = _reference(im, p, a, da)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(jac)), (tag, val, jac)
    ev, ej = qref.errors(val, jac, ref, rj)
    print(f"{tag}: {route} route vs dense longdouble: values {ev:.3g} (bar {val_tol:g}), Jacobian rows {ej:.3g} (bar {jac_tol:g})")
    if ev > val_tol or ej > jac_tol:
        hv, hj = _host_route_errors(im, p, a, da, ref, rj, engine_opt)
        print(f"{tag}: MISSED; host route vs the same reference: values {hv:.3g}, Jacobian rows {hj:.3g}")
        raise AssertionError(f"{tag}: {route} route values {ev:.3g} / rows {ej:.3g}; host route values {hv:.3g} / rows {hj:.3g}")
    return ref, rj, prep


def _rows(case):
    M, n, contigs = case[:3]
    return 600 if M > 256 else 1000 if contigs > 4 or n > 40 else 2000


@pytest.mark.parametrize("case", qref.SWEEP, ids=qref.sweep_id)
def test_q_gradient_over_the_shape_sweep(case, engine_opt):
    """One case per shape (M, n, contigs, pieces, directions): M != Mp in k_q_stats' three index expressions, several contigs, tail
    groups of the four-direction scalar through k_prep_csfs / k_q_reduce, more directions than pieces, M up to 1024 (k_q_reduce's
    66 560 bytes of dynamic LDS), and the two sample sizes either side of DevPrep::supported: n = 55 must report the device route,
    n = 56 the host route, at the same bars.  Dense standard-normal seeds (identity once); in two cases a zero column whose
    gradient must be exactly 0.0 and two equal columns in different direction groups whose gradients must be equal bit for bit."""
    M, n, ncontig, K, nder = case
    p = qref.sweep_inputs(case)
    im = _manager(p, _contigs(n, ncontig, _rows(case)))
    im.E_step()
    _set_params(im, p["a"], p["da"], p["s"])
    got = _q(im, nder)
    want = "host" if n == 56 else "device"
    ref, rj, _ = _check(qref.sweep_id(case), im, p, p["a"], p["da"], got, want, engine_opt)
    qref.check_marked_columns(case, got[1])
    assert len(im.gamma_sums) == ncontig and im.M == M
    if M > 2:
        assert np.abs(np.asarray(rj, dtype=float)).max() > 1.0          # (a gradient worth the name)


@pytest.mark.parametrize("M,n,ncontig", [(64, 20, 2), (100, 6, 3)])
def test_q_gradient_through_the_call_orders_of_an_m_step(M, n, ncontig, engine_opt):
    """One manager through what an optimiser does to it, every evaluation against the dense reference on that moment's parameters
    and statistics: Q before any E-step; twelve set_params / Q rounds on one set of statistics with the direction count cycling
    through 16, 0, 3, 33, 1 (the staging buffers regrow); theta / rho / alpha through their setters; a getter of the emission
    table between two evaluations (host route, and back to the device after the next set_params); two more E-steps with other
    parameters, save_gamma on for the first and off for the second, after which Q and its gradient must equal, bit for bit, those of a fresh
    manager taken through that last state only (the condition of test_reused_manager_equals_fresh_managers: where both ran the
    same passes) - a Q that still read the first E-step's statistics cannot."""
    from smcpp_amd.model import PiecewiseModel
    case = (M, n, ncontig, 16, 16)
    p = qref.sweep_inputs(case)
    contigs = _contigs(n, ncontig, 2000)
    rng = np.random.default_rng(5)
    a0, s = p["a"], p["s"]
    tag = f"M{M}-n{n}"

    def evaluate(label, im, a, nder, want="device", set_=True):
        da = rng.standard_normal((len(a), nder)) if nder else None
        if set_:
            _set_params(im, a, da, s)
        return da, _check(f"{tag} {label}", im, p, a, da, _q(im, nder), want, engine_opt)

    im = _manager(p, contigs)
    assert im.describe()["q_route"] == "none"
    # 1. before any E-step: the statistics of a freshly constructed HMM, staged from the host
    evaluate("before the first E-step", im, a0, 16)
    # 2. one E-step, many parameters on its statistics
    im.E_step()
    vals = []
    for i, nder in enumerate([16, 0, 3, 33, 1] * 2 + [16, 0]):
        a = a0 * (1.0 + 0.3 * (2.0 * rng.random(len(a0)) - 1.0))
        _, (ref, _, _) = evaluate(f"round {i} nder {nder}", im, a, nder)
        vals.append(float(ref.sum()))
    assert np.ptp(vals) > 1e-6 * abs(vals[0])                            # (the parameters did move Q)
    a, da = a0 * 1.1, rng.standard_normal((16, 5))
    _set_params(im, a, da, s)
    for name, f in (("theta", 1.3), ("rho", 0.7), ("alpha", 0.5)):
        setattr(im, name, getattr(im, name) * f)
        _check(f"{tag} after the {name} setter", im, p, a, da, _q(im, 5), "device", engine_opt)
    # 3. a getter between two evaluations
    assert len(im.emission_probs) == len(im.keys)
    _check(f"{tag} after reading emission_probs", im, p, a, da, _q(im, 5), "host", engine_opt)
    evaluate("after the next set_params", im, a0 * 0.9, 7)
    # 4. further E-steps with other parameters, save_gamma toggled on the way
    a2 = a0[::-1] * 1.5
    im.save_gamma = True
    im.model = PiecewiseModel(a0 * 0.8, s, 1e4, pid="pop1")
    im.E_step()
    im.save_gamma = False
    im.model = PiecewiseModel(a2, s, 1e4, pid="pop1")
    im.E_step()
    da2 = rng.standard_normal((16, 6))
    _set_params(im, a2, da2, s)
    got = _q(im, 6)
    _check(f"{tag} after the third E-step", im, p, a2, da2, got, "device", engine_opt)
    p2 = dict(p, theta=im.theta, rho=im.rho, alpha=im.alpha, a=a2)
    fresh = _manager(p2, contigs)
    fresh.E_step()
    _set_params(fresh, a2, da2, s)
    want = _q(fresh, 6)
    assert want[2] == "device"
    passes = [(int(t["fwd_passes"]), int(t["bwd_passes"])) for t in (im.last_timing(), fresh.last_timing())]
    print(f"{tag} reused against fresh manager: passes {passes}, values {np.max(np.abs(got[0] - want[0]) / np.abs(want[0])):.3g}")
    if passes[0] == passes[1]:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got[:2], want[:2])
    else:
        ev, ej = qref.errors(got[0], got[1], want[0], want[1])
        assert ev <= VAL_TOL and ej <= JAC_TOL, (ev, ej)


def test_q_gradient_after_an_e_step_that_needs_eigensystems(engine_opt):
    """Un-binned rows (spans up to 1e5) make smcpp_im::estep fetch the emission table to the host (eigensystems, hybrid rows), so Q
    straight after that E-step is the host's; the next set_params hands it back to the device kernels, which then read statistics
    that another kernel family wrote into d_gamma0 / d_xisum / d_gsum.  Both routes, in that order, against the dense reference."""
    from smcpp_amd import synth
    case = (64, 8, 1, 16, 6)
    p = qref.sweep_inputs(case)
    obs = np.ascontiguousarray(synth.synth_posterior_contig(20_000, 8), dtype=np.int32)
    im = _manager(p, [obs])
    _set_params(im, p["a"], p["da"], p["s"])
    im.E_step()
    plan = im.describe()["plan"]
    print("plan:", {k: plan[k] for k in ("chain_family", "scan_chains", "hybrid_rows", "eigen_free_statistics", "max_span", "long_rows_cut")})
    _check("un-binned, straight after the E-step", im, p, p["a"], p["da"], _q(im, 6), "host", engine_opt)
    _set_params(im, p["a"] * 1.05, p["da"], p["s"])
    _check("un-binned, after the next set_params", im, p, p["a"] * 1.05, p["da"], _q(im, 6), "device", engine_opt)


def test_floored_entries(engine_opt):
    """Inputs chosen on the CPU so that both floors bind (tests/qref.py::floor_inputs): at least 1 % of the entries of T and at
    least one entry of E have an identically zero row in the HOST Jacobian although no seed column is zero.  That is asserted on the
    host preparation before the device is asked, so the case cannot quietly stop covering floors (measured when written: 6.1 % of
    T, 13 entries of E in 2 of the 27 observed keys, and pi reaches its own 1e-20 floor)."""
    from smcpp_amd import _engine
    case, p = qref.floor_inputs()
    assert np.all(np.abs(p["da"]).max(axis=0) > 0)
    im = _manager(p, _contigs(p["n"], 1, 1000))
    prep = _engine.host_prep_onepop_jac(p["n"], p["hs"], p["pol"], p["a"], p["da"], p["s"], p["theta"], p["rho"], p["alpha"], im.keys)
    zT, zE = qref.floored_entries(prep)
    print(f"floors: {zT.mean():.4f} of T, {int(zE.sum())} entries of E in {int(zE.any(axis=1).sum())} of {len(im.keys)} keys")
    assert zT.mean() >= 0.01 and zE.sum() >= 1
    im.E_step()
    _set_params(im, p["a"], p["da"], p["s"])
    got = _q(im, case[4])
    _check("floors", im, p, p["a"], p["da"], got, "device", engine_opt)
    g0, xi, gs = qref.manager_statistics(im)
    assert float(np.sum(xi[zT])) > 0 or float(np.sum(gs[zE])) > 0        # (floored entries carry weight in this Q)
