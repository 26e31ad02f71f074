"""Long rows of RARE keys: the scan chains' underflow bounds, the E-step that is redone when a device-prepared table passes them,
and the statistics just inside them (inputs and their classes: tests/underflow_cases.py; tests/test_underflow_cases.py pins them
and the reference on the CPU).

The scan chains take a row of span s in s steps without rescaling, so they are refused when s log(min_h E[key][h]) < -450 on a row
they would expand step by step - and, since this file found out why, when s log(max_h E[key][h]) < -80 (below).  WHERE that is
decided depends on where the emission table lives when the E-step starts:
  * on the host (host preparation, set_raw, two populations, or a device table that estep() fetches first because the statistics
    need eigensystems - some row is longer than 64 positions and rows are not cut): ss_extract_generators() evaluates the bounds,
    the E-step runs on the dense kernels at once.  describe(): "scan_chains_refused": "emission underflow", "estep_redone": 0;
  * on the device (one population, eigen-free statistics): k_prep_csfs evaluates the same bounds (DevPrep flag 2; PrepOut::key_ok);
    estep() sees them when the chains and the statistics of the scan attempt have drained, fetches the table and enters itself
    again - on the host route above.  describe(): "estep_redone": 1 and "estep_redone_why".
Beyond 256 states there are no dense kernels: both routes end in a refusal that names the emission entry (not the structure of T).

WHAT THE FIRST RUN FOUND (the bound on the smallest entry alone, as the engine had it).  The rows "just inside the bound" gave NaN:
  near / near64, M = 13, 64 (one state per lane, float scans)    log-likelihood NaN, every statistic NaN
  near, M = 65, 150, 300 (fp64 scans, rows cut)                  log-likelihood finite (-1155.05 at M = 65), every xi entry NaN
The scan steps carry float intermediates (chains_ss.hpp: every scan of the stored passes at one state per lane; the float running
sum of the backward step in every form, which the span fold applies to rows scaled by 1 / c).  The evidence c of a row is at most
max_h(E)^s, so (1,1,8) x 34 (s log max = -108) and (0,1,8) x 100 (-388; -248 per piece of 64) are below float's e^-87 whatever the
data.  The fix is the second bound (prep_dev.hpp: SS_SPAN_LOG_MAX = -80, with its derivation), on both routes; rescaling inside
long rows, which would let the scans take such rows, is out of scope.  So of the three `near` rows only (1,0,0) x 50 (largest
entry: e^-42) runs on the scans (`near_run`), and `near` / `near64` are now refused like `past`.  Without that bound
test_past_the_bound_the_estep_is_redone[near*] and [near64*] fail (NaN), all twelve of them.

THE GUARD ON THE COMPUTED EVIDENCE.  max_h(E)^s bounds a row's evidence c from above only; on these contigs log c lies 2 to 14
below it.  A table bound alone therefore cannot keep NaN out (and any constant between -108 and -42 would have passed the tests
above).  Every scan-chain E-step now checks |log c| <= 80 on each row it expanded step by step, in the log-likelihood kernel
(kernels.hpp: LoglikArgs::range_flag), and is redone on the dense kernels otherwise; the refusal is remembered until the
parameters change.  `edge_run` ((0,1,8) x 19 and x 20: log c -75.8 and -78.0) must run on the scans and match the restatement;
`edge_redo` ((1,1,8) x 24 and x 23: both table bounds pass at -76.3 / -73.1, log c -87 / -88) must be redone - by the guard, on a
device and on a host table - and match it too.  tests/test_underflow_cases.py pins those log c from tests/llref.py, 1.5 away from 80.

Routes taken (asserted by every test before anything is compared; `family` is describe()["estep_chain_family"], the family the
E-step ended on - chain_mode() and plan.chain_family keep the family the manager was planned for, 5 / 6):
  near_run, M = 13, 64      scan chains (5), device table, eigen-free statistics, no redo
  near_run, M = 65, 150     the same with rows cut at 64 positions (a monomorphic run of 100), two / three states per lane
  near_run60, M = 300       the same, eight states per lane
  edge_run, M = 13 .. 150   scan chains (5), device table, no redo (rows cut beyond 64 states)
  edge_redo, M = 13 .. 150  device table: redone by the evidence guard, family 2 / 3; again: refused at once, the same bits; the same
                            manager on the host preparation: scan attempt, guard, redone
  past, near64, M <= 64     device table: redone, family 2; the same manager on the host preparation: family 2, no redo
  past, near, M = 65, 150   device table: redone, family 3; host preparation: family 3, no redo
  deep, near, M = 13, 64    NOT redone: a row above 64 positions brings the table to the host before the chains start, so the host
                            bound fires and the scan attempt is never launched (family 2, "emission underflow").  The issue this
                            file answers expected estep_redone == 1 for `deep`; the code's route is the better one and is asserted
  mixed (chunk 37), past / deep (chunk 20), past M = 150 (chunk 20)    as above, several chunks per contig
  past_one, M = 64          one manager: redone; unchanged: the table is on the host now, refused at once (twice, bit for bit);
                            theta x 5: scans; theta back: redone.  (The issue proposed theta x 20; that sends the MONOMORPHIC runs
                            past the bound on the smallest entry - underflow_cases has the figures - so x 5 it is.)
  hybrid, M = 64            hybrid scan chains (6), no redo: the x 5 000 row is an eigen-power step, the x 6 row is scanned
  twopop:M24                host preparation: the host bound -> family 2, no redo; with the row at span 2: scan chains
  M = 300, past / past_one  RuntimeError naming the emission entry, on the host route and on the device route (after the abandoned
                            scan attempt); the refused manager then runs theta x 5 on the scan chains and equals a fresh one

What the redo path did before any change to estep(): "redone" - on every case of this file, several chunks included.  The
"chunk-boundary iteration did not converge" throw in front of the flag check was not reached: a device table reaches the chains
only when no row is longer than 64 positions (or rows are cut), and there the passes were certified even where the vectors held
NaN (near64 above: one chunk per contig, NaN outputs, no exception).  estep() now looks at the flags before that throw all the
same (run_chains_ss returns false instead of throwing when the preparation flagged its table), so that a table which does break
the iteration is redone and not reported as a convergence failure.  No test reaches that return: it is untested.

Bars: LL_TOL on the log-likelihood, STAT_TOL on the xi sums (conftest.rel_err, per entry), the gamma sums per key (of the key's
largest entry), gammas[:, 0] and Q(separate=True), check_gamma_columns on every column under save_gamma - tests/test_gpu_parity.py's,
unchanged; device against host preparation at tests/test_gpu_prep.py's (log-likelihood 1e-12, xi sums 1e-9 of the largest, Q
1e-10); a reused manager against fresh ones at test_gpu_poison.test_reused_manager_equals_fresh_managers' (1e-10, 1e-9, 1e-9, the
same decoded index).  No statistic needed the wider treatment tests/test_gpu_stats_edges.py documents.  posterior_transitions: stay +
up + down equals the row's SPAN (the product's definition and tests/test_gpu_posterior_transitions.py's bar, 1e-9 relative; the
issue wrote span - 1).

Measured on one MI355X (range over the runs of a kind; every test prints its own; the file takes 7 s):
  against the restatement     log-likelihood   xi sums          gamma sums       gamma_0          Q               (bars 1e-6, 5e-6 x 4)
    near_run (+ 60)           1.4e-9 .. 2.1e-8 3.4e-7 .. 1.9e-6 4.3e-8 .. 1.8e-6 2.0e-9 .. 1.4e-7 1.0e-8 .. 2.4e-8
    past, past_one, mixed     1.4e-9 .. 6.2e-9 3.2e-7 .. 2.0e-6 1.0e-7 .. 1.8e-6 5.4e-11 .. 1.4e-7 2.5e-9 .. 3.3e-8
    near, near64 (refused)    8.9e-10 .. 3.2e-9 2.1e-7 .. 1.2e-6 1.1e-7 .. 9.3e-7 3.4e-11 .. 1.5e-10 6.4e-9 .. 1.9e-8
    deep                      4.4e-10 .. 6.5e-10 4.2e-7 .. 1.2e-6 1.6e-7 .. 1.4e-6 3.0e-12 .. 3.5e-11 6.0e-10 .. 1.0e-8
    hybrid / twopop:M24       1.5e-10 / 5.4e-8 1.1e-6 / 6.4e-7  6.0e-7 / 4.2e-7  2.8e-10 / 2.7e-11 2.8e-9 / 9.3e-9
    edge_run (scans)          1.5e-9 .. 1.2e-8 4.2e-7 .. 2.5e-6 1.5e-7 .. 1.4e-6 5.4e-9 .. 9.7e-8 9.6e-9 .. 6.2e-8
    edge_redo (M = 13, 64)    4.0e-10 .. 4.5e-9 3.0e-7 .. 1.1e-6 1.2e-7 .. 7.2e-7 1.3e-11 .. 5.2e-11 3.5e-9 .. 1.2e-8
  per-row posteriors (47 contig runs): worst column 4.5e-7 of its span (bar 2e-5), column sums 1.2e-15 (1e-9), large entries 2.6e-6 (1e-4)
  device against host preparation (28 pairs): log-likelihood 5.4e-15 (bar 1e-12), xi sums 8.3e-11 (1e-9), Q 3.4e-11 (1e-10)
  reused against fresh managers (5 states + M = 300): identical in every bit where compared at 1e-10 / 1e-9
  products after the redo: rows and windows 0.35 of 4 x the reference's own noise (rows 3.8e-7 against 1.08e-6); stay + up + down
    against the span 2.2e-16 (bar 1e-9)
"""
import numpy as np
import pytest

import underflow_cases as U
from conftest import rel_err
from test_gpu_gamma import _onepop, _twopop
from test_gpu_parity import GAMMA_SUM_RTOL, LL_TOL, STAT_TOL, check_gamma_columns, oracle_estep

pytestmark = pytest.mark.gpu

WHY = "too small"                       # in estep_redone_why and in the refusal beyond 256 states
DENSE = {True: 2, False: 3}             # the dense family by M <= 64


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _manager(name, M, host=False, chunk=0, save_gamma=False, theta_scale=1.0):
    cs = U.case(name, M)
    im = _onepop(M, cs["contigs"], cs["theta"] * theta_scale, cs["rho"])
    if host:
        im.set_prep_mode(True)
    if chunk:
        im.set_chunking(chunk)
    im.save_gamma = save_gamma
    return im, cs["contigs"]


def _route(im):
    d = im.describe()
    p, q = d["plan"], d["parameters"]
    return dict(chain_mode=im.chain_mode(), scan_chains=p["scan_chains"], states_per_lane=p["states_per_lane"],
                long_rows_cut=p["long_rows_cut"], source=q["source"], table=q["emission_table"], eigfree=p["eigen_free_statistics"],
                redone=d["estep_redone"], why=d["estep_redone_why"], family=d["estep_chain_family"], refused=d["scan_chains_refused"],
                chunks=(p["chunks_forward"], p["chunks_backward"]), hybrid=p["hybrid_rows"])


def _assert_route(im, label, **want):
    got = _route(im)
    print(f"{label}: route {got}")
    for k, v in want.items():
        assert got[k] == v, (label, k, got[k], v, got)
    assert (WHY in got["why"]) == (got["redone"] == 1), (label, got)
    return got


def _outputs(im):
    nc = len(im.logliks())
    gs = im.gamma_sums
    out = dict(ll=np.array(im.logliks()), xis=[np.array(x) for x in im.xisums], gs=[dict(g) for g in gs],
               q=np.array(im.Q(separate=True)), gam=[np.array(g) for g in im.gammas])
    if im.save_gamma:
        out["argmax"] = [np.asarray(im.gamma_argmax(c)).copy() for c in range(nc)]
    return out


def _flat(out):
    """The arrays of `_outputs` in one fixed order (bit-for-bit comparisons)."""
    v = [out["ll"], out["q"]] + out["xis"] + out["gam"] + [g[k] for g in out["gs"] for k in sorted(g)] + out.get("argmax", [])
    return [np.asarray(x) for x in v]


def _check_restatement(im, contigs, label, out=None):
    """Every statistic of the last E-step against the C restatement fed with the manager's own pi, T and emission table; -> worst."""
    out = _outputs(im) if out is None else out
    keys = im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    pi, T = im.pi, im.transition
    sg = im.save_gamma
    worst = dict(ll=0.0, xi=0.0, gs=0.0, g0=0.0, q=0.0)
    qsum = np.zeros(4)
    checks = []
    for c, ob in enumerate(contigs):
        o = oracle_estep(pi, T, keys, Etab, ob, save_gamma=sg)
        xs, gs, gam = out["xis"][c], out["gs"][c], out["gam"][c]
        assert np.isfinite(out["ll"][c]) and np.all(np.isfinite(xs)) and np.all(np.isfinite(gam)), (label, c)
        assert sorted(gs) == sorted(o["gamma_sums"]), (label, c)
        d = dict(ll=abs(out["ll"][c] - o["loglik"]) / max(1.0, abs(o["loglik"])), xi=rel_err(xs, o["xisum"]),
                 gs=max(float(np.max(np.abs(gs[k] - v)) / max(np.abs(v).max(), 1e-300)) for k, v in o["gamma_sums"].items()),
                 g0=rel_err(gam[:, 0], o["gamma"][:, 0]))
        for k, v in d.items():
            worst[k] = max(worst[k], v)
        qsum += o["q"]
        checks.append((c, ob, o))
    q = out["q"]
    assert np.all(np.isfinite(q)), (label, q)
    worst["q"] = float(np.max(np.abs(q - qsum) / np.maximum(np.abs(qsum), 1e-12)))
    print(f"{label}: against the restatement: log-likelihood {worst['ll']:.2e} (bar {LL_TOL:g}), xi sums {worst['xi']:.2e}, gamma sums "
          f"{worst['gs']:.2e}, gamma_0 {worst['g0']:.2e}, Q {worst['q']:.2e} (bar {STAT_TOL:g})")
    assert worst["ll"] <= LL_TOL, (label, worst)
    for k in ("xi", "gs", "g0", "q"):
        assert worst[k] <= STAT_TOL, (label, k, worst)
    if sg:
        for c, ob, o in checks:
            assert out["gam"][c].shape == (im.M, len(ob) + 1), (label, c)
            check_gamma_columns(out["gam"][c], o["gamma"], ob, arg_dev=out["argmax"][c], label=f"{label}, contig {c}")
    return worst


def _check_device_against_host(dev, host, label):
    """tests/test_gpu_prep.py's bars between a device and a host preparation."""
    dl = float(np.max(np.abs(dev["ll"] - host["ll"]) / np.abs(host["ll"])))
    dx = max(float(np.max(np.abs(a - b)) / np.abs(b).max()) for a, b in zip(dev["xis"], host["xis"]))
    nz = host["q"] != 0.0                                  # (a term that is zero on both sides, as test_gpu_prep's <= takes it)
    assert np.array_equal(dev["q"][~nz], host["q"][~nz]), (label, dev["q"], host["q"])
    dq = float(np.max(np.abs(dev["q"] - host["q"])[nz] / np.abs(host["q"])[nz]))
    print(f"{label}: device against host preparation: log-likelihood {dl:.2e} (bar 1e-12), xi sums {dx:.2e} (1e-9), Q {dq:.2e} (1e-10)")
    assert dl <= 1e-12 and dx <= 1e-9 and dq <= 1e-10, (label, dl, dx, dq)


def _check_reused_against_fresh(got, want, label):
    """test_gpu_poison.test_reused_manager_equals_fresh_managers' bars."""
    ll, llf = got["ll"].sum(), want["ll"].sum()
    dx = max(rel_err(a, b) for a, b in zip(got["xis"], want["xis"]))
    ga = np.array([g[k] for g in got["gs"] for k in sorted(g)])
    gb = np.array([g[k] for g in want["gs"] for k in sorted(g)])
    dg = float(np.max(np.abs(ga - gb)) / np.abs(gb).max())
    print(f"{label}: reused against fresh manager: log-likelihood {abs(ll - llf) / abs(llf):.2e} (bar 1e-10), xi sums {dx:.2e} (1e-9), "
          f"gamma sums {dg:.2e} (1e-9)")
    assert all(np.all(np.isfinite(x)) for x in _flat(got)), label
    assert abs(ll - llf) <= 1e-10 * abs(llf), (label, ll, llf)
    assert dx <= 1e-9 and dg <= 1e-9, (label, dx, dg)
    if "argmax" in got:
        assert all(np.array_equal(a, b) for a, b in zip(got["argmax"], want["argmax"])), label


def _same_bits(a, b, label):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and np.array_equal(x, y), f"{label}: array {i} differs in {int(np.sum(x != y))} entries"


def _past_or_deep(name, M, chunk, save_gamma, label):
    """Item 2 / 3: the device preparation (redone where the table is still on the device when the chains start: no row above 64
    positions, or rows cut; else the host bound at once), the host preparation, both against the restatement and against each other."""
    nc = len(U.case(name, M)["contigs"])
    longest = max(int(c[:, 0].max()) for c in U.case(name, M)["contigs"])
    im, contigs = _manager(name, M, chunk=chunk, save_gamma=save_gamma)
    im.E_step()
    redo = M > 64 or longest <= 64
    assert redo == (name not in ("deep", "near") or M > 64)
    r = _assert_route(im, label + ", device preparation", chain_mode=5, scan_chains=True, states_per_lane=(M + 63) // 64,
                      long_rows_cut=M > 64 and longest > 64, source="ONEPOP_DEVICE", redone=1 if redo else 0, family=DENSE[M <= 64],
                      refused="emission underflow", table="host", eigfree=False)
    if chunk:
        assert r["chunks"][0] > nc and r["chunks"][1] > nc, (label, r)
    dev = _outputs(im)
    _check_restatement(im, contigs, label + ", device preparation", dev)
    # the SAME manager on the host preparation (its table already fetched by the redo): the dense kernels with no redo
    im.set_prep_mode(True)
    im.E_step()
    _assert_route(im, label + ", host preparation", chain_mode=5, scan_chains=True, source="ONEPOP_HOST", redone=0, family=DENSE[M <= 64],
                  refused="emission underflow", table="host", eigfree=False)
    host = _outputs(im)
    _check_restatement(im, contigs, label + ", host preparation", host)
    del im
    _check_device_against_host(dev, host, label)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. just inside the bound: the scans run
# ---------------------------------------------------------------------------------------------------------------------------------
NEAR = [("near_run", 13), ("near_run", 64), ("near_run", 65), ("near_run", 150),
        # just inside the guard on the evidence of a scanned row (log c -75.8, -78.0 against 80)
        ("edge_run", 13), ("edge_run", 64), ("edge_run", 65), ("edge_run", 150)]


@pytest.mark.parametrize("save_gamma", [False, True], ids=["lean", "save_gamma"])
@pytest.mark.parametrize("name,M", NEAR, ids=[f"{n}:M{M}" for n, M in NEAR])
def test_near_the_bound_the_scans_run(name, M, save_gamma):
    label = f"{name}, M = {M}, save_gamma {int(save_gamma)}"
    im, contigs = _manager(name, M, save_gamma=save_gamma)
    im.E_step()
    _assert_route(im, label, chain_mode=5, scan_chains=True, states_per_lane=(M + 63) // 64, long_rows_cut=M > 64,
                  source="ONEPOP_DEVICE", redone=0, family=5, refused="", eigfree=True, table="device")
    _check_restatement(im, contigs, label)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2., 3. past the bound: redone (or refused on the host at once), one and several chunks
# ---------------------------------------------------------------------------------------------------------------------------------
PAST = [("past", 13), ("past", 64), ("past", 65), ("past", 150), ("deep", 13), ("deep", 64),
        # inside the bound on the smallest entry, past the one on the largest (underflow_cases: near_small, cut_small)
        ("near", 13), ("near64", 13), ("near", 64), ("near64", 64), ("near", 65), ("near", 150)]


@pytest.mark.parametrize("save_gamma", [False, True], ids=["lean", "save_gamma"])
@pytest.mark.parametrize("name,M", PAST, ids=[f"{n}:M{M}" for n, M in PAST])
def test_past_the_bound_the_estep_is_redone(name, M, save_gamma):
    _past_or_deep(name, M, 0, save_gamma, f"{name}, M = {M}, save_gamma {int(save_gamma)}")


CHUNKED = [("deep", 64, 20), ("past", 64, 20), ("mixed", 64, 37), ("past", 150, 20)]


@pytest.mark.parametrize("name,M,chunk", CHUNKED, ids=[f"{n}:M{M}:chunk{c}" for n, M, c in CHUNKED])
def test_past_the_bound_on_several_chunks(name, M, chunk):
    """Where "chunk-boundary iteration did not converge" would fire in front of the redo."""
    _past_or_deep(name, M, chunk, True, f"{name}, M = {M}, chunks of {chunk} rows, save_gamma 1")


EDGE = [13, 64, 65, 150]


@pytest.mark.parametrize("save_gamma", [False, True], ids=["lean", "save_gamma"])
@pytest.mark.parametrize("M", EDGE)
def test_evidence_past_the_float_range_is_redone(M, save_gamma):
    """edge_redo: both table bounds pass (span x log max E = -76.3, -73.1), the rows' evidence is e^-87 and e^-88: the guard on what
    the scans computed (kernels.hpp: LoglikArgs::range_flag) sends the E-step to the dense kernels, on a device and on a host table;
    a second E-step on the same parameters goes there at once."""
    label = f"edge_redo, M = {M}, save_gamma {int(save_gamma)}"
    im, contigs = _manager("edge_redo", M, save_gamma=save_gamma)
    im.E_step()
    r = _assert_route(im, label + ", device preparation", chain_mode=5, scan_chains=True, states_per_lane=(M + 63) // 64,
                      long_rows_cut=M > 64, source="ONEPOP_DEVICE", redone=1, family=DENSE[M <= 64], refused="emission underflow",
                      table="host", eigfree=False)
    assert "evidence" in r["why"], r
    dev = _outputs(im)
    _check_restatement(im, contigs, label + ", device preparation", dev)
    im.E_step()
    _assert_route(im, label + ", same parameters again", redone=0, family=DENSE[M <= 64], refused="emission underflow", table="host")
    _same_bits(dev, _outputs(im), label + ", second E-step against the redone one")
    im.set_prep_mode(True)
    im.E_step()
    r = _assert_route(im, label + ", host preparation", source="ONEPOP_HOST", redone=1, family=DENSE[M <= 64], refused="emission underflow")
    assert "evidence" in r["why"], r
    host = _outputs(im)
    _check_restatement(im, contigs, label + ", host preparation", host)
    _check_device_against_host(dev, host, label)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. one manager across the bound and back
# ---------------------------------------------------------------------------------------------------------------------------------
def test_manager_that_crosses_the_bound():
    M, label = 64, "past_one, M = 64, one manager"
    cs = U.case("past_one", M)
    th0, th1 = cs["theta"], U.CROSS * cs["theta"]
    for th, side in ((th0, True), (th1, False)):
        _, _, keys, E = U.host_table(M, cs["contigs"], th, cs["rho"])
        vals = [lo for _, lo, _ in U.bound(E, keys, cs["contigs"][0], U.cut_for(M))]
        assert len(vals) == 1 and all((v < U.BOUND - U.MARGIN) == side and (v > U.BOUND + U.MARGIN) == (not side) for v in vals), (th, vals)

    def fresh(scale):
        f, _ = _manager("past_one", M, save_gamma=True, theta_scale=scale)
        f.E_step()
        o, r = _outputs(f), _route(f)
        del f
        return o, r
    want0, r0 = fresh(1.0)
    want1, r1 = fresh(U.CROSS)
    assert r0["redone"] == 1 and r1["redone"] == 0 and r1["family"] == 5, (r0, r1)
    im, contigs = _manager("past_one", M, save_gamma=True)
    im.E_step()
    _assert_route(im, label + ", first E-step", redone=1, family=2, refused="emission underflow", source="ONEPOP_DEVICE")
    first = _outputs(im)
    _check_reused_against_fresh(first, want0, label + ", first E-step")
    # nothing changed: the table stays on the host, where the host bound refuses the scan chains at once
    im.E_step()
    _assert_route(im, label + ", second E-step", redone=0, family=2, refused="emission underflow", table="host")
    second = _outputs(im)
    _check_reused_against_fresh(second, want0, label + ", second E-step")
    im.E_step()
    _assert_route(im, label + ", third E-step", redone=0, family=2, refused="emission underflow", table="host")
    _same_bits(second, _outputs(im), label + ", second against third E-step")
    im.theta = th1
    im.E_step()
    _assert_route(im, label + ", theta x 5", redone=0, family=5, refused="", table="device", eigfree=True)
    moved = _outputs(im)
    _check_reused_against_fresh(moved, want1, label + ", theta x 5")
    _check_restatement(im, contigs, label + ", theta x 5", moved)
    assert abs(moved["ll"].sum() - first["ll"].sum()) >= 1e-3 * abs(first["ll"].sum())
    im.theta = th0
    im.E_step()
    _assert_route(im, label + ", theta back", redone=1, family=2, refused="emission underflow", source="ONEPOP_DEVICE")
    back = _outputs(im)
    _check_reused_against_fresh(back, want0, label + ", theta back")
    _check_restatement(im, contigs, label + ", theta back", back)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the redo reads nothing the abandoned attempt left behind
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = [("past", 64, 20, True), ("deep", 64, 0, False)]


@pytest.mark.parametrize("name,M,chunk,save_gamma", POISON, ids=[f"{n}:M{M}:chunk{c}" for n, M, c, _ in POISON])
def test_redo_on_poisoned_memory(engine_opt, name, M, chunk, save_gamma):
    from test_gpu_poison import _clean_and_poisoned
    label = f"{name}, M = {M}, chunks of {chunk}, poison"
    contigs = U.case(name, M)["contigs"]
    routes = []

    def build():
        im, _ = _manager(name, M, chunk=chunk)
        return im

    def check(im):
        # (after the two E-steps of test_gpu_poison._outputs: the second finds the table on the host)
        routes.append(_assert_route(im, label, family=2, refused="emission underflow", redone=0))
        _check_restatement(im, contigs, label)
    _clean_and_poisoned(engine_opt, build, check, save_gamma)
    # ... and the FIRST E-step of a poisoned manager alone (the redone one for `past`) against a clean one, bit for bit
    outs = {}
    for mode in (None, "nan"):
        engine_opt("SMCPP_DEBUG_POISON", mode)
        im, _ = _manager(name, M, chunk=chunk, save_gamma=save_gamma)
        im.E_step()
        _assert_route(im, label + f", first E-step, poison {mode}", redone=1 if name == "past" else 0, family=2)
        outs[mode] = _outputs(im)
        del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    assert all(np.all(np.isfinite(x)) for x in _flat(outs["nan"])), label
    _same_bits(outs["nan"], outs[None], label + ", first E-step, poisoned against clean")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the products after a redone E-step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_products_after_a_redone_estep():
    import test_gpu_loglik_track as LT
    M, label = 64, "past, M = 64, products after the redo"
    im, contigs = _manager("past", M, save_gamma=True)
    im.E_step()
    _assert_route(im, label, redone=1, family=2)
    for c, ob in enumerate(contigs):
        # rows sum to logliks()[c] (fp), windows == differences of the positions bit for bit (W = 7 among them), signs
        assert 7 in LT.WIDTHS
        LT.check_identities(im, c, ob, f"{label}, contig {c}")
    worst = LT.check_against_llref("underflow:past:M64", im, contigs)
    print(f"{label}: rows and windows against llref: {worst:.3f} of 4 x the reference's own noise")
    assert worst <= 1.0, worst
    for c, ob in enumerate(contigs):
        t = im.posterior_transitions(c)
        spans = np.concatenate([[0.0], ob[:, 0].astype(float)])
        tot = t["stay"] + t["up"] + t["down"]
        assert all(v.shape == (len(ob) + 1,) and np.all(np.isfinite(v)) and np.all(v >= 0.0) for v in t.values()), label
        assert tot[0] == 0.0
        d = float(np.max(np.abs(tot[1:] - spans[1:]) / spans[1:]))
        print(f"{label}, contig {c}: stay + up + down against the span {d:.2e} (bar {GAMMA_SUM_RTOL:g})")
        assert d <= GAMMA_SUM_RTOL, (label, c, d)
        # a span-1 row holds one position
        assert np.all(np.abs(tot[1:][ob[:, 0] == 1] - 1.0) <= GAMMA_SUM_RTOL)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the rows the bound exempts; the host bound of a two-population manager
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("save_gamma", [False, True], ids=["lean", "save_gamma"])
def test_hybrid_rows_are_exempt(save_gamma):
    label = f"hybrid, M = 64, save_gamma {int(save_gamma)}"
    im, contigs = _manager("hybrid", 64, save_gamma=save_gamma)
    im.E_step()
    _assert_route(im, label, chain_mode=6, scan_chains=True, hybrid=True, states_per_lane=1, long_rows_cut=False, source="ONEPOP_DEVICE",
                  redone=0, family=6, refused="")
    _check_restatement(im, contigs, label)


@pytest.mark.parametrize("save_gamma", [False, True], ids=["lean", "save_gamma"])
def test_two_populations_take_the_host_bound(save_gamma):
    tp = U.twopop_case()
    label = f"twopop:M{U.TWOPOP_M}, key {tp['key']} x {tp['span']}, save_gamma {int(save_gamma)}"
    assert tp["value"] < U.BOUND - U.MARGIN
    im = _twopop(U.TWOPOP_M, tp["contigs"])
    im.save_gamma = save_gamma
    im.E_step()
    r = _assert_route(im, label, chain_mode=5, scan_chains=True, states_per_lane=1, long_rows_cut=False, redone=0, family=2,
                      refused="emission underflow", table="host")
    assert r["source"].startswith("TWOPOP"), r
    _check_restatement(im, tp["contigs"], label)
    # the same contigs without the long row keep the scan chains
    plain = [c.copy() for c in tp["contigs"]]
    plain[0][tp["special"][0][1], 0] = 2
    im = _twopop(U.TWOPOP_M, plain)
    im.E_step()
    _assert_route(im, label + ", the row at span 2", redone=0, family=5, refused="")


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. beyond 256 states: the refusal names its cause
# ---------------------------------------------------------------------------------------------------------------------------------
def test_beyond_256_states_the_refusal_names_the_emission_entry():
    M = 300
    structure = "must have the structure"
    ims = {}
    for host in (True, False):
        im, _ = _manager("past" if host else "past_one", M, host=host)
        ims[host] = im
        with pytest.raises(RuntimeError, match="emission entry is too small") as e:
            im.E_step()
        assert structure not in str(e.value) and "more than 256 hidden states" in str(e.value), str(e.value)
        d = im.describe()
        print(f"past, M = 300, {'host' if host else 'device'} preparation: refused ({str(e.value)[:60]}...), estep_redone {d['estep_redone']}")
        assert d["estep_redone"] == (0 if host else 1), d
        assert d["parameters"]["source"] == ("ONEPOP_HOST" if host else "ONEPOP_DEVICE"), d["parameters"]
    # the manager of the device route is still usable: theta x 5 leaves the bound, and it equals a fresh manager there
    im = ims[False]
    del ims
    cs = U.case("past_one", M)
    im.theta = U.CROSS * cs["theta"]
    im.E_step()
    _assert_route(im, "past, M = 300, theta x 5 after the refusal", redone=0, family=5, refused="", states_per_lane=8, eigfree=True)
    got = _outputs(im)
    del im
    f, _ = _manager("past_one", M, theta_scale=U.CROSS)
    f.E_step()
    _check_reused_against_fresh(got, _outputs(f), "past, M = 300, theta x 5 after the refusal")
    del f


def test_near_the_bound_at_300_states():
    """tests/test_gpu_bigm.py's bars (LL_TOL, STAT_TOL up to 512 states) on 60 rows."""
    M, label = 300, "near_run60, M = 300"
    im, contigs = _manager("near_run60", M)
    im.E_step()
    _assert_route(im, label, chain_mode=5, scan_chains=True, states_per_lane=8, long_rows_cut=True, source="ONEPOP_DEVICE", redone=0,
                  family=5, refused="", eigfree=True, table="device")
    _check_restatement(im, contigs, label)
