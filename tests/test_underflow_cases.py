"""tests/underflow_cases.py pinned on the CPU: the cases lie where tests/test_gpu_underflow.py needs them against the scan chains'
underflow bound (span x log(min_h E) < -450), and the C restatement (oracle/) is as good a reference on long rows of rare keys as
everywhere else.

Per M in {13, 64, 65, 150, 300}, on the host preparation:
  * every `near` row lies in [-445, -400], every `past` row below -455, every `deep` row below -455 with span x log(max_h E) < -750
    as well; the (0,1,8) x 100 row stays above -400 per piece beyond 64 states.  The margin of 5 around -450 keeps a last-bit
    difference between the device and host tables from moving a case across the bound;
  * against the bound on the LARGEST entry (-80, prep_dev.hpp): span x log(max_h E) is above -75 on the rows the scans are to take
    ("near", the monomorphic runs, the scanned hybrid row, past_one at theta x 5) and below -85 on "near_small" / "cut_small";
  * the edge rows pass both table bounds, and their evidence from llref.rows is inside 78.5 (edge_run) / outside 81.5 (edge_redo):
    the engine's guard on the computed evidence of a scanned row is |log c| <= 80; no other row of those contigs is outside 78.5;
  * the restatement is finite on every case, its gamma columns sum to their spans (GAMMA_SUM_RTOL = 1e-9);
  * its log-likelihood is within 5e-8 relative of tests/llref.track (float64, every position normalised): seven times the worst
    value on the same contig without special rows (7.1e-9) and well inside LL_TOL = 1e-6.

Measured (printed by the tests): relative difference of the restatement's log-likelihood from llref.track, worst over the cases
of a state count: M = 13 4.6e-10, M = 64 2.2e-9, M = 65 3.7e-9, M = 150 1.4e-8, M = 300 3.0e-8 (`mixed`; bar 5e-8); gamma column
sums against the span 3.1e-15 at worst (bar 1e-9).  (1,1,8) has span 34 in `near`, not 35 as first proposed: log min E is -12.73,
and 35 positions give -445.5, outside the stated range.
"""
import numpy as np
import pytest

import llref
import underflow_cases as U
from oracle import oracle

MS = (13, 64, 65, 150, 300)
GAMMA_SUM_RTOL = 1e-9        # (test_gpu_parity.GAMMA_SUM_RTOL; that module is GPU-only)
LL_REF_TOL = 5e-8


def _names(M):
    return ("near", "near64", "near_run", "past", "deep", "mixed") if M <= U.CUT else \
        ("near", "near_run", "past", "mixed") + (("near_run60",) if M == 300 else ())


@pytest.mark.parametrize("M", MS)
def test_cases_keep_their_side_of_the_bound(M):
    seen = set()
    for name in _names(M):
        cs = U.case(name, M)
        _, _, keys, E = U.host_table(M, cs["contigs"], cs["theta"], cs["rho"])
        per = {}
        for c, ob in enumerate(cs["contigs"]):
            for r, lo, hi in U.bound(E, keys, ob, U.cut_for(M)):
                per[(c, r)] = (lo, hi)
        assert sorted(per) == sorted((c, r) for c, r, *_ in cs["special"]), (name, sorted(per), cs["special"])
        for c, r, key, span, cls in cs["special"]:
            lo, hi = per[(c, r)]
            ob = cs["contigs"][c]
            assert tuple(ob[r]) == (span, *key)
            # never adjacent to another long row
            assert (r == 0 or ob[r - 1, 0] == 1) and (r == len(ob) - 1 or ob[r + 1, 0] == 1)
            print(f"M = {M}, {name}: contig {c} row {r} {key} x {span} ({cls}): span x log min {lo:.1f}, span x log max {hi:.1f}")
            if cls == "near":
                assert -445.0 <= lo <= -400.0 and hi > U.LARGE, (M, name, key, span, lo, hi)
            elif cls == "near_small":
                assert -445.0 <= lo <= -400.0 and hi < U.SMALL, (M, name, key, span, lo, hi)
            elif cls == "past":
                assert lo < U.BOUND - U.MARGIN and hi > -750.0, (M, name, key, span, lo, hi)
            elif cls == "deep":
                assert lo < U.BOUND - U.MARGIN and hi < -750.0, (M, name, key, span, lo, hi)
            else:
                assert cls == "cut_small" and M > U.CUT and lo > -400.0 and hi < U.SMALL, (M, name, key, span, lo, hi)
            seen.add(cls)
        # every other long row of the one-population contigs is a monomorphic run of at most 59 positions
        for ob in cs["contigs"]:
            other = np.setdiff1d(np.nonzero(ob[:, 0] > 1)[0], U.special_rows(ob))
            assert np.all(ob[other, 0] <= 100) and np.sum(ob[other, 0] >= 60) <= 1 and np.all(ob[other, 1:] == np.array(U.MONO))
            assert np.all(U.bound_of_key(E, keys, U.MONO, ob[other, 0].max(initial=1))[1] > U.LARGE)
            assert len(ob) == 1 or (ob[0, 0] == 1 and ob[-1, 0] == 1)
    assert seen == ({"near", "near_small", "past", "deep"} if M <= U.CUT else {"near", "near_small", "past", "cut_small"})


def test_crossing_the_bound_with_theta():
    """The crossing manager of test_gpu_underflow runs `past_one` at theta x 5 (underflow_cases.CROSS): the (1,0,0) x 64 row and the
    monomorphic runs are inside both bounds there, outside at theta x 1 (the row) and at theta x 20 (the runs).  `past` itself
    cannot cross: at theta x 20 both its rows leave the bound on the smallest entry, but (1,1,8) x 40 stays past the one on the
    largest entry."""
    cs = U.case("past", 64)
    _, _, keys, E = U.host_table(64, cs["contigs"], 20.0 * cs["theta"], cs["rho"])
    got = U.bound(E, keys, cs["contigs"][0], U.cut_for(64))
    print(f"past at theta x 20: {[(r, round(lo, 1), round(hi, 1)) for r, lo, hi in got]}")
    assert len(got) == 2 and all(lo > U.BOUND + U.MARGIN for _, lo, _ in got), got
    assert got[0][2] > U.LARGE and got[1][2] < U.SMALL, got
    one = U.case("past_one", 64)
    ob = one["contigs"][0]
    longest_run = int(ob[np.all(ob[:, 1:] == np.array(U.MONO), axis=1), 0].max())
    for M in (64, 300):
        for scale, inside in ((1.0, False), (U.CROSS, True), (20.0, False)):
            _, _, keys, E = U.host_table(M, one["contigs"], scale * one["theta"], one["rho"])
            (_, lo, hi), = U.bound(E, keys, ob, U.cut_for(M))
            mlo, mhi = (float(v[0]) for v in U.bound_of_key(E, keys, U.MONO, longest_run))
            print(f"past_one, M = {M}, theta x {scale:g}: (1,0,0) x 64 {lo:.1f} / {hi:.1f}, monomorphic x {longest_run} {mlo:.1f} / {mhi:.1f}")
            ok = min(lo, mlo) > U.BOUND + U.MARGIN and min(hi, mhi) > U.LARGE
            assert ok == inside and (inside or min(lo, mlo) < U.BOUND - U.MARGIN), (M, scale, lo, hi, mlo, mhi)


def test_hybrid_and_twopop_cases():
    cs = U.case("hybrid", 64)
    ob = cs["contigs"][0]
    _, _, keys, E = U.host_table(64, cs["contigs"], cs["theta"], cs["rho"])
    by_row = {r: lo for r, lo, _ in U.bound(E, keys, ob, 1 << 30)}
    (_, r_pow, _, s_pow, _), (_, r_scan, _, s_scan, _) = cs["special"]
    mono = ob[np.all(ob[:, 1:] == np.array(U.MONO), axis=1), 0]
    assert mono.max() > 512 and s_pow == 5000 and s_scan == 6           # the hybrid plan; threshold 6: the second row is scanned
    assert by_row[r_pow] < U.BOUND - U.MARGIN                           # (exempt: an eigen-power step)
    assert by_row[r_scan] > -100.0 and {r: hi for r, _, hi in U.bound(E, keys, ob, 1 << 30)}[r_scan] > U.LARGE
    print(f"hybrid: (1,0,0) x 5000 {by_row[r_pow]:.0f} (exempt), x 6 {by_row[r_scan]:.1f}")
    tp = U.twopop_case()
    _, _, keys, E = U.twopop_host_table(U.TWOPOP_M, tp["contigs"])
    got = {r: lo for r, lo, _ in U.bound(E, keys, tp["contigs"][0], 1 << 30)}
    at = tp["special"][0][1]
    print(f"twopop:M{U.TWOPOP_M}: key {tp['key']} x {tp['span']}: {got[at]:.1f}; the other long rows of rare keys: "
          f"{[round(v, 1) for r, v in got.items() if r != at]}")
    assert got[at] < U.BOUND - U.MARGIN and tp["span"] <= 64
    assert all(v > -400.0 for r, v in got.items() if r != at)
    assert all(len(U.special_rows(c)) == 0 for c in tp["contigs"][1:])


@pytest.mark.parametrize("M", (13, 64, 65, 150))
def test_edge_rows_and_their_evidence(M):
    for name in ("edge_run", "edge_redo"):
        cs = U.case(name, M)
        ob = cs["contigs"][0]
        pi, T, keys, E = U.host_table(M, cs["contigs"], cs["theta"], cs["rho"])
        logc = llref.rows(llref.track(pi, T, keys, E, ob), ob)[1:]
        per = {r: (lo, hi) for r, lo, hi in U.bound(E, keys, ob, U.cut_for(M))}
        assert (ob[:, 0].max() == 100) == (M > U.CUT)
        special = [r for _, r, *_ in cs["special"]]
        for _, r, key, span, cls in cs["special"]:
            lo, hi = per[r]
            print(f"M = {M}, {name}: {key} x {span}: span x log min {lo:.1f}, span x log max {hi:.1f}, log c {logc[r]:.2f}")
            assert lo > U.BOUND + U.MARGIN and hi >= -80.0 + 1.0, (M, name, key, span, lo, hi)          # both table bounds pass
            if cls == "edge_run":
                assert abs(logc[r]) < U.EVIDENCE - U.EVIDENCE_MARGIN, (M, key, span, logc[r])
            else:
                assert cls == "edge_redo" and abs(logc[r]) > U.EVIDENCE + U.EVIDENCE_MARGIN, (M, key, span, logc[r])
        others = np.setdiff1d(np.arange(len(ob)), special)
        assert np.all(np.abs(logc[others]) < U.EVIDENCE - U.EVIDENCE_MARGIN)


def _restatement(M, name):
    cs = U.case(name, M)
    pi, T, keys, E = U.host_table(M, cs["contigs"], cs["theta"], cs["rho"])
    worst_ll = worst_sum = 0.0
    for c, ob in enumerate(cs["contigs"]):
        o = oracle.estep(pi, T, keys, E, ob, save_gamma=True)
        assert np.isfinite(o["loglik"]) and np.all(np.isfinite(o["xisum"])) and np.all(np.isfinite(o["gamma"])), (M, name, c)
        assert all(np.all(np.isfinite(v)) for v in o["gamma_sums"].values())
        spans = ob[:, 0].astype(float)
        worst_sum = max(worst_sum, float(np.max(np.abs(o["gamma"][:, 1:].sum(axis=0) - spans) / spans)))
        ell = llref.track(pi, T, keys, E, ob)
        worst_ll = max(worst_ll, abs(ell[-1] - o["loglik"]) / abs(ell[-1]))
    return worst_ll, worst_sum


@pytest.mark.parametrize("M", MS)
def test_restatement_on_the_cases(M):
    for name in _names(M):
        if name in ("near64", "near_run60") or (name == "near_run" and M == 300):
            continue                   # (rows of `near`; M = 300: near_run60 is what the GPU test runs - the restatement costs seconds)
        ll, sm = _restatement(M, name)
        print(f"M = {M}, {name}: restatement against llref.track {ll:.2e} (bar {LL_REF_TOL:g}), gamma column sums {sm:.2e} (bar {GAMMA_SUM_RTOL:g})")
        assert sm <= GAMMA_SUM_RTOL, (M, name, sm)
        assert ll <= LL_REF_TOL, (M, name, ll)
