"""The sufficient-statistics kernels at their slab, team and share edges (smcpp_amd/csrc/kernels.hpp: k_s1_scalars, k_rank_acc<0..3>
with and without teams, k_rank_acc_wide, k_eig_fused2 + k_fin_Z2, k_eig_uw, k_span_scan / k_span_big, k_sum_parts, k_fin_both).

How these kernels cut their work is decided once per manager by smcpp_im::make_slabs() and per E-step by resolve_stats_plan(); every
cut has an edge where a kernel can drop a row, count it twice or read a partial nobody wrote.  The contigs here are therefore built
BY COUNT (`_build`): a recipe names how many span-1 rows of each key and how many rows of each (span, key) group a contig holds, the
rows are interleaved deterministically (the keys of the span-1 rows in rotation, the span > 1 rows spread over the gaps between
them, first and last row of span 1 wherever the contig has two span-1 rows), and every test first counts the rows it was given.

  EDGE, 21 contigs in ONE manager (each contig is a reduction range of its own), named by their span-1 row count:
    0 (span > 1 rows only) 1 2 3 4 5           the tails of one group of 4 rows (the MFMA k dimension of a span-1 rank update)
    15 16 17 63 64 65                          SMCPP_SLAB_ROWS=16: slab tails, a team of four slabs -1 / +1 slab
    127 128 129 143 144 145                    ... 8 and 9 slabs around the 8 shares of k_sum_parts, two teams + 1; default slabs:
    127 128 129 511 512 513                    tails of the 128-row slab, four slabs +-1
    span-1 rows per (contig, key)              0 (the key occurs in another contig only) 1 3 4 5 15 16 17 255 256 257: the 16 rows
                                               in flight and the 256-row slabs of k_s1_scalars, the key segments of k_rank_acc<3>
    rows per (contig, span, key) group         1 3 4 5 15 16 17, 31 32 33 (16-row slabs), 127 128 129 (default slabs); spans 2, 3,
                                               31, 63, 64; 58 groups of one row in one contig; two contigs without a span > 1 row;
                                               two eigen keys (monomorphic, missing), so the padding slabs of make_slabs appear
  ONE / TWO: managers of one and of two contigs (M = 64): fin_blocks x contigs = 19 / 36 <= 128, where k_fin_both may signal the
    host itself; EDGE at M = 64 has 399 blocks, where a one-thread kernel does it.
  NO_GT1: a manager without any span > 1 row (eigen: "none").
  TWOPOP: seven-column rows (M = 48); UNSTRUCTURED: set_raw with a T of no structure, which runs generation 2 with no switch.

Forms (each asserted from describe() BEFORE anything is compared; M = 13, 48, 64 (one state per lane), 80 (two), 144 (k_rank_acc_wide
on a ragged 256 x 128 block)).  The default span-1 form of a small input at M <= 64 with span > 1 rows is "one pass" (the span > 1
branch holds the main stream: engine_plans.hpp, crit_main), so the two-kernel form is asked for with SMCPP_S1_FUSE=0 there:
    default                  M <= 64: one pass, teams, fold on the scans;  M = 80: two kernels, teams;  M = 144: two kernels, wide
    SMCPP_S1_FUSE=0          two kernels (k_s1_scalars + k_rank_acc<0>) at M <= 64;  =1 on NO_GT1 (whose default is two kernels)
    SMCPP_STATS_TEAM=0       per slab (M = 144: wide without teams; with SMCPP_RANK_WIDE=0: per slab)
    SMCPP_RANK_WIDE=0        M = 144: teams
    SMCPP_SPAN_SCAN=0        fold on the matrix cores
    SMCPP_EIGFREE=0          generation 2 (M <= 64) / classic (M = 80, 144) on the binned rows themselves, eigen_free_statistics false
    save_gamma               two kernels; k_s1_scalars also writes the rows
    SMCPP_SLAB_ROWS=16       crossed with default, two kernels, per slab and the eigensystem forms (slab_rows_* 16 instead of 128)

Checks, per case and per contig (a failure names the contig's recipe):
  1. against the C restatement fed with the manager's own pi, T, keys and emission table: every entry of the xi sums (STAT_TOL
     relative), the gamma sums per key (STAT_TOL of the key's largest entry, same key set), gamma_0 (STAT_TOL), the log-likelihood
     (LL_TOL) - the bars of tests/test_gpu_parity.py;
  2. mass: sum(xisums[c]) and sum(gamma_sums[c]) equal the contig's positions to STAT_TOL (one lost or doubled position of at most
     20 000 is 10 bars);
  3. forms whose sums have positive terms only against each other (two kernels / one pass, teams / per slab, wide / narrow, 16-row /
     default slabs, save_gamma on / off): rtol 1e-11, atol 1e-13 of the largest entry - a re-ordered sum of at most 60 000 rows.
     The eigensystem forms subtract: restatement only, their difference from the eigen-free result is printed;
  4. save_gamma: a key's gamma sums against the sum of its rows' columns - span-1-only keys to (rows + 8) 2^-52 sum|terms|
     (k_s1_scalars adds the very values it stores), the others to GAMMA_TOL x the positions of the key's rows;
  5. SMCPP_DEBUG_POISON=nan, two E-steps on one manager with the model moved by +-2 % in between: everything finite, (contig, key)
     pairs without rows exactly zero, checks 1 and 2 on every contig, and the second E-step bit for bit what a fresh, unpoisoned
     manager gives on the second parameters (warm start is off: it is opt-in).

Which keys a contig's span-1 rows carry is this file's choice (the counts are not), and it matters for check 1: alpha is stored as
float by the reference and here, and on a few hundred rows that are a run of ONE polymorphic key the posterior never visits some
states, so the xi entries of those states are sums of tiny float products.  There the restatement ITSELF is 1e-5 .. 2e-4 (relative,
per entry) off an fp64 forward-backward of the same positions - measured on the CPU, outside this suite - and no engine can meet 5e-6
of it.  The recipes therefore mix keys; the one split that still missed (512 span-1 rows as 255 x (0, 7, 8) + 257 monomorphic: restatement
5e-5 off fp64 on entries of 1e-10 of the largest, engine 2.8e-5 .. 4.4e-5 off the restatement on the same entries at M >= 48, every form
alike and equal to each other to 1e-15) became 255 x (1, 0, 8) + 257 x (1, 0, 0), where the restatement is 7e-7 off fp64.

Measured on one MI355X (worst over the contigs of a case, range over the 77 runs: 60 form cases, the other managers, both E-steps of check 5; the file takes 5 s):
  check 1   log-likelihood 2.2e-09 .. 8.9e-08 (bar 1e-6), xi entries 3.6e-07 .. 2.7e-06 (5e-6), gamma sums 9.0e-08 .. 1.5e-06 (5e-6),
            gamma_0 6.6e-14 .. 8.6e-07 (5e-6)
  check 2   mass of the xi sums 8.9e-10 .. 3.7e-08, of the gamma sums 0 .. 8.2e-09 (5e-6)
  check 3   35 pairs of forms + 3 on NO_GT1: xi sums at most 9.5e-05 of the bar (1e-15 relative), gamma sums 3.3e-04 of it
            eigensystem forms against the eigen-free statistics (printed, not asserted): xi sums 6.3e-08 .. 7.3e-07, gamma sums
            7.3e-09 .. 1.4e-08
  check 4   span-1-only keys 0.09 .. 0.15 of (rows + 8) 2^-52 sum|terms|; the other keys 3.1e-04 .. 6.2e-04 of GAMMA_TOL x positions
  check 5   second E-step of the poisoned, reused manager = fresh clean manager in every bit (6 cases; the chains take 6 / 6 / 6
            passes at M = 48 and 1 / 1 / 1 at M = 80, reused and fresh alike)
No bug was found.  Tail masks removed one at a time on a scratch build (never committed), cases of this file that fail:
  `cur.valid &&` of k_rank_acc's consume         64 of 73: every case at M <= 128 and the narrow forms at M = 144 (72 misses per case)
  `if (!ok[u]) continue` of k_s1_scalars         49: every case whose span-1 form is "two kernels", none of the one-pass cases
  `vr ?` of k_eig_fused2                         8: the generation-2 cases (SMCPP_EIGFREE=0 at M <= 64, the unstructured T), no other
"""
import ctypes as C

import numpy as np
import pytest

from stats_cases import EDGE, KINDS, MS, S16, _contigs, _forms
from test_gpu_gamma import RH_B, TH_B, _onepop, _twopop, _unstructured
from test_gpu_parity import GAMMA_TOL, LL_TOL, STAT_TOL, oracle_estep

pytestmark = pytest.mark.gpu

FORMS = {M: _forms(M) for M in MS}
CASES = [(M, name) for M in MS for name in FORMS[M]]
# shares of k_sum_parts per reduction range of the 21-contig manager: max(8, min(16, 2048 / (contigs x blocks of Mp x Mp)))
SHARES = {13: 16, 48: 10, 64: 8, 80: 8, 144: 8}
ALL_SWITCHES = ("SMCPP_S1_FUSE", "SMCPP_STATS_TEAM", "SMCPP_RANK_WIDE", "SMCPP_SPAN_SCAN", "SMCPP_EIGFREE", "SMCPP_SLAB_ROWS")

_RUNS = {}


def _outputs(im, contigs):
    """Every statistic of the last E-step, the gamma sums of ALL (contig, key) pairs (the getter's raw table: pairs without rows
    included) and the parameters the restatement needs."""
    from smcpp_amd import _engine as E
    keys = im.keys
    K, M = len(keys), im.M
    ep = im.emission_probs
    gsr, present = np.zeros((len(contigs), K, M)), np.zeros((len(contigs), K), dtype=np.uint8)
    for c in range(len(contigs)):
        E.check(E.lib().smcpp_get_gamma_sums(im._im, c, E.dptr(gsr[c]), present[c].ctypes.data_as(C.POINTER(C.c_ubyte))))
    gam = im.gammas
    d = im.describe()
    return dict(ll=np.array(im.logliks()), xis=[x.copy() for x in im.xisums], gsr=gsr, present=present.astype(bool),
                g0=[g[:, 0].copy() for g in gam], gam=gam if im.save_gamma else None, keys=[tuple(int(x) for x in k) for k in keys],
                keys_arr=np.array(keys), pi=np.array(im.pi), T=np.array(im.transition), E=np.array([ep[tuple(k)] for k in keys.tolist()]),
                plan=d["plan"], st=d["statistics"])


def _manager(kind, M, contigs):
    if kind == "twopop":
        return _twopop(M, contigs)
    if kind == "unstructured":
        return _unstructured(M, contigs, TH_B, RH_B)
    return _onepop(M, contigs, TH_B, RH_B)


def _run(engine_opt, kind, M, switches, save_gamma=False):
    """One manager built UNDER the switches (make_slabs runs once per manager), one E-step; shared by the tests of the process."""
    key = (kind, M, tuple(sorted(switches.items())), save_gamma)
    if key not in _RUNS:
        contigs = _contigs(kind)
        for name in ALL_SWITCHES:
            engine_opt(name, switches.get(name))
        im = _manager(kind, M, contigs)
        im.save_gamma = save_gamma
        im.E_step()
        _RUNS[key] = _outputs(im, contigs)
        del im
        for name in ALL_SWITCHES:
            engine_opt(name, None)
    return _RUNS[key]


def _assert_plan(out, want, eigfree, slab16, label):
    st, plan = out["st"], out["plan"]
    for k, v in want.items():
        assert st[k] == v, (label, k, st[k], v, st)
    assert plan["eigen_free_statistics"] is eigfree, (label, plan)
    rows = 16 if slab16 else 128
    assert (st["slab_rows_span1"], st["slab_rows_span_gt1"]) == (rows, rows), (label, st)
    assert 8 <= st["reduction_shares"] <= 16, (label, st)


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------
def _gs(out, c):
    return {k: out["gsr"][c][j] for j, k in enumerate(out["keys"]) if out["present"][c][j]}


def _restatements(out, contigs):
    """The C restatement of every contig on the parameters of `out`: once per (parameters, contig) in a process (oracle_estep's
    cache), the contigs side by side on a few threads (the restatement is plain C behind ctypes and keeps no state)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    oracle.lib()                                           # (loaded once, before the threads ask for it)
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda ob: oracle_estep(out["pi"], out["T"], out["keys_arr"], out["E"], ob, save_gamma=False), contigs))


def _check_restatement_and_mass(out, kind, label, measures=("ll", "xi", "gs", "g0", "mass_xi", "mass_gs")):
    """Checks 1 and 2 on every contig: every contig is measured, then every miss is reported with its contig's recipe.
    -> the worst value of each measure over the contigs."""
    recipes, contigs = KINDS[kind][0], _contigs(kind)
    bars = dict(ll=LL_TOL, xi=STAT_TOL, gs=STAT_TOL, g0=STAT_TOL, mass_xi=STAT_TOL, mass_gs=STAT_TOL)
    worst = dict.fromkeys(bars, 0.0)
    misses = []
    for c, (rc, ob, o) in enumerate(zip(recipes, contigs, _restatements(out, contigs))):
        where = f"{label}, contig {c} {rc[0]} {rc[1]} {rc[2] if len(rc[2]) < 8 else str(len(rc[2])) + ' groups of one row'}"
        xs, gs, g0 = out["xis"][c], _gs(out, c), out["g0"][c]
        assert np.all(np.isfinite(xs)) and np.all(np.isfinite(out["gsr"][c])) and np.all(np.isfinite(g0)) and np.isfinite(out["ll"][c]), where
        rx = np.abs(xs - o["xisum"]) / np.maximum(np.abs(o["xisum"]), 1e-300)
        d = dict(ll=abs(out["ll"][c] - o["loglik"]) / max(1.0, abs(o["loglik"])), xi=float(rx.max()),
                 g0=float(np.max(np.abs(g0 - o["gamma"][:, 0]) / np.maximum(np.abs(o["gamma"][:, 0]), 1e-300))))
        assert sorted(gs) == sorted(o["gamma_sums"]), (where, sorted(gs), sorted(o["gamma_sums"]))
        d["gs"] = max([float(np.max(np.abs(gs[k] - v)) / max(np.abs(v).max(), 1e-300)) for k, v in o["gamma_sums"].items()], default=0.0)
        positions = float(ob[:, 0].sum())
        d["mass_xi"] = abs(float(xs.sum()) - positions) / positions
        d["mass_gs"] = abs(float(sum(v.sum() for v in gs.values())) - positions) / positions
        for k in measures:
            worst[k] = max(worst[k], d[k])
            if d[k] > bars[k]:
                i, j = np.unravel_index(rx.argmax(), rx.shape)
                misses.append(f"{where}: {k} {d[k]:.3e} above {bars[k]:g}" +
                              (f" (entry ({i}, {j}) = {o['xisum'][i, j]:.2e}, largest entry {o['xisum'].max():.2e})" if k == "xi" else ""))
        # (contig, key) pairs without rows: exactly zero in the raw table
        assert not np.any(out["gsr"][c][~out["present"][c]]), f"{where}: gamma sums of a key without rows are not zero"
    print(f"{label}: " + ", ".join(f"{k} {worst[k]:.2e}" for k in measures))
    assert not misses, "\n".join([f"{len(misses)} misses"] + misses)
    return worst


def _forms_differ(a, b):
    """-> (xi sums, gamma sums): the largest difference in units of the bar of check 3, rtol 1e-11 + atol 1e-13 of the largest entry."""
    wx = wg = 0.0
    for c in range(len(a["xis"])):
        x0, x1 = b["xis"][c], a["xis"][c]
        wx = max(wx, float(np.max(np.abs(x1 - x0) / (1e-11 * np.abs(x0) + 1e-13 * np.abs(x0).max()))))
        assert np.array_equal(a["present"][c], b["present"][c])
        for j in np.nonzero(b["present"][c])[0]:
            v0, v1 = b["gsr"][c][j], a["gsr"][c][j]
            wg = max(wg, float(np.max(np.abs(v1 - v0) / (1e-11 * np.abs(v0) + 1e-13 * np.abs(v0).max()))))
    return wx, wg


def _check_rows_against_sums(out, kind, label):
    """Check 4 (save_gamma): a key's gamma sums against the sum of the stored columns of its rows."""
    recipes, contigs = KINDS[kind][0], _contigs(kind)
    w1 = we = 0.0
    for c, (rc, ob) in enumerate(zip(recipes, contigs)):
        gam = out["gam"][c]
        assert gam.shape == (len(out["pi"]), len(ob) + 1) and np.all(np.isfinite(gam)), (label, rc)
        for j, k in enumerate(out["keys"]):
            rows = np.nonzero((ob[:, 1:] == np.array(k)).all(axis=1))[0]
            if len(rows) == 0:
                continue
            cols = gam[:, rows + 1]
            diff = np.abs(out["gsr"][c][j] - cols.sum(axis=1))
            if np.all(ob[rows, 0] == 1):
                bound = (len(rows) + 8) * 2.0 ** -52 * np.abs(cols).sum(axis=1)
                w1 = max(w1, float(np.max(diff / np.maximum(bound, 1e-300))))
                assert np.all(diff <= bound), f"{label}, contig {c} {rc}, span-1 key {k}: sums and rows differ by {diff.max():.3e}"
            else:
                bound = GAMMA_TOL * float(ob[rows, 0].sum())
                we = max(we, float(diff.max() / bound))
                assert diff.max() <= bound, f"{label}, contig {c} {rc}, key {k}: sums and rows differ by {diff.max():.3e} (bound {bound:.3e})"
    print(f"{label}: gamma sums against the stored rows: span-1-only keys {w1:.2f} of their bound, the other keys {we:.2e} of theirs")


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,form", CASES, ids=[f"M{M}-{name}" for M, name in CASES])
def test_form_against_restatement(engine_opt, M, form):
    """Checks 1 and 2 (and 4 under save_gamma) of one form on the 21 contigs of EDGE, its plan asserted first."""
    switches, save_gamma, want, eigfree = FORMS[M][form]
    label = f"M = {M}, {form}"
    out = _run(engine_opt, "edge", M, switches, save_gamma)
    _assert_plan(out, want, eigfree, "SMCPP_SLAB_ROWS" in switches, label)
    assert out["st"]["reduction_shares"] == SHARES[M], (label, out["st"])
    assert out["plan"]["save_gamma"] is save_gamma and out["plan"]["states"] == M, out["plan"]
    assert out["plan"]["states_per_lane"] == (M + 63) // 64 and out["plan"]["eigen_keys"] == 2 and out["plan"]["max_span"] == 64, out["plan"]
    _check_restatement_and_mass(out, "edge", label)
    if save_gamma:
        _check_rows_against_sums(out, "edge", label)
    if not eigfree:
        # the eigensystem forms subtract: printed against the eigen-free result of the same slabs, not asserted
        base = _run(engine_opt, "edge", M, S16 if "SMCPP_SLAB_ROWS" in switches else {}, False)
        dx = max(float(np.max(np.abs(a - b) / np.abs(b))) for a, b in zip(out["xis"], base["xis"]))
        dg = max(float(np.max(np.abs(out["gsr"][c][j] - base["gsr"][c][j])) / np.abs(base["gsr"][c][j]).max())
                 for c in range(len(out["xis"])) for j in np.nonzero(base["present"][c])[0])
        print(f"{label}: against the eigen-free statistics: xi sums {dx:.2e}, gamma sums {dg:.2e} (not asserted)")


def _pairs(M):
    """(form, form it is compared with) of check 3: only forms whose sums have positive terms."""
    if M <= 64:
        p = [("two_kernels", "default"), ("per_slab", "default"), ("two_kernels_per_slab", "two_kernels"), ("save_gamma", "two_kernels")]
        crossed = ("default", "two_kernels", "per_slab", "two_kernels_per_slab")
    elif M <= 128:
        p = [("per_slab", "default"), ("save_gamma", "default")]
        crossed = ("default", "per_slab")
    else:
        p = [("narrow", "default"), ("wide_no_teams", "default"), ("per_slab", "narrow"), ("save_gamma", "default")]
        crossed = ("default", "narrow", "per_slab")
    return p + [(name + "_slab16", name) for name in crossed]


@pytest.mark.parametrize("M", MS)
def test_forms_against_each_other(engine_opt, M):
    """Check 3: two kernels / one pass, teams / per slab, wide / narrow, 16-row / default slabs, save_gamma on / off, same contigs:
    every entry of the xi sums and of the gamma sums to the rounding of a re-ordered sum."""
    for a, b in _pairs(M):
        ra = _run(engine_opt, "edge", M, FORMS[M][a][0], FORMS[M][a][1])
        rb = _run(engine_opt, "edge", M, FORMS[M][b][0], FORMS[M][b][1])
        for name, r in ((a, ra), (b, rb)):
            _assert_plan(r, FORMS[M][name][2], FORMS[M][name][3], "SMCPP_SLAB_ROWS" in FORMS[M][name][0], f"M = {M}, {name}")
        wx, wg = _forms_differ(ra, rb)
        print(f"M = {M}: {a} against {b}: xi sums {wx:.2e}, gamma sums {wg:.2e} of rtol 1e-11 + atol 1e-13 max")
        assert wx <= 1.0 and wg <= 1.0, (M, a, b, wx, wg)


def test_few_and_many_contigs_take_both_finalisations(engine_opt):
    """k_fin_both signals the host itself while fin_blocks(Mp, K) x contigs <= 128 (engine_plans.hpp), else a one-thread kernel
    does: a manager of one contig and one of two (M = 64) are on one side, EDGE on the other; all three against the restatement."""
    M = 64
    blocks = {}
    for kind in ("one", "two", "edge"):
        out = _run(engine_opt, kind, M, {}, False)
        _assert_plan(out, FORMS[M]["default"][2], True, False, f"M = {M}, {kind}")
        _check_restatement_and_mass(out, kind, f"M = {M}, {kind}")
        Mp, K, nc = out["plan"]["states_padded"], out["plan"]["keys"], len(out["xis"])
        blocks[kind] = (-(-Mp * Mp // 256) + -(-(K + 1) * Mp // 256)) * nc
        print(f"M = {M}, {kind}: {nc} contigs, {K} keys: fin_blocks x contigs = {blocks[kind]}")
    assert blocks["one"] <= 128 and blocks["two"] <= 128 < blocks["edge"], blocks


def test_manager_without_span_gt1_rows(engine_opt):
    """No span > 1 row in any contig: eigen "none", nothing forks (two kernels by default); SMCPP_S1_FUSE=1 runs the one-pass form."""
    M = 48
    res = {}
    for name, sw, form in (("default", {}, "two kernels"), ("one pass", {"SMCPP_S1_FUSE": "1"}, "one pass"),
                           ("one pass, 16-row slabs", {"SMCPP_S1_FUSE": "1", "SMCPP_SLAB_ROWS": "16"}, "one pass"),
                           ("per slab, 16-row slabs", {"SMCPP_STATS_TEAM": "0", "SMCPP_SLAB_ROWS": "16"}, "two kernels")):
        out = res[name] = _run(engine_opt, "no_gt1", M, sw, False)
        assert out["st"]["eigen"] == "none" and out["st"]["span1_form"] == form and out["plan"]["eigen_keys"] == 0, (name, out["st"])
        assert out["st"]["rank_update"] == ("per slab" if "SMCPP_STATS_TEAM" in sw else "teams"), (name, out["st"])
        assert out["st"]["slab_rows_span1"] == (16 if "SMCPP_SLAB_ROWS" in sw else 128), (name, out["st"])
        _check_restatement_and_mass(out, "no_gt1", f"M = {M}, no span > 1 rows, {name}")
    for name in list(res)[1:]:
        wx, wg = _forms_differ(res[name], res["default"])
        print(f"M = {M}, no span > 1 rows: {name} against default: xi sums {wx:.2e}, gamma sums {wg:.2e} of the bar")
        assert wx <= 1.0 and wg <= 1.0, (name, wx, wg)


def test_unstructured_transition_matrix_runs_generation_2(engine_opt):
    """set_raw with a T of no structure (M = 48): the eigensystem statistics of generation 2 (k_eig_fused2 + k_fin_Z2) with no
    switch, on default slabs (127 / 128 / 129 rows per group: the last MFMA batch of 16 holds 15 / 16 / 1 rows)."""
    out = _run(engine_opt, "unstructured", 48, {}, False)
    assert out["st"]["eigen"] == "generation 2" and out["plan"]["eigen_free_statistics"] is False, (out["st"], out["plan"])
    assert out["st"]["slab_rows_span_gt1"] == 128 and out["st"]["span1_form"] == "two kernels", out["st"]
    _check_restatement_and_mass(out, "unstructured", "M = 48, unstructured T")


@pytest.mark.parametrize("slab16", [False, True], ids=["default_slabs", "slab16"])
def test_two_populations(engine_opt, slab16):
    """Seven-column rows (M = 48)."""
    out = _run(engine_opt, "twopop", 48, S16 if slab16 else {}, False)
    _assert_plan(out, FORMS[48]["default"][2], True, slab16, "M = 48, two populations")
    assert out["keys_arr"].shape[1] == 6
    _check_restatement_and_mass(out, "twopop", f"M = 48, two populations, {'16-row' if slab16 else 'default'} slabs")


def test_slab_plan_follows_slab_rows(engine_opt):
    """SMCPP_SLAB_ROWS is clamped to at least 16 (no upper clamp), span > 1 slabs are rounded up to a multiple of 16, span-1 slabs to a
    multiple of 4: the plan under SMCPP_SLAB_ROWS=16 differs from the default's, and other values come out as documented."""
    contigs = _contigs("one")
    got = {}
    for v in (None, "16", "1", "18", "200"):
        engine_opt("SMCPP_SLAB_ROWS", v)
        im = _onepop(13, contigs, TH_B, RH_B)
        im.E_step()
        st = im.describe()["statistics"]
        got[v] = (st["slab_rows_span1"], st["slab_rows_span_gt1"], st["reduction_shares"])
        del im
    engine_opt("SMCPP_SLAB_ROWS", None)
    print(f"slab plan per SMCPP_SLAB_ROWS: {got}")
    assert got == {None: (128, 128, 16), "16": (16, 16, 16), "1": (16, 16, 16), "18": (20, 32, 16), "200": (200, 208, 16)}, got
    assert got["16"] != got[None]


REUSE = [(48, "default"), (48, "two_kernels"), (48, "eigensystem"), (48, "default_slab16"), (80, "default"), (80, "eigensystem")]


@pytest.mark.parametrize("M,form", REUSE, ids=[f"M{M}-{name}" for M, name in REUSE])
def test_empty_ranges_and_reuse_on_poisoned_memory(engine_opt, M, form):
    """Check 5.  SMCPP_DEBUG_POISON=nan: every fresh float allocation is NaN.  An E-step, the model moved by +-2 %, a second E-step
    on the same manager: everything finite, (contig, key) pairs without rows exactly zero, checks 1 and 2 on every contig (the one
    without span-1 rows and the two without span > 1 rows among them), and the second E-step bit for bit what a fresh manager
    without poison gives on the second parameters (warm start is opt-in and off)."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    switches, save_gamma, want, eigfree = FORMS[M][form]
    contigs = _contigs("edge")
    a, s = synth.model_pieces()
    a2 = np.asarray(a, dtype=float) * (1.0 + 0.02 * (-1.0) ** np.arange(len(a)))
    label = f"M = {M}, {form}, poisoned"
    for name in ALL_SWITCHES:
        engine_opt(name, switches.get(name))
    engine_opt("SMCPP_DEBUG_POISON", "nan")
    im = _onepop(M, contigs, TH_B, RH_B)
    assert im.describe()["plan"]["warm_start"] is False
    im.E_step()
    first = _outputs(im, contigs)
    _assert_plan(first, want, eigfree, "SMCPP_SLAB_ROWS" in switches, label)
    _check_restatement_and_mass(first, "edge", label + ", first E-step")
    im.model = PiecewiseModel(a2, s, 1e4, "pop1")
    im.E_step()
    second = _outputs(im, contigs)
    del im
    _check_restatement_and_mass(second, "edge", label + ", second E-step")
    assert abs(second["ll"].sum() - first["ll"].sum()) >= 1e-6 * abs(first["ll"].sum()), "the second parameters do not move the log-likelihood"
    engine_opt("SMCPP_DEBUG_POISON", None)
    fresh_im = _onepop(M, contigs, TH_B, RH_B)
    fresh_im.model = PiecewiseModel(a2, s, 1e4, "pop1")
    fresh_im.E_step()
    fresh = _outputs(fresh_im, contigs)
    del fresh_im
    for name in ALL_SWITCHES:
        engine_opt(name, None)
    print(f"{label}: passes to the certificate {first['plan']['passes_to_certificate']} / {second['plan']['passes_to_certificate']}, "
          f"fresh {fresh['plan']['passes_to_certificate']}")
    assert np.array_equal(second["present"], fresh["present"])
    assert np.array_equal(second["ll"], fresh["ll"]), label
    assert np.array_equal(second["gsr"], fresh["gsr"]), label
    for c, rc in enumerate(EDGE):
        assert np.array_equal(second["xis"][c], fresh["xis"][c]), (label, rc)
        assert np.array_equal(second["g0"][c], fresh["g0"][c]), (label, rc)
