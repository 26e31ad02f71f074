"""The statistics phase's plan and layout against tests/stats_plans.json: what smcpp_im::resolve_stats_plan() and the cut of the slabs gave
for every recipe, state count and form of tests/stats_cases.py BEFORE the layout was gathered into StatsLayout (engine_manager.hpp),
recorded through the host hook smcpp_host_stats_plan - tools/record_stats_plans.py holds the cases.

CPU: for EVERY case the hook gives the recorded object exactly ("statistics" as describe() prints it; "layout": counts, sizes, and per
list its length and the FNV-1a hash of its elements).  The forms' expected fields (stats_cases._forms: what tests/test_gpu_stats_edges.py
asserts from describe() on the device) hold without a device.  The cut's structure is asserted from the counts the hook returns,
against counts worked out here from the recipes alone: every row in exactly one slab of every list that covers it, slabs per
range, padding slabs in front of a change of eigen key, teams of four per reduction range, pieces of 64 positions.

GPU: a real manager after one E-step prints the "statistics" the hook gives for the device's own compute-unit count (the launched path
and the host view are the same code); and SMCPP_STATS_TEAM changed between construction and E-step - the slab target is the
construction's, the form of the rank updates the E-step's, and the partials are sized for what runs.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import stats_cases as sc
from conftest import ROOT

_spec = importlib.util.spec_from_file_location("record_stats_plans", os.path.join(ROOT, "tools", "record_stats_plans.py"))
rsp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rsp)

TABLE = json.load(open(os.path.join(ROOT, "tests", "stats_plans.json")))
CASES = rsp.cases()
FOLDS = ("none", "fold on the scans", "fold on the matrix cores")
# shares of k_sum_parts per reduction range of the 21-contig manager: max(8, min(16, 2048 / (contigs x blocks of Mp x Mp)))
SHARES = {13: 16, 48: 10, 64: 8, 80: 8, 144: 8}


def test_recipes_hold_every_count():
    """Every count the docstring of tests/test_gpu_stats_edges.py lists is present in the contigs as built, counted from the rows per
    contig, key and group; span-1 and span > 1 rows alternate, and a 16-row slab of the natural row order sees more than one key."""
    contigs = sc._contigs("edge")
    n1, n1k, grp, spans, none_gt1 = set(), set(), set(), set(), 0
    used = set()
    for c in contigs:
        s1, gt1 = sc._counted(c, sc.KEYS1)
        used |= set(s1)
        n1.add(sum(s1.values()))
        n1k |= set(s1.values())
        grp |= set(gt1.values())
        spans |= {g[0] for g in gt1}
        none_gt1 += not gt1
    for c in contigs:                   # a key of another contig that this contig does not hold: an empty (contig, key) range
        if used - set(sc._counted(c, sc.KEYS1)[0]):
            n1k.add(0)
    assert n1 >= sc.WANT_N1, sorted(sc.WANT_N1 - n1)
    assert n1k >= sc.WANT_N1_KEY, sorted(sc.WANT_N1_KEY - n1k)
    assert grp >= sc.WANT_GROUP, sorted(sc.WANT_GROUP - grp)
    assert spans >= sc.WANT_SPANS and max(spans) == 64, sorted(spans)
    assert none_gt1 >= 1 and len(contigs) >= 20
    assert max(sum(1 for v in sc._counted(c, sc.KEYS1)[1].values() if v == 1) for c in contigs) >= 50        # many groups of one row
    eig_keys = {g[1] for c in contigs for g in sc._counted(c, sc.KEYS1)[1]}
    assert eig_keys == {"mono", "miss"}
    c = contigs[[r[0] for r in sc.EDGE].index("n1=63")]
    s1rows = c[c[:, 0] == 1]
    assert len(np.unique(s1rows[:16, 1:], axis=0)) >= 4                                  # mixed keys inside one 16-row slab
    assert np.any((c[:-1, 0] == 1) & (c[1:, 0] > 1)) and np.any((c[:-1, 0] > 1) & (c[1:, 0] == 1))
    for kind in ("one", "two", "no_gt1", "twopop"):
        sc._contigs(kind)
    assert all(not sc._counted(c, sc.KEYS1)[1] for c in sc._contigs("no_gt1"))
    assert all(c.shape[1] == 7 for c in sc._contigs("twopop"))


def test_table_covers_every_case():
    assert set(TABLE["cases"]) == set(CASES) and TABLE["compute_units"] == rsp.COMPUTE_UNITS
    assert {k for k, _, _ in CASES.values()} == set(sc.KINDS) and {m for _, m, _ in CASES.values()} == set(sc.MS)


def _ceil(a, b):
    return -(-a // b)


def _expected_counts(kind, s_1, s_e):
    """What the cut must give for a kind's recipes with s_1 rows per span-1 rank slab and s_e per span > 1 slab, from the recipes alone."""
    recipes, keytab = sc.KINDS[kind]
    names = {k for _, s1, _ in recipes for k, v in s1.items() if v} | {g[1] for _, _, gt1 in recipes for g, v in gt1.items() if v}
    key_order = sorted(names, key=lambda k: keytab[k])                     # (the engine's key ids: lexicographic)
    eig_order = [k for k in key_order if any(g[1] == k for _, _, gt1 in recipes for g in gt1)]
    e = dict(n1=0, ne=0, pieces=0, K=len(key_order), Ke=len(eig_order), contigs=len(recipes), buckets=0,
             rk=0, sc=0, fk=0, eg=0, eg_pad=0, ek=0, ek_pad=0, teams_rk=0, teams_fk=0, teams_eg=0)
    eg_total, last_key, bucket_sizes = 0, None, []
    for _, s1, gt1 in recipes:
        n1c = sum(s1.values())
        e["n1"] += n1c
        e["ne"] += sum(gt1.values())
        e["pieces"] += sum(n * _ceil(g[0], 64) for g, n in gt1.items())
        rk = _ceil(n1c, s_1)
        fk = sum(_ceil(n, s_1) for n in s1.values())
        e["rk"] += rk; e["fk"] += fk
        e["sc"] += sum(_ceil(n, 256) for n in s1.values())
        e["teams_rk"] += _ceil(rk, 4); e["teams_fk"] += _ceil(fk, 4)
        for k in eig_order:
            groups = sorted((g[0], n) for g, n in gt1.items() if g[1] == k and n)
            for _, n in groups:
                # slabs of one eigen key start a workgroup of four: the padding slabs belong to the bucket in front of them
                if eg_total and last_key != k:
                    while eg_total % 4:
                        eg_total += 1; e["eg_pad"] += 1; bucket_sizes[-1] += 1
                last_key = k
                bucket_sizes.append(_ceil(n, s_e))
                eg_total += bucket_sizes[-1]
            rows = sum(n for _, n in groups)
            if rows:
                while (e["ek"] + e["ek_pad"]) % 4:
                    e["ek_pad"] += 1
                e["ek"] += _ceil(rows, s_e)
    e["buckets"] = len(bucket_sizes)
    e["eg"] = eg_total - e["eg_pad"]
    e["teams_eg"] = sum(_ceil(b, 4) for b in bucket_sizes)
    return e


def _assert_structure(kind, lay):
    ls = lay["lists"]
    e = _expected_counts(kind, lay["slab_rows_span1"], lay["slab_rows_span_gt1"])
    n = {k: v["n"] for k, v in ls.items()}
    assert (lay["rows_span1"], lay["rows_span_gt1"], lay["pieces"]) == (e["n1"], e["ne"], e["pieces"]), (lay, e)
    # every span-1 row in exactly one slab of slabs_rk, slabs_sc and slabs_fk; every span > 1 row in one of slabs_eg and of slabs_ek
    for name, rows in (("slabs_rk", e["n1"]), ("slabs_sc", e["n1"]), ("slabs_fk", e["n1"]), ("slabs_eg", e["ne"]), ("slabs_ek", e["ne"])):
        assert ls[name]["rows"] == rows and ls[name]["tiles_the_rows"] is True, (name, ls[name], rows)
    assert n["perm1"] == n["perm1k"] == e["n1"] and n["perme"] == n["epos_gid"] == n["erow_desc"] == n["erow_slab"] == e["ne"], n
    for name in ("slabs_rk", "slabs_sc", "slabs_fk"):
        assert ls[name]["padding"] == 0, (name, ls[name])
    assert (n["slabs_rk"], n["slabs_sc"], n["slabs_fk"]) == (e["rk"], e["sc"], e["fk"]), (n, e)
    # len(slabs_eg) - padding = sum over groups of ceil(rows / slab_rows); the same per (contig, eigen key) for slabs_ek
    assert (n["slabs_eg"] - ls["slabs_eg"]["padding"], ls["slabs_eg"]["padding"]) == (e["eg"], e["eg_pad"]), (ls["slabs_eg"], e)
    assert (n["slabs_ek"] - ls["slabs_ek"]["padding"], ls["slabs_ek"]["padding"]) == (e["ek"], e["ek_pad"]), (ls["slabs_ek"], e)
    # teams: ceil(slabs / 4) per reduction range, summed over the ranges (contigs; buckets, with the padding slabs they hold)
    assert (n["teams_rk"], n["teams_fk"], n["teams_eg"]) == (e["teams_rk"], e["teams_fk"], e["teams_eg"]), (n, e)
    C, K, Ke = e["contigs"], e["K"], e["Ke"]
    assert n["gk_slab_off"] == n["fk_gk_off"] == C * K + 1 and n["s1_slab_off"] == n["s1_team_off"] == n["fk_c_off"] == n["fk_c_team_off"] == C + 1, n
    assert n["ce_bucket_off"] == n["ce_row_off"] == n["ek_slab_off"] == C * Ke + 1, n
    assert n["eb_gid"] == e["buckets"] and n["eb_slab_off"] == n["eb_team_off"] == e["buckets"] + 1, (n, e)


@pytest.mark.parametrize("cid", list(CASES))
def test_host_view_reproduces_the_recorded_plan_and_layout(cid, engine_opt):
    kind, M, form = CASES[cid]
    got = rsp.host_view(kind, M, form, TABLE["compute_units"], engine_opt)
    assert got == rsp.unfold(TABLE["cases"][cid], TABLE["lists"])
    st, lay = got["statistics"], got["layout"]
    switches, save_gamma, want, eigfree = sc._forms(M)[form]
    rows = 16 if "SMCPP_SLAB_ROWS" in switches else 128
    assert (st["slab_rows_span1"], st["slab_rows_span_gt1"]) == (rows, rows) == (lay["slab_rows_span1"], lay["slab_rows_span_gt1"]), (cid, st)
    assert 8 <= st["reduction_shares"] <= 16 and st["reduction_shares"] == lay["reduction_shares"], (cid, st)
    assert lay["teams"] is (switches.get("SMCPP_STATS_TEAM") != "0"), (cid, lay)
    if kind in ("edge", "one", "two", "twopop"):
        # the forms' expected fields, as tests/test_gpu_stats_edges.py asserts them from describe() on the device
        for k, v in want.items():
            assert st[k] == v, (cid, k, st[k], v, st)
        assert (st["eigen"] in FOLDS) is eigfree, (cid, st)
    if kind == "edge":
        assert st["reduction_shares"] == SHARES[M], (cid, st)
    if kind == "no_gt1":
        # (SMCPP_EIGFREE=0 names the classic form, which launches nothing where there is no eigen key)
        assert st["eigen"] == ("classic" if "SMCPP_EIGFREE" in switches else "none") and lay["rows_span_gt1"] == 0, (cid, st)
    if kind == "unstructured":
        assert st["eigen"] == ("generation 2" if M <= 64 else "classic"), (cid, st)
    _assert_structure(kind, lay)


# ---------------------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------------------
GPU_FORMS = [(M, f) for M in (13, 64, 80, 144) for f in ("default", "per_slab", "eigensystem", "save_gamma") + (("two_kernels",) if M <= 64 else ())]


def _manager(M, engine_opt, switches, save_gamma=False):
    from test_gpu_gamma import RH_B, TH_B, _onepop
    for name in rsp.SWITCHES:
        engine_opt(name, switches.get(name))
    im = _onepop(M, sc._contigs("two"), TH_B, RH_B)
    im.save_gamma = save_gamma
    return im


@pytest.mark.gpu
@pytest.mark.parametrize("M,form", GPU_FORMS, ids=[f"M{M}-{f}" for M, f in GPU_FORMS])
def test_manager_runs_the_host_plan(M, form, engine_opt):
    """Kind `two` (five span-1 rank slabs in two teams): describe()["statistics"] after one E-step is the hook's for this device."""
    import torch
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    switches, save_gamma = sc._forms(M)[form][:2]
    im = _manager(M, engine_opt, switches, save_gamma)
    im.E_step()
    got = im.describe()["statistics"]
    del im
    assert got == rsp.host_view("two", M, form, cu, engine_opt)["statistics"]
    for k, v in sc._forms(M)[form][2].items():
        assert got[k] == v, (k, got)


def _close(a, b):
    """The bar of check 3 of tests/test_gpu_stats_edges.py: rtol 1e-11, atol 1e-13 of the largest entry."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-11 * np.abs(b) + 1e-13 * np.abs(b).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("M,extra", [(80, {}), (64, {"SMCPP_S1_FUSE": "0"})], ids=["M80", "M64-two_kernels"])
@pytest.mark.parametrize("built_with_teams", [True, False], ids=["teams_then_per_slab", "per_slab_then_teams"])
def test_stats_team_switch_changed_between_construction_and_estep(M, extra, built_with_teams, engine_opt):
    """The two-kernel span-1 form on kind `two` (five slabs, two teams): a manager built under one setting of SMCPP_STATS_TEAM and
    stepped under the other runs the rank updates the E-step's setting asks for, on partials sized for them, and gives the xi sums,
    gamma sums, gamma_0 and log-likelihoods of a manager that had the E-step's setting from the start."""
    from test_gpu_stats_edges import _outputs
    contigs = sc._contigs("two")
    at_build, at_step = ({}, {"SMCPP_STATS_TEAM": "0"}) if built_with_teams else ({"SMCPP_STATS_TEAM": "0"}, {})
    im = _manager(M, engine_opt, dict(extra, **at_build))
    engine_opt("SMCPP_STATS_TEAM", at_step.get("SMCPP_STATS_TEAM"))
    im.E_step()
    moved = _outputs(im, contigs)
    del im
    ref_im = _manager(M, engine_opt, dict(extra, **at_step))
    ref_im.E_step()
    ref = _outputs(ref_im, contigs)
    del ref_im
    want = "per slab" if built_with_teams else "teams"
    assert moved["st"]["rank_update"] == want and ref["st"]["rank_update"] == want, (moved["st"], ref["st"])
    assert moved["st"]["span1_form"] == "two kernels", moved["st"]
    assert moved["st"] == ref["st"]                      # (on inputs this small both managers cut the same slabs)
    assert _close(moved["ll"], ref["ll"]), (moved["ll"], ref["ll"])
    assert np.array_equal(moved["present"], ref["present"])
    for c in range(len(contigs)):
        assert _close(moved["xis"][c], ref["xis"][c]) and _close(moved["g0"][c], ref["g0"][c]), c
        for j in np.nonzero(ref["present"][c])[0]:
            assert _close(moved["gsr"][c][j], ref["gsr"][c][j]), (c, j)
