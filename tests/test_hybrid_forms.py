"""Which form of the hybrid rows' eigen-power step the plan picks for every (state count, eigen keys) that tests/test_gpu_hybrid_forms.py
runs, from the host hook alone (`smcpp_host_chain_plan` with the compute-unit count of tests/chain_plans.json): the table of
tests/hybrid_cases.py - literal forms, tables in LDS and cold eigen keys, derived from the LDS sizes, not from the rule - and what
the GPU cases rely on in their inputs, checked where no GPU is present."""
import json
import os

import numpy as np
import pytest

import hybrid_cases as hc
from conftest import ROOT

CU = json.load(open(os.path.join(ROOT, "tests", "chain_plans.json")))["compute_units"]
_IN = {}


def _input(case, r):
    if (case, r) not in _IN:
        _IN[case, r] = hc.case_input(case, r)
    return _IN[case, r]


def _plan(inp, rows_per_chunk=hc.CHUNK_ROWS):
    from smcpp_amd import _engine, synth
    return _engine.host_chain_plan((inp["n"],), (2,), inp["contigs"], synth.hidden_states(inp["M"]), CU, rows_per_chunk)


def test_the_table_of_forms_follows_from_the_lds_sizes():
    """The constants of hybrid_cases.FORMS against the byte counts each form is decided on, spelled out once more."""
    for (Mp, ke), (form, in_lds) in hc.FORMS.items():
        per_key = 4 * Mp * (Mp + 1) * 8
        if ke * per_key <= 120 * 1024:
            assert (form, in_lds) == (hc.ALL, ke), (Mp, ke)
        elif ke * per_key // 2 <= 136 * 1024:
            assert (form, in_lds) == (hc.SPLIT, ke), (Mp, ke)
        else:
            assert form == hc.COLD and in_lds == (136 * 1024) // (per_key // 2) and 1 <= in_lds < ke, (Mp, ke)
    # the cases reach every entry but two plain ones of the small tables
    assert set(hc.FORMS) - {(16 * ((v[0] + 15) // 16), v[1]) for c, v in hc.CASES.items() if c != 15} == {(16, 3), (32, 2)}


@pytest.mark.parametrize("case,r", hc.INPUTS)
def test_host_plan_reports_the_form(case, r):
    inp = _input(case, r)
    d, fwd, _ = _plan(inp)
    plan, hyb = d["plan"], d["hybrid"]
    assert plan["states"] == inp["M"] and plan["states_padded"] == inp["Mp"] and plan["eigen_keys"] == inp["Ke"]
    assert plan["keys"] == len(inp["keys"]) and plan["max_span"] == hc.LONGEST
    if case == 15:
        assert hyb is None and plan["chain_family"] == 2 and not plan["hybrid_rows"] and not plan["scan_chains"]
        return
    assert plan["chain_family"] == 6 and plan["hybrid_rows"]
    assert hyb["form"] == inp["form"] and hyb["tables_in_lds"] == inp["tables_in_lds"] and hyb["cold_eigen_keys"] == inp["cold"]
    assert hyb["eigen_keys"] == inp["Ke"] and hyb["threshold"] == 6 and hyb["hot_eigen_key"] == inp["hot"]
    assert hyb["workgroup_wavefronts"] == 4
    assert hyb["all_keys_in_lds"] == (case != 12) and (hyb["emission_slots_in_lds"] < plan["keys"]) == (case == 12)
    # the long contig is cut into a dozen chunks, the short one into three or four, the one-row contig is one
    per_contig = np.bincount(fwd[:, 0], minlength=3)
    assert 12 <= per_contig[0] <= 13 and 3 <= per_contig[1] <= 4 and per_contig[2] == 1


def test_cold_and_hot_keys_cover_every_index():
    """The rotations make every eigen-key index the cold one once (cases 10 and 13), the hot one once (case 5), and case 14 has two
    disjoint cold pairs."""
    cold = {c: [tuple(_input(c, r)["cold"]) for r in range(len(hc.CASES[c][4]))] for c in (10, 13, 14)}
    assert sorted(cold[10]) == [(0,), (1,), (2,), (3,)] and sorted(cold[13]) == [(0,), (1,), (2,)]
    assert len(cold[14]) == 2 and sorted(cold[14][0] + cold[14][1]) == [0, 1, 2, 3]
    assert sorted(_input(5, r)["hot"] for r in range(3)) == [0, 1, 2]


@pytest.mark.parametrize("th", [1, 40])
def test_threshold_switch_reaches_the_plan(th, engine_opt):
    engine_opt("SMCPP_HYB_TH", th)
    inp = _input(14, 0)
    hyb = _plan(inp)[0]["hybrid"]
    assert hyb["threshold"] == th and hyb["form"] == hc.COLD and hyb["cold_eigen_keys"] == inp["cold"]


@pytest.mark.parametrize("case,r", hc.INPUTS)
def test_inputs_hold_what_the_gpu_cases_rely_on(case, r):
    """Only eigen keys have span > 1; every eigen key has, for either threshold, a row on each side of it and a row of 10^5 in the
    long and the short contig, at least 30 rows above the larger threshold in the long contig, and at least one in the long contig's
    first and last chunk (rows 1 .. 200 and the last 200: chunks by rows)."""
    inp = _input(case, r)
    long_, short, one = inp["contigs"]
    assert 2500 <= len(long_) < 2540 and 700 <= len(short) < 725 and len(one) == 1 and one[0, 0] > 512
    keys = {tuple(k) for c in inp["contigs"] for k in c[:, 1:].tolist()}
    assert keys == set(inp["keys"]) and sorted(keys) == sorted(inp["keys"])
    for c in inp["contigs"]:
        assert c[:, 0].min() >= 1 and c[:, 0].max() == hc.LONGEST
        assert {tuple(k) for k in c[c[:, 0] > 1, 1:].tolist()} <= set(inp["eigen_keys"])
    frac1 = np.mean(long_[:, 0] == 1)
    assert 0.40 <= frac1 <= 0.50
    for k in inp["eigen_keys"]:
        for c in (long_, short):
            spans = c[np.all(c[:, 1:] == np.array(k), axis=1), 0]
            for t in hc.TH:
                assert t in spans and t + 1 in spans
            assert hc.LONGEST in spans
        rows = hc.long_rows(long_, k, max(hc.TH))
        assert len(rows) >= 30
        assert rows.min() < hc.CHUNK_ROWS - 8 and rows.max() >= len(long_) - hc.CHUNK_ROWS + 8
