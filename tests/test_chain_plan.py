"""The chain phase's plan against tests/chain_plans.json: what the engine planned for a table of small inputs BEFORE the plan was
gathered into ChainPlan / ChainPass (engine_manager.hpp), recorded on an MI355X through the public hooks alone (describe(),
chunks(), chain_mode()) after one E-step per case, one process per case - tools/record_chain_plans.py holds the cases and inputs.

CPU: `smcpp_host_chain_plan`, the host-only view of the same resolve and cut functions a manager runs, called with the recorded
compute-unit count, gives for EVERY case of the table the recorded "plan" object (with "power_jumps"), chain family and both
chunk lists (length, crc32 of the int32 array, first and last three chunks).  Compared exactly, except for what is not plan but
state an E-step on a device leaves behind, which a host-only view cannot know:

  passes_to_certificate   learned by run_chains_ss from the device's flags;
  eigen_free_statistics   decided per E-step from the transition matrix;
  host_threads            omp_get_max_threads() of the machine that ran;
  warm_start              the caller's setting (smcpp_set_warm_start), no argument of the hook;
  passes_launched         the hook gives the passes a first E-step launches UP FRONT.  Where the recorded E-step certified within
                          them (passes_to_certificate <= that count) the two are equal; where it did not, run_chains_ss launched
                          further rounds of three passes each (engine_plans.hpp), so the recorded count is the hook's plus a multiple
                          of three, capped at the plan's pass budget.  (The hand-built size inputs forget slowly: up to 294 passes.)

The same test documents the size rule of one state per lane in its own unit - positions per SIMD - by calling the hook with four
compute units: the plan changes at 1 300, 1 900 and 11 700 positions per SIMD.

GPU: for seven small cases a real manager after one E-step gives the table's describe() / chunks() / chain_mode() AND the host
hook's (called with the device's own compute-unit count): the launched path and the host view are the same code.  The warm start's
second E-step exists on the device only.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("record_chain_plans", os.path.join(ROOT, "tools", "record_chain_plans.py"))
rcp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rcp)

TABLE = json.load(open(os.path.join(ROOT, "tests", "chain_plans.json")))
STATE = ("passes_to_certificate", "eigen_free_statistics", "host_threads", "warm_start", "passes_launched")
_INPUTS = {}


def _input(name):
    if name not in _INPUTS:
        _INPUTS[name] = rcp.build_input(name)
    return _INPUTS[name]


def host_view(case, compute_units, engine_opt):
    """The hook on a case's input under its switches and its last set_chunking: -> (plan dict, chunk digests of both lists)."""
    from smcpp_amd import _engine, synth
    for k, v in case["env"].items():
        engine_opt(k, v)
    inp = _input(case["input"])
    rows_per_chunk = ([0] + [st[1] for st in case["steps"] if isinstance(st, tuple)])[-1]
    d, fwd, bwd = _engine.host_chain_plan(inp["n"], inp["na"], inp["contigs"], synth.hidden_states(inp["M"]), compute_units, rows_per_chunk)
    for k in case["env"]:
        engine_opt(k, None)
    return d["plan"], rcp.chunk_digest(fwd), rcp.chunk_digest(bwd)


def family_of(plan):
    return plan["chain_family"]


def test_table_covers_every_case():
    assert set(TABLE["cases"]) == set(rcp.CASES) and TABLE["compute_units"] > 0


@pytest.mark.parametrize("cid", list(rcp.CASES))
def test_host_plan_reproduces_the_recorded_plan(cid, engine_opt):
    rec = TABLE["cases"][cid]
    plan, fwd, bwd = host_view(rcp.CASES[cid], TABLE["compute_units"], engine_opt)
    want = rec["plan"]
    assert set(plan) == set(want)
    assert {k: plan[k] for k in plan if k not in STATE} == {k: want[k] for k in want if k not in STATE}
    assert family_of(plan) == rec["chain_mode"]
    assert fwd == rec["chunks_forward"] and bwd == rec["chunks_backward"]
    up_front, launched = plan["passes_launched"], want["passes_launched"]
    if want["passes_to_certificate"] <= up_front:
        assert launched == up_front
    else:
        assert launched > up_front and (launched - up_front) % 3 == 0


def test_size_regimes_change_at_1300_1900_11700_positions_per_simd(engine_opt):
    """One state per lane on four compute units (16 SIMDs): below 1 300 positions per SIMD light passes with one wavefront; from
    1 300 the float halo with one; from 1 900 with two; from 11 700 three wavefronts and no halo."""
    from smcpp_amd import _engine, synth
    seen = {}
    for positions in (1300 * 16 - 1, 1300 * 16, 1900 * 16 - 1, 1900 * 16, 11700 * 16 - 1, 11700 * 16):
        # rows alternating span 1 and span 64 (65 k + 2 positions), filled up with span-1 rows to the exact count
        c = rcp._alt(positions - 2)[0]
        fill = np.zeros((positions - int(c[:, 0].sum()), 4), dtype=np.int32)
        fill[:, 0] = 1; fill[:, 1:] = (0, 1, rcp.N)
        d, _, _ = _engine.host_chain_plan((rcp.N,), (2,), [np.vstack([c, fill])], synth.hidden_states(64), 4)
        p = d["plan"]
        assert p["positions"] == positions and p["states_per_lane"] == 1
        seen[positions // 16] = (p["wavefronts_per_simd"], p["halo_pass"], p["light_passes_forward"] > 0)
    assert sorted(seen) == [1299, 1300, 1899, 1900, 11699, 11700]
    for per_simd, v in seen.items():
        want = (1, False, True) if per_simd < 1300 else (1, True, False) if per_simd < 1900 else (2, True, False) if per_simd < 11700 else (3, False, False)
        assert v == want, (per_simd, v, want)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", rcp.GPU_SAMPLE)
def test_manager_runs_the_recorded_and_the_host_plan(cid, engine_opt):
    import torch
    rec = TABLE["cases"][cid]
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    got = rcp.run_case(cid, engine_opt)
    assert cu == TABLE["compute_units"]          # (the table is the MI355X's)
    for snap, want in [(got, rec)] + ([(got["second"], rec["second"])] if "second" in rec else []):
        assert {k: v for k, v in snap["plan"].items() if k != "host_threads"} == {k: v for k, v in want["plan"].items() if k != "host_threads"}
        assert snap["chain_mode"] == want["chain_mode"]
        assert snap["chunks_forward"] == want["chunks_forward"] and snap["chunks_backward"] == want["chunks_backward"]
    plan, fwd, bwd = host_view(rcp.CASES[cid], cu, engine_opt)
    mine = got["plan"]
    assert {k: plan[k] for k in plan if k not in STATE} == {k: mine[k] for k in mine if k not in STATE}
    assert family_of(plan) == got["chain_mode"] and fwd == got["chunks_forward"] and bwd == got["chunks_backward"]
    if mine["passes_to_certificate"] <= plan["passes_launched"]:
        assert mine["passes_launched"] == plan["passes_launched"]
