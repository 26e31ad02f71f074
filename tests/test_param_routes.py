"""The parameter phase's routes against tests/param_routes.json: what every route computed BEFORE its decisions were gathered into
ParamPlan / EstepRoute (engine_manager.hpp), recorded on an MI355X through the public calls alone, one process per case, every
case twice - tools/record_param_routes.py holds the cases, inputs and steps.  Every case reproduced byte for byte between its
two runs (the table's "not_reproducible" is empty), so every case is held exactly.

GPU: each case is replayed in-process.  After every step the describe() fields of the table (q_route, chain family, eigen-free
statistics, per-row gamma form, the statistics' eigen form), the crc32 of the raw bytes of every returned array and the text of a
refusal must equal the record.  The device and the host preparation differ in the last bits, so equal bytes also say that the
same route ran.  The new "parameters" object of describe() is held to an expectation written by hand beside each case: after
every step where the emission table and T live (two letters: d = device / h = host, g = generators / e = expanded; "-" = the
object is still null), and the rest of the object at the end of the case.

CPU: resolve_param_plan's truth table through smcpp_host_param_plan - every combination of the manager's state with SMCPP_PREP,
SMCPP_T_LAZY, SMCPP_Q and the literal-CSFS flag - and the order of precedence where several conditions force the host.  (Source and
why_host are what the object shows of the plan; what SMCPP_T_LAZY and SMCPP_Q plan shows on the GPU: "transition" is "generators"
only where a lazy T was planned, and the table's q_route and bytes hold Q's route.)
"""
import importlib.util
import itertools
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("record_param_routes", os.path.join(ROOT, "tools", "record_param_routes.py"))
rpr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rpr)

TABLE = json.load(open(os.path.join(ROOT, "tests", "param_routes.json")))

DEV, HOST1 = "ONEPOP_DEVICE", "ONEPOP_HOST"
# case -> (where the tables live after every step, then at the end: source, why_host, transition_jacobian, key_list, lean)
EXPECT = {
    # the lean E-step leaves the table on the device and expands T behind the chains; the getter of E fetches it for good
    "default": ("- de de de de he he he he he", DEV, "none", "none", "local", True),
    # Q's device route reads the planes; the getter of dT expands them, the getter of dE fetches the table
    "seeds": ("- de de de de de he he he", DEV, "none", "expanded", "local", True),
    "prep_mode_host": ("- - he he he he he", HOST1, "prep mode", "none", "local", True),
    "prep_mode_host_seeds": ("- - he he he he he", HOST1, "prep mode", "expanded", "local", True),
    "env_prep_host": ("- he he he he", HOST1, "switch", "none", "local", True),
    "csfs_direct": ("- - he he he he", HOST1, "literal CSFS", "none", "local", True),
    "size_not_supported": ("- he he he he", HOST1, "size not supported", "none", "local", True),
    "t_lazy_off": ("- de de de de", DEV, "none", "none", "local", True),
    # the host loops of Q fetch the table (and expand dT)
    "q_host": ("- de de he he", DEV, "none", "none", "local", True),
    "q_host_seeds": ("- de he he", DEV, "none", "expanded", "local", True),
    "raw_structured": ("he he he he he he", "RAW", "none", "none", "local", True),
    "raw_unstructured": ("he he he he", "RAW", "none", "none", "local", False),
    # set_theta on a manager that has a model leaves the raw path: the next E-step prepares on the device again
    "raw_then_theta": ("- de he he he he de de de", DEV, "none", "none", "local", True),
    "global_keys": ("- - de de de de he he", DEV, "none", "none", "global", True),
    "global_keys_seeds": ("- - de de de he he", DEV, "none", "expanded", "global", True),
    "global_keys_host": ("- - - he he he he he", HOST1, "prep mode", "none", "global", True),
    "save_gamma": ("- - de de de", DEV, "none", "none", "local", True),
    # not lean: the E-step itself fetches the table, in front of the generators
    "save_gamma_scan_off": ("- - he he he", DEV, "none", "none", "local", False),
    "eigfree_off": ("- he he he", DEV, "none", "none", "local", False),
    "dense_chains": ("- he he he", DEV, "none", "none", "local", False),
    "long_spans": ("- he he he he", DEV, "none", "none", "local", False),
    # set_params alone moves nothing; the getter of E fetches the table of the parameters before, the E-step prepares anew
    "getters_between_pi_T_E": ("- de de de de he de de he he he he", DEV, "none", "none", "local", True),
    "getters_between_E_T_pi": ("- de de he he he de de de de de he", DEV, "none", "none", "local", True),
    "getter_before_first_preparation": ("-", None, None, None, None, None),
    # the Jacobian getters prepare (with seeds T is expanded at once); the E-step finds fresh parameters and the table on the host
    "jac_getters_first": ("- he he he he he he he he he", DEV, "none", "expanded", "local", True),
    "jac_getters_after": ("- de de de he he he", DEV, "none", "expanded", "local", True),
    # the score track fetches into locals: the table stays on the device and Q on its device route
    "score_then_q": ("- - de de de de", DEV, "none", "expanded", "local", True),
    "hidden_states_between": ("- de de de de de de", DEV, "none", "none", "local", True),
    "prep_mode_toggled": ("- de de he he he de de de", DEV, "none", "none", "local", True),
    # Q prepares without an E-step: T stays as its generators until the E-step's statistics need the matrix
    "params_set_again": ("- de de dg de de", DEV, "none", "none", "local", True),
    "q_before_estep": ("- dg de de", DEV, "none", "none", "local", True),
    "twopop": ("- he he he he he he", "TWOPOP_DEVICE_BATCH", "none", "none", "local", False),
    "twopop_seeds": ("- he he he he he", "TWOPOP_HOST", "derivative seeds (two populations)", "expanded", "local", False),
    "twopop_prep_mode_host": ("- - he he he he", "TWOPOP_HOST", "prep mode", "none", "local", False),
    "M257_eigfree_off": ("he", "RAW", "none", "none", "local", False),
    "M257_unstructured": ("he", "RAW", "none", "none", "local", False),
}


def test_table_covers_every_case_and_every_case_reproduced():
    assert set(TABLE["cases"]) == set(rpr.CASES) == set(EXPECT)
    assert TABLE["not_reproducible"] == {}          # (every case is held exactly below)


def _residency(par):
    return "-" if par is None else ("d" if par["emission_table"] == "device" else "h") + ("g" if par["transition"] == "generators" else "e")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(rpr.CASES))
def test_route_reproduces_the_recorded_bytes(cid, engine_opt):
    want = TABLE["cases"][cid]
    got = rpr.run_case(cid, engine_opt)
    pars = [r.pop("parameters", None) for r in got]
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (cid, j, g, w)
    assert len(got) == len(want)
    codes, source, why, jac, key_list, lean = EXPECT[cid]
    done = [r for r in got if "error" not in r]
    seen = [_residency(p) for p in pars[:len(done)]]
    assert seen == codes.split(), (cid, seen)
    last = pars[len(done) - 1] if done else None
    if source is None:
        assert last is None
        return
    assert (last["source"], last["why_host"], last["transition_jacobian"], last["key_list"]) == (source, why, jac, key_list), (cid, last)
    assert last["lean"] is lean and last["eigen_free_statistics"] is lean
    if any(r["step"] == "estep" for r in done):        # (the same fact in the chain plan's words, which the table holds)
        assert last["eigen_free_statistics"] == done[-1]["describe"]["eigen_free_statistics"]


# ---- CPU: the truth table of resolve_param_plan ---------------------------------------------------------------------------------
def _expected_plan(npop, raw, force, nder, n, direct, prep_host):
    """Source and why_host as the code before ParamPlan decided them.  One population (engine_params.hpp:97-98 at that commit):
    `!host_only && !force_host_prep && DevPrep::supported(..) && !csfs_direct_flag()` - the first term that fails names the reason,
    in that order.  Two populations (engine_params.hpp:50-52): `host_only2 || force_host_prep || nder > 0` - the first that holds.
    The raw path returned before either (engine_params.hpp:29)."""
    if raw:
        return "RAW", "none"
    why = "switch" if prep_host else "prep mode" if force else None
    if npop == 2:
        why = why or ("derivative seeds (two populations)" if nder > 0 else None)
        return ("TWOPOP_HOST" if why else "TWOPOP_DEVICE_BATCH"), why or "none"
    why = why or ("size not supported" if n > 55 else "literal CSFS" if direct else None)
    return (HOST1 if why else DEV), why or "none"


@pytest.mark.parametrize("switches", list(itertools.product((False, True), repeat=4)),
                         ids=lambda s: "prep%d-lazy%d-q%d-direct%d" % tuple(int(x) for x in s))
def test_param_plan_truth_table(switches, engine_opt):
    from smcpp_amd import _engine
    prep_host, lazy_off, q_host, direct = switches
    engine_opt("SMCPP_PREP", "host" if prep_host else None)
    engine_opt("SMCPP_T_LAZY", "0" if lazy_off else None)
    engine_opt("SMCPP_Q", "host" if q_host else None)
    # (the literal-CSFS flag is read from SMCPP_CSFS_DIRECT once per process; tests move it through its C-ABI setter)
    before = _engine.host_set_csfs_direct(direct)
    try:
        for npop, raw, force, nder, n, glob in itertools.product((1, 2), (False, True), (False, True), (0, 3), (4, 55, 56), (False, True)):
            p = _engine.host_param_plan(npop, raw, force, nder, n, 16 + 17, glob)
            source, why = _expected_plan(npop, raw, force, nder, n, direct, prep_host)
            state = (npop, raw, force, nder, n, glob)
            assert (p["source"], p["why_host"]) == (source, why), (state, p)
            assert p["key_list"] == ("global" if glob else "local")
            # a manager that has prepared nothing yet: the table on the host, T expanded, no E-step
            assert (p["emission_table"], p["transition"], p["lean"], p["eigen_free_statistics"]) == ("host", "expanded", False, False)
            assert p["transition_jacobian"] == ("expanded" if nder and not raw else "none")
    finally:
        _engine.host_set_csfs_direct(before)


def test_param_plan_precedence_where_several_conditions_hold(engine_opt):
    """Everything at once (switch, prep mode, unsupported size, literal CSFS; seeds for two populations): the switch is named; without
    it the prep mode; without both the size before the literal CSFS / the seeds."""
    from smcpp_amd import _engine
    before = _engine.host_set_csfs_direct(True)
    try:
        for npop, third in ((1, "size not supported"), (2, "derivative seeds (two populations)")):
            engine_opt("SMCPP_PREP", "host")
            assert _engine.host_param_plan(npop, False, True, 2, 56)["why_host"] == "switch"
            engine_opt("SMCPP_PREP", None)
            assert _engine.host_param_plan(npop, False, True, 2, 56)["why_host"] == "prep mode"
            assert _engine.host_param_plan(npop, False, False, 2, 56)["why_host"] == third
        assert _engine.host_param_plan(1, False, False, 2, 55)["why_host"] == "literal CSFS"
        assert _engine.host_param_plan(2, False, False, 0, 56)["source"] == "TWOPOP_DEVICE_BATCH"      # (size and CSFS form: one population only)
    finally:
        _engine.host_set_csfs_direct(before)
