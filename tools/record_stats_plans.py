"""Records the statistics phase's plan and layout on the recipes of tests/stats_cases.py: tests/stats_plans.json.

Needs no GPU: every case is one call of the host hook smcpp_host_stats_plan (build_layout, make_chunks, the layout cut, the route and
the plan of a first E-step) under the case's switches, for one fixed compute-unit count that is written into the table.

    python tools/record_stats_plans.py [--out tests/stats_plans.json]

Cases: every kind of stats_cases.KINDS (edge, one, two, no_gt1; twopop at M = 48 only; unstructured = the contigs of edge with
structured_T = 0), every M of stats_cases.MS, every form of stats_cases._forms(M) with its switches and its save_gamma; id
"<kind>:M<M>:<form>".  A case records {"statistics": describe()'s object, "layout": the hook's layout object}; the "lists" member
of the layout (length and FNV-1a hash of every list) depends on the contigs and the slab size only, so the table holds every distinct
one once, under "lists", and a case names it.  tests/test_stats_plan.py imports cases / host_view from here.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stats_cases as sc  # noqa: E402

COMPUTE_UNITS = 256
SWITCHES = ("SMCPP_S1_FUSE", "SMCPP_STATS_TEAM", "SMCPP_RANK_WIDE", "SMCPP_SPAN_SCAN", "SMCPP_EIGFREE", "SMCPP_SLAB_ROWS")


def cases():
    """id -> (kind, M, form name)"""
    out = {}
    for kind in sc.KINDS:
        for M in ((48,) if kind == "twopop" else sc.MS):
            for form in sc._forms(M):
                out[f"{kind}:M{M}:{form}"] = (kind, M, form)
    return out


def host_view(kind, M, form, compute_units, set_option):
    """The hook on a kind's contigs under the form's switches: -> {"statistics": ..., "layout": ...}."""
    from smcpp_amd import _engine, synth
    switches, save_gamma = sc._forms(M)[form][:2]
    for name in SWITCHES:
        set_option(name, switches.get(name))
    try:
        n, na = ((4, 3), (2, 0)) if kind == "twopop" else ((8,), (2,))
        return _engine.host_stats_plan(n, na, sc._contigs(kind), synth.hidden_states(M), compute_units, save_gamma, kind != "unstructured")
    finally:
        for name in SWITCHES:
            set_option(name, None)


def _dumps(x):
    return json.dumps(x, sort_keys=True, separators=(",", ":"))


def fold(view, lists):
    """The record of a view: its "lists" replaced by their name in `lists` (added there when new)."""
    lay = dict(view["layout"])
    name = hashlib.sha1(_dumps(lay["lists"]).encode()).hexdigest()[:12]
    lists.setdefault(name, lay["lists"])
    lay["lists"] = name
    return {"statistics": view["statistics"], "layout": lay}


def unfold(rec, lists):
    return {"statistics": rec["statistics"], "layout": dict(rec["layout"], lists=lists[rec["layout"]["lists"]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "stats_plans.json"))
    args = ap.parse_args()
    from smcpp_amd import _engine
    lists, recs = {}, {}
    for cid, (kind, M, form) in cases().items():
        recs[cid] = fold(host_view(kind, M, form, COMPUTE_UNITS, _engine.set_option), lists)
    with open(args.out, "w") as f:                  # one case per line
        f.write('{"compute_units":%d,"lists":{\n' % COMPUTE_UNITS)
        f.write(",\n".join(f"{_dumps(k)}:{_dumps(v)}" for k, v in lists.items()))
        f.write('\n},"cases":{\n')
        f.write(",\n".join(f"{_dumps(k)}:{_dumps(v)}" for k, v in recs.items()))
        f.write("\n}}\n")
    print(f"wrote {args.out}: {len(recs)} cases, {len(lists)} distinct lists objects", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
