"""Records what every route of the parameter phase computes on a table of small inputs: tests/param_routes.json.

Every case is a fixed sequence of public calls on a fresh manager, in a process of its own on a GPU.  After each step the record
holds describe()'s q_route, plan.chain_family, plan.eigen_free_statistics, plan.per_row_gamma and statistics.eigen, the zlib.crc32
of the raw bytes of every array the step returned and, for a refusal, the exact text of smcpp_last_error.  The device and the host
preparation differ in the last bits (exp / expm1), so equal bytes also say that the same route ran.

    python tools/record_param_routes.py [--out tests/param_routes.json]     # all cases twice, one child process per run
    python tools/record_param_routes.py --case ID [--dump DIR]              # one case, JSON on stdout (arrays as DIR/<step>_<name>.npy)

A case whose two runs differ in a crc is listed under "not_reproducible" with the largest relative difference of each such array.
tests/test_param_routes.py imports CASES / run_case from here and replays every case in-process.

Steps: "model" / "model_seeds" / "model_b" set the model (without seeds, with identity seeds, other sizes without seeds);
("prep", host) = set_prep_mode; ("raw", "s" | "u") = set_raw with the host preparation's tables, T as prepared (structured) or with
one entry moved (unstructured); ("theta", v); "hs" = set the hidden states again (inner boundaries x 1.03); "global" = a global key
list of this input's keys and those of a second contig; "packunpack" = pack_stats -> unpack_stats; "gamma_on" = save_gamma;
("csfs", on) = smcpp_host_set_csfs_direct; "estep"; "stats" = loglik, xisums, gamma_sums (and the per-row posteriors where stored);
"Q" = Q's four terms (and their Jacobian where seeds are set); "score" = the score track's first call; "pi" "T" "E" "emission"
"dpi" "dT" "dE" = the getters.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TH, RH = 2.5e-2, 6.25e-3               # the benchmark model's theta, rho per 100 bp bin


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _contig(index, n, rows, stretch=1, without_b=None):
    """The first `rows` rows of a synthetic binned contig (spans up to 19); stretch: the span > 1 rows that many times as long;
    without_b: rows with that many derived alleles in the sample are left out first."""
    from smcpp_amd import synth
    c = synth.synth_contig(index, 4_000_000, n)
    c = c[c[:, 2] != without_b] if without_b is not None else c
    assert len(c) > rows, len(c)
    c = np.ascontiguousarray(c[:rows], dtype=np.int32).copy()
    c[:, 0] = np.where(c[:, 0] > 1, c[:, 0] * stretch, 1)
    return c


def _twopop_contigs():
    """tests/test_gpu_split.py's smallest input: example.12 of the reference's CI flow (vcf2smc, then base.py's pipeline without
    thinning / binning): un-binned rows, a = (2, 0)."""
    from smcpp_amd import data as D, vcf2smc as V
    vcf = os.path.join(ROOT, "tests", "golden", "example.vcf.gz")
    c, hdr = V.vcf2smc(vcf, "1", pop1=("msp1", ["msp_1", "msp_2"]), pop2=("msp2", ["msp_3", "msp_4", "msp_0"]), d=["msp_1", "msp_1"])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "example.12.smc.gz")
        V.write_smc(path, c, hdr)
        c = D.load_smc(path)
    c.data = D.compress_repeated_obs(c.data)
    cs = D.drop_small_contigs(D.break_long_spans(c, 100000), 100000)
    return tuple(int(x) for x in cs[0].n), [np.ascontiguousarray(x.data, dtype=np.int32) for x in cs]


def build_input(name):
    """-> dict(n, M, contigs[, extra]); extra: a contig whose keys join the global key list."""
    if name == "one":
        return dict(n=(4,), M=16, contigs=[_contig(1, 4, 4000)])
    if name == "fewer_keys":
        # (n = 4 has 11 keys and 4 000 rows show them all: this contig lacks two of those the second one holds)
        return dict(n=(4,), M=16, contigs=[_contig(1, 4, 4000, without_b=3)], extra=_contig(2, 4, 1500))
    if name == "long_spans":
        return dict(n=(4,), M=16, contigs=[_contig(1, 4, 4000, stretch=16)])     # rows of up to 304 positions: no eigen-free statistics
    if name == "n56":
        return dict(n=(56,), M=16, contigs=[_contig(1, 56, 2000)])
    if name == "M257":
        return dict(n=(4,), M=257, contigs=[_contig(1, 4, 4000)])
    if name == "two":
        n, contigs = _twopop_contigs()
        return dict(n=n, M=1, contigs=contigs)
    raise KeyError(name)


# ---- cases: id -> (input, switches, steps) -------------------------------------------------------------------------------------
def _case(inp, steps, env=None):
    return dict(input=inp, env=dict(env or {}), steps=tuple(steps))


_RUN = ("model", "estep", "stats", "Q")
CASES = {
    "default": _case("one", _RUN + ("T", "E", "pi", "Q", "estep", "stats")),
    "seeds": _case("one", ("model_seeds", "estep", "stats", "Q", "dpi", "dT", "dE", "emission", "Q")),
    "prep_mode_host": _case("one", (("prep", True),) + _RUN + ("E", "T")),
    "prep_mode_host_seeds": _case("one", (("prep", True), "model_seeds", "estep", "stats", "Q", "dT", "dE")),
    "env_prep_host": _case("one", _RUN + ("E",), {"SMCPP_PREP": "host"}),
    "csfs_direct": _case("one", (("csfs", True),) + _RUN + ("E",)),
    "size_not_supported": _case("n56", _RUN + ("E",)),
    "t_lazy_off": _case("one", _RUN + ("T",), {"SMCPP_T_LAZY": "0"}),
    "q_host": _case("one", _RUN + ("stats",), {"SMCPP_Q": "host"}),
    "q_host_seeds": _case("one", ("model_seeds", "estep", "Q", "stats"), {"SMCPP_Q": "host"}),
    "raw_structured": _case("one", (("raw", "s"), "estep", "stats", "Q", "T", "E")),
    "raw_unstructured": _case("one", (("raw", "u"), "estep", "stats", "Q")),
    "raw_then_theta": _case("one", ("model", "estep", ("raw", "s"), "estep", "stats", ("theta", 3e-2), "estep", "stats", "Q")),
    "global_keys": _case("fewer_keys", ("model", "global", "estep", "stats", "packunpack", "Q", "E", "Q")),
    "global_keys_seeds": _case("fewer_keys", ("model_seeds", "global", "estep", "packunpack", "Q", "dE", "Q")),
    "global_keys_host": _case("fewer_keys", (("prep", True), "model", "global", "estep", "stats", "packunpack", "Q", "E")),
    "save_gamma": _case("one", ("gamma_on",) + _RUN),
    "save_gamma_scan_off": _case("one", ("gamma_on",) + _RUN, {"SMCPP_GAMMA_SCAN": "0"}),
    "eigfree_off": _case("one", _RUN, {"SMCPP_EIGFREE": "0"}),
    "dense_chains": _case("one", _RUN, {"SMCPP_SS": "0"}),
    "long_spans": _case("long_spans", _RUN + ("E",)),
    # (the value getters prepare nothing: between set_params and the E-step they give the tables of the parameters before)
    "getters_between_pi_T_E": _case("one", ("model", "estep", "model_b", "pi", "T", "E", "estep", "stats", "E", "T", "pi", "Q")),
    "getters_between_E_T_pi": _case("one", ("model", "estep", "model_b", "E", "T", "pi", "estep", "stats", "Q", "pi", "T", "E")),
    "getter_before_first_preparation": _case("one", ("model", "pi")),
    "jac_getters_first": _case("one", ("model_seeds", "dE", "dT", "dpi", "estep", "stats", "Q", "dpi", "dT", "dE")),
    "jac_getters_after": _case("one", ("model_seeds", "estep", "dT", "Q", "emission", "Q", "stats")),
    "score_then_q": _case("one", ("gamma_on", "model_seeds", "estep", "score", "Q", "stats")),
    "hidden_states_between": _case("one", ("model", "estep", "stats", "hs", "estep", "stats", "Q")),
    "prep_mode_toggled": _case("one", ("model", "estep", ("prep", True), "estep", "stats", ("prep", False), "estep", "stats", "Q")),
    "params_set_again": _case("one", ("model", "estep", "model_b", "Q", "estep", "stats")),
    "q_before_estep": _case("one", ("model", "Q", "estep", "Q")),
    "twopop": _case("two", _RUN + ("E", "pi", "T")),
    "twopop_seeds": _case("two", ("model_seeds", "estep", "stats", "Q", "dE", "dT")),
    "twopop_prep_mode_host": _case("two", (("prep", True),) + _RUN + ("E",)),
    "M257_eigfree_off": _case("M257", (("raw", "s"), "estep"), {"SMCPP_EIGFREE": "0"}),
    "M257_unstructured": _case("M257", (("raw", "u"), "estep")),
}


# ---- one case -------------------------------------------------------------------------------------------------------------------
def crc(x):
    return int(zlib.crc32(np.ascontiguousarray(x).tobytes()) & 0xFFFFFFFF)


def _table(d):
    """A getter's {key: vector} dictionary as one array, keys in order."""
    return np.array([d[k] for k in sorted(d)])


def _models(inp, which):
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    a, s = synth.model_pieces()
    if which == "model_b":
        a = a * (1.0 + 0.1 * np.cos(np.arange(len(a))))
    if len(inp["n"]) == 1:
        m = PiecewiseModel(a, s, 1e4, "pop1")
        m.differentiable = which == "model_seeds"
        return m
    m1 = PiecewiseModel(a[:6], s[:6], 1e4, pid="msp1")
    m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(4)), s[:4], 1e4, pid="msp2")
    m1.differentiable = m2.differentiable = which == "model_seeds"
    return TwoPopulationModel(m1, m2, 0.3)


def manager(inp):
    from smcpp_amd import _smcpp, synth
    hs = synth.hidden_states(inp["M"])
    if len(inp["n"]) == 1:
        im = _smcpp.PyOnePopInferenceManager(inp["n"][0], inp["contigs"], hs, ("pop1",), 0.5)
    else:
        im = _smcpp.PyTwoPopInferenceManager(*inp["n"], 2, 0, inp["contigs"], hs, ("msp1", "msp2"), 0.5)
    im.theta = TH; im.rho = RH; im.alpha = 1.0
    return im


def _jac(im, name, shape):
    from smcpp_amd import _engine as E
    nder = int(E.lib().smcpp_num_derivatives(im._im))
    out = np.full(shape + (max(nder, 1),), np.nan)
    E.check(getattr(E.lib(), name)(im._im, E.dptr(out)))
    return out[..., :nder]


def _emission(im):
    from smcpp_amd import _engine as E
    nder = int(E.lib().smcpp_num_derivatives(im._im))
    cols = int(E.lib().smcpp_num_emission_cols(im._im))
    out = np.full((im.M, cols), np.nan); jac = np.full((im.M, cols, max(nder, 1)), np.nan)
    E.check(E.lib().smcpp_get_emission(im._im, E.dptr(out), E.dptr(jac) if nder else None))
    return {"emission": out, "demission": jac[..., :nder]}


def do_step(im, inp, st):
    """Runs one step; -> {name: array} of what it returned."""
    from smcpp_amd import _engine as E, synth
    if st in ("model", "model_seeds", "model_b"):
        im.model = _models(inp, st)
    elif st == "estep":
        im.E_step()
    elif st == "stats":
        out = {"loglik": im.logliks(), "xisums": np.array(im.xisums), "gamma_sums": np.concatenate([_table(g) for g in im.gamma_sums])}
        if im.describe()["plan"]["per_row_gamma"] != "none":
            out["gamma"] = np.concatenate(im.gammas, axis=1)
        return out
    elif st == "Q":
        nder = int(E.lib().smcpp_num_derivatives(im._im))
        if nder:
            q, jac = im.Q_with_gradient()
            return {"Q": q, "dQ": jac}
        return {"Q": np.array(im.Q(separate=True))}
    elif st == "pi":
        return {"pi": im.pi}
    elif st == "T":
        return {"transition": im.transition}
    elif st == "E":
        return {"emission_probs": _table(im.emission_probs)}
    elif st == "emission":
        return _emission(im)
    elif st == "dpi":
        return {"dpi": _jac(im, "smcpp_get_pi_jac", (im.M,))}
    elif st == "dT":
        return {"dT": _jac(im, "smcpp_get_transition_jac", (im.M, im.M))}
    elif st == "dE":
        return {"dE": _jac(im, "smcpp_get_emission_probs_jac", (len(im.keys), im.M))}
    elif st == "gamma_on":
        im.save_gamma = True
    elif st == "score":
        return {"score_rows": im.score_rows(0, 0, 60, 1)}
    elif st == "hs":
        hs = synth.hidden_states(inp["M"])
        hs[1:-1] *= 1.03
        im.hidden_states = hs
    elif st == "global":
        other = manager(dict(inp, contigs=[inp["extra"]]))
        gk = np.unique(np.vstack([im.keys, other.keys]), axis=0)
        assert len(gk) > len(im.keys)
        del other
        im.set_global_keys(gk)
    elif st == "packunpack":
        buf = im.pack_stats()
        im.unpack_stats(buf)
        return {"packed": buf}
    elif st[0] == "prep":
        im.set_prep_mode(st[1])
    elif st[0] == "theta":
        im.theta = st[1]
    elif st[0] == "csfs":
        E.host_set_csfs_direct(st[1])
    elif st[0] == "raw":
        a, s = synth.model_pieces()
        keys = im.keys
        pi, T, Et = E.host_prep_onepop(inp["n"][0], synth.hidden_states(inp["M"]), 0.5, a, s, TH, RH, 1.0, keys)
        if st[1] == "u":
            # one entry moved within its row: stochastic still, no longer the reference's HJTransition structure
            T = T.copy()
            T[0, -1] += 0.25 * T[0, 0]; T[0, 0] *= 0.75
        im.set_raw(pi, T, keys, Et)
    else:
        raise KeyError(st)
    return {}


def snapshot(im):
    d = im.describe()
    p, st = d["plan"], d.get("statistics")
    s = {"q_route": d["q_route"], "chain_family": p["chain_family"], "eigen_free_statistics": p["eigen_free_statistics"],
         "per_row_gamma": p["per_row_gamma"], "statistics_eigen": st["eigen"] if st else None}
    if "parameters" in d:                  # (printed from the parameter plan on; not part of the recorded table)
        s["parameters"] = d["parameters"]
    return s


def run_case(cid, set_option, dump=None):
    """Sets the case's switches through set_option(name, value), runs its steps on a fresh manager; -> one record per step
    ({"step", "describe", "crc"} or, for a refusal, {"step", "error"}: the case ends there)."""
    from smcpp_amd import _engine as E
    case = CASES[cid]
    for k, v in case["env"].items():
        set_option(k, v)
    direct = None
    try:
        inp = build_input(case["input"])
        im = manager(inp)
        recs = []
        for j, st in enumerate(case["steps"]):
            name = st if isinstance(st, str) else f"{st[0]}={st[1]}"
            if not isinstance(st, str) and st[0] == "csfs":
                direct = E.host_set_csfs_direct(False)
            try:
                arrays = do_step(im, inp, st)
            except RuntimeError as e:
                recs.append({"step": name, "error": str(e)})
                break
            if dump:
                os.makedirs(dump, exist_ok=True)
                for k, v in arrays.items():
                    np.save(os.path.join(dump, f"{j:02d}_{k}.npy"), np.ascontiguousarray(v))
            snap = snapshot(im)
            rec = {"step": name, "describe": {k: v for k, v in snap.items() if k != "parameters"}, "crc": {k: crc(v) for k, v in arrays.items()}}
            if "parameters" in snap:
                rec["parameters"] = snap["parameters"]
            recs.append(rec)
        del im
        return recs
    finally:
        if direct is not None:
            E.host_set_csfs_direct(direct)
        for k in case["env"]:
            set_option(k, None)


def _child(cid, dump):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cid, "--dump", dump], capture_output=True, text=True, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
    if r.returncode != 0 or not lines:
        print(f"case {cid} failed with exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
        return None
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--dump")
    ap.add_argument("--only", help="comma-separated case ids: record these and merge them into the table at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "param_routes.json"))
    args = ap.parse_args()
    if args.case:
        from smcpp_amd import _engine
        print("RECORD " + json.dumps(run_case(args.case, _engine.set_option, args.dump)), flush=True)
        return 0
    table = {"cases": {}, "not_reproducible": {}}
    only = args.only.split(",") if args.only else None
    if only:
        old = json.load(open(args.out))
        table["not_reproducible"] = {c: v for c, v in old["not_reproducible"].items() if c in CASES and c not in only}
        done = {c: v for c, v in old["cases"].items() if c not in only}
    with tempfile.TemporaryDirectory() as tmp:
        for cid in CASES:
            if only and cid not in only:
                if cid in done:
                    table["cases"][cid] = done[cid]
                continue
            runs = []
            for r in (1, 2):
                rec = _child(cid, os.path.join(tmp, f"{cid}_{r}"))
                if rec is None:
                    return 1               # nothing more is started on the device behind a case that failed
                runs.append(rec)
            table["cases"][cid] = runs[0]
            if runs[0] != runs[1]:
                # the same calls twice gave other bytes: the largest relative difference of every array that differs
                spread = {}
                for j, (a, b) in enumerate(zip(*runs)):
                    for k in a.get("crc", {}):
                        if a["crc"][k] != b.get("crc", {}).get(k):
                            x, y = (np.load(os.path.join(tmp, f"{cid}_{r}", f"{j:02d}_{k}.npy")) for r in (1, 2))
                            spread[f"{j:02d}_{k}"] = float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300)))
                table["not_reproducible"][cid] = {"spread": spread, "second_run": runs[1]}
            last = runs[0][-1]
            print(f"{cid}: {len(runs[0])} steps, {'reproduced' if runs[0] == runs[1] else 'NOT reproduced'}; last: "
                  f"{last.get('error') or last['describe']}", flush=True)
    write_table(table, args.out)
    print(f"wrote {args.out}: {len(table['cases'])} cases, {len(table['not_reproducible'])} not reproducible", flush=True)
    return 0


def write_table(table, path):
    """One case per line."""
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"not_reproducible":%s,"cases":{\n' % dumps(table["not_reproducible"]))
        f.write(",\n".join(f"{dumps(cid)}:{dumps(rec)}" for cid, rec in table["cases"].items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    sys.exit(main())
