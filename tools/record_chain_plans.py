"""Records what the chain phase plans for a table of small inputs: tests/chain_plans.json.

Every case runs in a process of its own on a GPU: it builds its input (smcpp_amd.synth with fixed seeds, or hand-built rows), sets its
switches, runs one E-step on the benchmark model and records, through the public hooks only, describe()["plan"] (with its
"power_jumps" object), chain_mode() and both chunk lists (length, zlib.crc32 of the int32 array, first and last three chunks).

    python tools/record_chain_plans.py [--out tests/chain_plans.json]      # all cases, one child process each
    python tools/record_chain_plans.py --case ID                           # one case, JSON on stdout

tests/test_chain_plan.py imports CASES / build_input from here and holds the host-only view of the plan (smcpp_host_chain_plan) and
a real manager to the recorded table.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N = 8                                  # haploid sample size of the one-population inputs
TH_B, RH_B = 2.5e-2, 6.25e-3           # the benchmark model's theta, rho per 100 bp bin (binned rows)
TH_U, RH_U = 2e-4, 6e-5                # per base pair (un-binned rows)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _edged(body, ncol=4):
    """First and last row of span 1."""
    if body[0, 0] == 1 and body[-1, 0] == 1:
        return np.ascontiguousarray(body, dtype=np.int32)
    first = np.zeros((1, ncol), dtype=np.int32); first[0, 0] = 1; first[0, 1] = 1
    last = np.zeros((1, ncol), dtype=np.int32); last[0, 0] = 1
    return np.ascontiguousarray(np.vstack([first, body, last]), dtype=np.int32)


def _tiny(long_span, ncol=4):
    one = np.zeros((1, ncol), dtype=np.int32); one[0, 0] = 1; one[0, 1] = 1
    two = np.zeros((2, ncol), dtype=np.int32); two[:, 0] = (long_span, 1)
    return [one, two]


def _rows(seed, positions, max_span, n=N, twopop=None, stretch=1):
    """Binned synthetic rows cut to about `positions` positions, spans capped at max_span; stretch > 1: the span > 1 rows that many
    times as long (rows for the engine to cut).  (tests/test_gpu_seams.py builds its inputs the same way.)"""
    from smcpp_amd import synth
    bp = 100 * positions + 4000
    c = (synth.synth_contig_twopop(seed, bp, *twopop) if twopop else synth.synth_contig(seed, bp, n)).copy()
    c[:, 0] = np.minimum(np.where(c[:, 0] > 1, c[:, 0] * stretch, 1), max_span)
    cut = int(np.searchsorted(np.cumsum(c[:, 0]), positions))
    assert 0 < cut < len(c), (cut, len(c))
    return _edged(c[:cut], ncol=c.shape[1])


def _alt(positions, long_span=64, long_keys=((0, 0, N),)):
    """Hand-built rows: a span-1 row of key (0, 1, N), then a row of `long_span` positions whose key cycles through long_keys."""
    pairs = positions // (1 + long_span)
    c = np.zeros((2 * pairs, 4), dtype=np.int32)
    c[0::2, 0] = 1; c[0::2, 1:] = (0, 1, N)
    c[1::2, 0] = long_span
    lk = np.asarray(long_keys, dtype=np.int32)
    c[1::2, 1:] = lk[np.arange(pairs) % len(lk)]
    return [_edged(c)]


def _unbinned(eigen_keys):
    """3 000 un-binned rows (spans up to 1e5) whose span > 1 rows hold `eigen_keys` distinct keys."""
    from smcpp_amd import synth
    c = synth.synth_posterior_contig(3000, N, seed=31).copy()
    long_rows = np.nonzero(c[:, 0] > 1)[0]
    if eigen_keys == 1:
        c[long_rows, 1:] = (0, 0, N)
    for j in range(2, eigen_keys):                     # (the generator gives two: monomorphic and missing)
        c[long_rows[j::7], 1:] = (0, 0, N - j + 1)
    return [_edged(c)]


def build_input(name):
    """-> dict(n, na, contigs, M, theta, rho); n / na are tuples (one entry per population)."""
    one = dict(n=(N,), na=(2,), theta=TH_B, rho=RH_B)
    if name == "one_chunk":
        # 1 500 rows, 2 000 positions (below twice the 1 024-position floor): the first 500 span > 1 rows keep two positions
        c = _rows(1, 40_000, 64)[:1500].copy()
        c[:, 0] = np.minimum(c[:, 0], 2)
        c[np.nonzero(c[:, 0] > 1)[0][500:], 0] = 1
        return dict(one, M=16, contigs=[_edged(c)])
    if name in ("A64", "A32"):
        # tests/test_gpu_seams.py's input A: 58 chunks at the 1 024-position floor on the first contig
        return dict(one, M=int(name[1:]), contigs=[_rows(101, 60_000, 64), _rows(102, 2_500, 64), _rows(103, 6_000, 64), _rows(104, 1_100, 64)] + _tiny(64))
    if name.startswith("size_"):
        return dict(one, M=64, contigs=_alt(int(float(name[5:]) * 1e6)))
    if name.startswith("B"):
        return dict(one, M=int(name[1:]), contigs=[_rows(111, 30_000, 300, stretch=4)] + _tiny(300))
    if name.startswith("hyb"):
        ke = int(name[3:])
        return dict(one, M=32 if ke == 1 else 64, contigs=_unbinned(ke), theta=TH_U, rho=RH_U)
    if name == "twopop_many_keys":
        c = _rows(121, 100_000, 64, twopop=(10, 10))          # 125 keys
        return dict(n=(10, 10), na=(2, 0), theta=TH_B, rho=RH_B, M=48, contigs=[c])
    if name == "one_eigen_key":
        return dict(one, M=64, contigs=_alt(300_000))
    if name == "two_eigen_keys":
        return dict(one, M=64, contigs=_alt(300_000, long_keys=((0, 0, N), (0, 0, N - 1))))
    if name == "short_spans":
        return dict(one, M=64, contigs=_alt(300_000, long_span=4))
    raise KeyError(name)


# ---- cases: id -> (input, switches, steps) -------------------------------------------------------------------------------------
# steps: what happens between construction and the record; ("chunking", r) = set_chunking(r), "warm" = set_warm_start(True),
# "estep" = one E-step.  The record is taken at the end (a case with two E-steps records after each: "second").
def _case(inp, env=None, steps=("estep",)):
    return dict(input=inp, env=dict(env or {}), steps=tuple(steps))


CASES = {"one_chunk": _case("one_chunk"), "chunks58": _case("A64")}
for _s in ("1.0", "1.5", "2.5", "13"):
    CASES[f"size_{_s}M"] = _case(f"size_{_s}")
CASES["size_2.5M_wpc2"] = _case("size_2.5", {"SMCPP_SS_WPC": "2"})
for _m in (100, 256, 300, 600):
    CASES[f"M{_m}"] = _case(f"B{_m}")
    CASES[f"M{_m}_halo0"] = _case(f"B{_m}", {"SMCPP_SS_HALO": "0"})
    CASES[f"M{_m}_halo1"] = _case(f"B{_m}", {"SMCPP_SS_HALO": "1"})
    CASES[f"M{_m}_halo_lengths"] = _case(f"B{_m}", {"SMCPP_HALO_LF": "1500", "SMCPP_HALO_DF": "400", "SMCPP_HALO_LB": "2000", "SMCPP_HALO_DB": "600"})
    CASES[f"M{_m}_share0.3"] = _case(f"B{_m}", {"SMCPP_SS_FWD_SHARE": "0.3"})
    CASES[f"M{_m}_share0.03"] = _case(f"B{_m}", {"SMCPP_SS_FWD_SHARE": "0.03"})
for _k in (1, 2, 4):
    CASES[f"hyb{_k}"] = _case(f"hyb{_k}")
    CASES[f"hyb{_k}_off"] = _case(f"hyb{_k}", {"SMCPP_HYBRID": "0"})
    CASES[f"hyb{_k}_th3"] = _case(f"hyb{_k}", {"SMCPP_HYB_TH": "3"})
    CASES[f"hyb{_k}_wpc2"] = _case(f"hyb{_k}", {"SMCPP_SS_WPC": "2"})
CASES.update({
    "keys_beyond_lds": _case("twopop_many_keys", {"SMCPP_SS_WPC": "3"}),
    "M32_two_row_scans": _case("A32"),
    "M32_h32_off": _case("A32", {"SMCPP_SS_H32": "0"}),
    "dense_M16": _case("one_chunk", {"SMCPP_CHAIN": "dense"}),
    "dense_M64": _case("A64", {"SMCPP_CHAIN": "dense"}),
    "dense_M64_bpc3": _case("A64", {"SMCPP_CHAIN": "dense", "SMCPP_COOP_BPC": "3"}),
    "dense_M100": _case("B100", {"SMCPP_CHAIN": "dense"}),
    "ss_off": _case("A64", {"SMCPP_SS": "0"}),
    "lock": _case("A64", {"SMCPP_CHAIN": "lock"}),
    "lock_auto_one_key": _case("one_eigen_key", {"SMCPP_SS": "0", "SMCPP_LOCK_MIN_ROWS": "1"}),
    "lock_auto_no_dominant_key": _case("two_eigen_keys", {"SMCPP_SS": "0", "SMCPP_LOCK_MIN_ROWS": "1"}),
    "rows_per_chunk700": _case("A64", {"SMCPP_ROWS_PER_CHUNK": "700"}),
    "set_chunking300": _case("A64", steps=(("chunking", 300), "estep")),
    "set_chunking300_back0": _case("A64", steps=(("chunking", 300), ("chunking", 0), "estep")),
    "dense_M64_prepass_off": _case("A64", {"SMCPP_CHAIN": "dense", "SMCPP_POWER_PREPASS": "0"}),
    "dense_M64_long_chunks": _case("A64", {"SMCPP_CHAIN": "dense", "SMCPP_ROWS_PER_CHUNK": "2500"}),
    "jump_small_unset": _case("A64"),
    "jump_large_unset": _case("one_eigen_key"),
    "jump0": _case("one_eigen_key", {"SMCPP_SS_JUMP": "0"}),
    "jump16": _case("A64", {"SMCPP_SS_JUMP": "16"}),
    "jump5": _case("A64", {"SMCPP_SS_JUMP": "5"}),
    "jump_saves_little": _case("short_spans", {"SMCPP_SS_JUMP": "8"}),
    "mixed_off": _case("A64", {"SMCPP_SS_MIXED": "0"}),
    "light_2_1": _case("A64", {"SMCPP_SS_LIGHT_F": "2", "SMCPP_SS_LIGHT_B": "1"}),
    "cert_pass": _case("A64", {"SMCPP_SS_CERT_PASS": "1"}),
    "warm_start": _case("A64", steps=("warm", "estep", "estep")),
})
# the cases a real manager is held to in tests/test_chain_plan.py (the warm start's second E-step exists on the device only)
GPU_SAMPLE = ["one_chunk", "chunks58", "M100", "hyb2", "dense_M64", "lock", "warm_start"]


# ---- one case -------------------------------------------------------------------------------------------------------------------
def chunk_digest(ch):
    ch = np.ascontiguousarray(ch, dtype=np.int32).reshape(-1, 5)
    return {"n": int(len(ch)), "crc": int(zlib.crc32(ch.tobytes()) & 0xFFFFFFFF), "first": ch[:3].tolist(), "last": ch[-3:].tolist()}


def manager(inp):
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    a, s = synth.model_pieces()
    hs = synth.hidden_states(inp["M"])
    if len(inp["n"]) == 1:
        im = _smcpp.PyOnePopInferenceManager(inp["n"][0], inp["contigs"], hs, ("pop1",), 0.5)
        im.model = PiecewiseModel(a, s, 1e4, "pop1")
    else:
        im = _smcpp.PyTwoPopInferenceManager(*inp["n"], *inp["na"], inp["contigs"], hs, ("pop1", "pop2"), 0.5)
        im.model = TwoPopulationModel(PiecewiseModel(a, s, 1e4, pid="pop1"),
                                      PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(8)), s[:8], 1e4, pid="pop2"), 0.3)
    im.theta = inp["theta"]; im.rho = inp["rho"]; im.alpha = 1.0
    return im


def snapshot(im):
    d = im.describe()
    return {"plan": d["plan"], "chain_mode": im.chain_mode(),            # ("power_jumps" is an object inside "plan")
            "chunks_forward": chunk_digest(im.chunks(False)), "chunks_backward": chunk_digest(im.chunks(True))}


def run_case(cid, set_option):
    """Sets the case's switches through set_option(name, value), runs its steps on a fresh manager; -> the record."""
    case = CASES[cid]
    for k, v in case["env"].items():
        set_option(k, v)
    try:
        im = manager(build_input(case["input"]))
        rec, esteps = None, 0
        for st in case["steps"]:
            if st == "warm":
                im.set_warm_start(True)
            elif st == "estep":
                im.E_step()
                esteps += 1
                if esteps == 1:
                    rec = snapshot(im)
                else:
                    rec["second"] = snapshot(im)
            else:
                im.set_chunking(st[1])
        del im
        return rec
    finally:
        for k in case["env"]:
            set_option(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "chain_plans.json"))
    args = ap.parse_args()
    if args.case:
        from smcpp_amd import _engine
        print("RECORD " + json.dumps(run_case(args.case, _engine.set_option)), flush=True)
        return 0
    import torch
    table = {"compute_units": int(torch.cuda.get_device_properties(0).multi_processor_count), "cases": {}}
    for cid in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", cid], capture_output=True, text=True, timeout=240)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            # nothing more is started on the device behind a case that failed
            print(f"case {cid} failed with exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1
        table["cases"][cid] = json.loads(lines[-1][7:])
        p = table["cases"][cid]["plan"]
        print(f"{cid}: family {table['cases'][cid]['chain_mode']}, {p['chunks_forward']} / {p['chunks_backward']} chunks", flush=True)
    write_table(table, args.out)
    print(f"wrote {args.out}: {len(table['cases'])} cases", flush=True)
    return 0


def write_table(table, path):
    """One case per line, no padding: the file stays well under 100 KB."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"compute_units":%d,"cases":{\n' % table["compute_units"])
        f.write(",\n".join(f"{dumps(cid)}:{dumps(rec)}" for cid, rec in table["cases"].items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    sys.exit(main())
