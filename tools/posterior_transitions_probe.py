"""What the posterior transition products cost beside the E-step they follow.

Three inputs, one manager each, in one process:

  posterior64     the input of `bench.py --workload posterior64`: M = 64, n = 8, 10^6 un-binned rows (`synth_posterior_contig`)
  binned100M_M64  the binned 100 Mbp contig of tools/gamma_scan_probe.py at M = 64, n = 20 (235 552 rows of 100 bp bins)
  binned100M_M256 the same contig at M = 256, n = 50

Per input: two `save_gamma` E-steps to settle, then `--repeats` rounds after `--warmup` of (a) the `save_gamma` E-step, wall clock up
to the log-likelihood on the host, (b) `posterior_transitions(0)`, (c) `posterior_transition_windows(0, W)`; both calls end in a
device synchronise and a copy to the host.  Reported per leg: the minimum and the spread (max - min); the sums over the rows beside the
trace and triangle sums of the contig's xisum as a sanity line.  One JSON line per input, to stdout and appended to --out.

    python tools/posterior_transitions_probe.py [--rows N] [--repeats K] [--warmup W] [--window BP] [--only NAME] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the posterior64 input")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_transitions.log"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel

    a, s_ = synth.model_pieces()

    def posterior64():
        return 64, 8, synth.synth_posterior_contig(args.rows, 8, seed=7), 2e-4, 6e-5

    def binned(M, n):
        return lambda: (M, n, np.ascontiguousarray(synth.synth_contig(0, 100_000_000, n), dtype=np.int32), synth.THETA, synth.RHO)

    inputs = {"posterior64": posterior64, "binned100M_M64": binned(64, 20), "binned100M_M256": binned(256, 50)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for name, make in inputs.items():
        if args.only and name != args.only:
            continue
        M, n, contig, theta, rho = make()
        im = _smcpp.PyOnePopInferenceManager(n, [contig], synth.hidden_states(M), ("pop1",), 0.5, device=0)
        im.model = PiecewiseModel(a, s_, 1e4, pid="pop1")
        im.theta = theta; im.rho = rho; im.alpha = 1.0
        im.save_gamma = True
        im.E_step()
        im.E_step()
        im.loglik()

        def estep():
            im.E_step()
            return im.loglik()

        legs = {"estep_save_gamma": estep, "posterior_transitions": lambda: im.posterior_transitions(0),
                "posterior_transition_windows": lambda: im.posterior_transition_windows(0, args.window)}
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= args.warmup:
                    times[k].append(dt)
        t = im.posterior_transitions(0)
        X = im.xisums[0]
        plan = im.describe()["plan"]
        res = {"input": name, "M": M, "rows": len(contig), "base_pairs": int(contig[:, 0].astype(np.int64).sum()),
               "longest_row": int(contig[:, 0].max()), "window": args.window, "repeats": args.repeats,
               "plan": {k: plan[k] for k in ("chain_family", "states_per_lane", "long_rows_cut", "per_row_gamma")},
               "sum_stay_up_down": [float(t[k].sum()) for k in ("stay", "up", "down")],
               "xisum_trace_upper_lower": [float(np.trace(X)), float(np.triu(X, 1).sum()), float(np.tril(X, -1).sum())],
               "legs": {k: {"min_ms": round(min(v), 3), "spread_ms": round(max(v) - min(v), 3), "all_ms": [round(x, 3) for x in v]}
                        for k, v in times.items()}}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del im


if __name__ == "__main__":
    main()
