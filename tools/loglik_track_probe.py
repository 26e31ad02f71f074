"""What the log-likelihood track costs beside the E-step and the exact posterior windows of the same run.

The inputs of tools/posterior_positions_probe.py, one manager each, in one process:

  posterior64     the input of `bench.py --workload posterior64` cut to --rows rows: M = 64, n = 8, un-binned (`synth_posterior_contig`)
  binned100M_M64  the binned 100 Mbp contig at M = 64, n = 20 (rows of 100 bp bins)
  binned100M_M256 the same contig at M = 256, n = 50

Per input: two `save_gamma` E-steps to settle (the exact posterior windows need one; the track does not), then `--repeats` rounds
after `--warmup` of (a) the E-step, wall clock up to the log-likelihood on the host, (b) `posterior_windows_exact(0, W)`,
(c) `loglik_windows(0, W)`, (d) `loglik_positions(0, step=--grid)`, (e) `loglik_rows(0)`; every call ends in a device synchronise and
a copy to the host.  Reported per leg: the minimum, the median and the spread (max - min); the launch shape of (c) and (d) (`ll_items`,
`ll_waves`, `ll_walk_worst_ratio`; read once, outside the timed rounds), the ratio (c) / (b), and how far the windows' sum lies from the E-step's log-likelihood.
One JSON line per input, to stdout and appended to --out.

    python tools/loglik_track_probe.py [--rows N] [--repeats K] [--warmup W] [--window BP] [--grid STEP] [--only NAME] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000, help="rows of the posterior64 input")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik_track.log"))
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
        if not args.only:                  # (a run of one input appends its line)
            open(args.out, "w").close()
    for name, make in inputs.items():
        if args.only and name != args.only:
            continue
        M, n, contig, theta, rho = make()
        hs = synth.hidden_states(M)
        im = _smcpp.PyOnePopInferenceManager(n, [contig], hs, ("pop1",), 0.5, device=0)
        im.model = PiecewiseModel(a, s_, 1e4, pid="pop1")
        im.theta = theta; im.rho = rho; im.alpha = 1.0
        im.save_gamma = True
        im.E_step()
        im.E_step()
        im.loglik()

        def estep():
            im.E_step()
            return im.loglik()

        legs = {"estep_save_gamma": estep, "posterior_windows_exact": lambda: im.posterior_windows_exact(0, args.window),
                "loglik_windows": lambda: im.loglik_windows(0, args.window), "loglik_positions": lambda: im.loglik_positions(0, step=args.grid),
                "loglik_rows": lambda: im.loglik_rows(0)}
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= args.warmup:
                    times[k].append(dt)
        # the launch shape of the two walking calls, taken once, outside the timed rounds
        shape = {}
        for key in ("loglik_windows", "loglik_positions"):
            n_out = len(legs[key]())
            d = im.describe()
            shape[key] = {"outputs": int(n_out), "items": d["ll_items"], "waves": d["ll_waves"], "walk_worst_ratio": d["ll_walk_worst_ratio"]}
        ll = float(im.logliks()[0])
        off = abs(float(im.loglik_windows(0, args.window).sum()) - ll) / abs(ll)
        plan = im.describe()["plan"]
        best = {k: min(v) for k, v in times.items()}
        res = {"input": name, "M": M, "rows": len(contig), "positions": int(contig[:, 0].astype(np.int64).sum()),
               "longest_row": int(contig[:, 0].max()), "window": args.window, "grid": args.grid, "repeats": args.repeats,
               "plan": {k: plan[k] for k in ("chain_family", "states_per_lane", "long_rows_cut", "hybrid_rows")},
               "launch": shape,
               "loglik_windows_over_windows_exact": round(best["loglik_windows"] / best["posterior_windows_exact"], 3),
               "loglik_windows_over_estep": round(best["loglik_windows"] / best["estep_save_gamma"], 3),
               "windows_sum_off_loglik_rel": off,
               "legs": {k: {"min_ms": round(min(v), 3), "median_ms": round(float(np.median(v)), 3), "spread_ms": round(max(v) - min(v), 3)}
                        for k, v in times.items()}}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del im


if __name__ == "__main__":
    main()
