"""What the per-position posterior products cost beside the E-step and the per-row products they follow.

Three inputs, one manager each, in one process:

  posterior64     the input of `bench.py --workload posterior64` cut to --rows rows: M = 64, n = 8, un-binned (`synth_posterior_contig`)
  binned100M_M64  the binned 100 Mbp contig of tools/posterior_transitions_probe.py at M = 64, n = 20 (rows of 100 bp bins)
  binned100M_M256 the same contig at M = 256, n = 50

Per input: two `save_gamma` E-steps to settle, then `--repeats` rounds after `--warmup` of (a) the `save_gamma` E-step, wall clock up
to the log-likelihood on the host, (b) `posterior_transitions(0)`, (c) `posterior_windows(0, W)`, (d) `posterior_position_summary` on
a grid of every --grid-th position (argmax, mean, three quantile states), (e) `posterior_windows_exact(0, W)`; every call ends in a
device synchronise and a copy to the host.  Reported per leg: the minimum and the spread (max - min); the launch shape of (d) and (e)
(`position_waves`, `position_rows_walked`), the ratios (d) / (b) and (e) / (c), and how far the two window products lie apart.
One JSON line per input, to stdout and appended to --out.

    python tools/posterior_positions_probe.py [--rows N] [--repeats K] [--warmup W] [--window BP] [--grid STEP] [--only NAME] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_positions.log"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    from smcpp_amd.posterior import average_coal_times

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
        hs = synth.hidden_states(M)
        model = PiecewiseModel(a, s_, 1e4, pid="pop1")
        im = _smcpp.PyOnePopInferenceManager(n, [contig], hs, ("pop1",), 0.5, device=0)
        im.model = model
        im.theta = theta; im.rho = rho; im.alpha = 1.0
        im.save_gamma = True
        im.E_step()
        im.E_step()
        im.loglik()
        w = average_coal_times(model, hs)

        def estep():
            im.E_step()
            return im.loglik()

        shape = {}

        def summary():
            r = im.posterior_position_summary(0, weights=w, quantiles=(0.025, 0.5, 0.975), step=args.grid)
            d = im.describe()
            shape["summary"] = {"positions": len(r["argmax"]), "waves": d["position_waves"], "rows_walked": d["position_rows_walked"]}
            return r

        def exact():
            r = im.posterior_windows_exact(0, args.window)
            d = im.describe()
            shape["windows_exact"] = {"windows": r.shape[1], "waves": d["position_waves"], "rows_walked": d["position_rows_walked"]}
            return r

        legs = {"estep_save_gamma": estep, "posterior_transitions": lambda: im.posterior_transitions(0),
                "posterior_windows": lambda: im.posterior_windows(0, args.window), "posterior_position_summary": summary,
                "posterior_windows_exact": exact}
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= args.warmup:
                    times[k].append(dt)
        apart = np.abs(im.posterior_windows_exact(0, args.window) - im.posterior_windows(0, args.window)).max(axis=0)
        plan = im.describe()["plan"]
        best = {k: min(v) for k, v in times.items()}
        res = {"input": name, "M": M, "rows": len(contig), "positions": int(contig[:, 0].astype(np.int64).sum()),
               "longest_row": int(contig[:, 0].max()), "window": args.window, "grid": args.grid, "repeats": args.repeats,
               "plan": {k: plan[k] for k in ("chain_family", "states_per_lane", "long_rows_cut", "per_row_gamma")},
               "launch": shape,
               "summary_over_transitions": round(best["posterior_position_summary"] / best["posterior_transitions"], 3),
               "windows_exact_over_windows": round(best["posterior_windows_exact"] / best["posterior_windows"], 3),
               "windows_apart_max": float(apart.max()), "windows_apart_median": float(np.median(apart)),
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
