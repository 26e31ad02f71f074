"""What sampled posterior paths cost beside the E-step they follow.

Three inputs, one manager each, in one process (those of tools/posterior_transitions_probe.py):

  posterior64     the input of `bench.py --workload posterior64`: M = 64, n = 8, `--rows` un-binned rows (`synth_posterior_contig`;
                  10^6 rows are 4.8e8 positions - a path is that many DEPENDENT draws, so the default here is 10^4 rows)
  binned100M_M64  the binned 100 Mbp contig of tools/gamma_scan_probe.py at M = 64, n = 20 (235 552 rows, 10^6 positions)
  binned100M_M256 the same contig at M = 256, n = 50

Per input: two `save_gamma` E-steps to settle, then `--repeats` rounds after `--warmup` of (a) the `save_gamma` E-step, wall clock up
to the log-likelihood on the host, (b) `posterior_transitions(0)`, (c) `posterior_sample_rows(0, K)` for K = 1, 16, 256; every call
ends in a device synchronise and a copy to the host.  Reported per leg: the median, the minimum and the spread (max - min); for the
sampler also nanoseconds per draw and path, the paths per wavefront the host chose, and the ratio of 256 paths to 1 path (256 would
be the cost of 256 calls; what is below it is what the parallelism over paths buys).  The mean number of breakpoints of the 256
paths beside the expected count (up + down of `posterior_transitions`) is a sanity line.  One JSON line per input, to stdout and
appended to --out.

    python tools/posterior_paths_probe.py [--rows N] [--repeats K] [--warmup W] [--only NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = (1, 16, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000, help="rows of the posterior64 input")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_paths.log"))
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
        positions = int(contig[:, 0].astype(np.int64).sum()) + 1

        def estep():
            im.E_step()
            return im.loglik()

        legs = {"estep_save_gamma": estep, "posterior_transitions": lambda: im.posterior_transitions(0)}
        for K in PATHS:
            legs[f"sample_rows_{K}"] = lambda K=K: im.posterior_sample_rows(0, K, args.seed)
        times = {k: [] for k in legs}
        batch = {}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                dt = 1e3 * (time.perf_counter() - t0)
                if r >= args.warmup:
                    times[k].append(dt)
                if k.startswith("sample_rows_"):
                    batch[k] = im.describe()["path_batch"]
        t = im.posterior_transitions(0)
        pr = im.posterior_sample_rows(0, 256, args.seed)
        breaks = (pr["up"].astype(np.int64) + pr["down"]).sum(axis=1)
        plan = im.describe()["plan"]
        med = {k: statistics.median(v) for k, v in times.items()}
        res = {"input": name, "M": M, "rows": len(contig), "positions": positions, "longest_row": int(contig[:, 0].max()),
               "repeats": args.repeats, "warmup": args.warmup,
               "plan": {k: plan[k] for k in ("chain_family", "states_per_lane", "long_rows_cut", "per_row_gamma")},
               "expected_breakpoints": float(t["up"].sum() + t["down"].sum()),
               "mean_breakpoints_of_256_paths": float(breaks.mean()), "se_of_the_mean": float(breaks.std(ddof=1) / 16.0),
               "legs": {k: {"median_ms": round(med[k], 3), "min_ms": round(min(v), 3), "spread_ms": round(max(v) - min(v), 3),
                            "all_ms": [round(x, 3) for x in v]} for k, v in times.items()},
               "ns_per_draw_and_path": {str(K): round(1e6 * med[f"sample_rows_{K}"] / (positions * K), 3) for K in PATHS},
               "paths_per_wavefront": {str(K): batch[f"sample_rows_{K}"] for K in PATHS},
               "ratio_256_paths_to_1": round(med["sample_rows_256"] / med["sample_rows_1"], 3)}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del im


if __name__ == "__main__":
    main()
