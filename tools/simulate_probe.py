"""What drawing whole data sets from the model costs.

One `Simulator` (smcpp_amd/simulate.py) at M = 64, n = 8, theta = 2e-4 and rho = 6e-5 per base pair (the un-binned figures of the
tests), the synthetic model; 22 contigs of the C3 lengths (47 - 248 Mbp, 2.87e9 positions per replicate) x {1, 16, 128} replicates.
Per replicate count, `--repeats` calls of `im.simulate` after `--warmup`: wall clock including every resumed device call and every
copy to the host (the events of all (contig, replicate) pairs of a device call are capped at 2^24, so a data set takes several).
Reported: the median, the minimum and the spread (max - min) of the wall clock, the events drawn, the device calls, microseconds per
event of the LONGEST (contig, replicate) pair - the dependent chain a wavefront walks, three draws per event - and nanoseconds per
event over all pairs.  One JSON line per replicate count, to stdout and appended to --out.

    python tools/simulate_probe.py [--repeats K] [--warmup W] [--scale F] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLICATES = (1, 16, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0, help="factor on the contig lengths")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate.log"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from smcpp_amd import simulate, synth
    from smcpp_amd.model import PiecewiseModel

    a, s_ = synth.model_pieces()
    M, n, theta, rho = 64, 8, 2e-4, 6e-5
    sim = simulate.Simulator(PiecewiseModel(a, s_, 1e4, pid="pop1"), n, synth.hidden_states(M), theta, rho, device=0)
    lengths = [max(1, int(x * 1_000_000 * args.scale)) for x in synth.C3_LENGTHS_MBP]
    pi, T, E = sim.tables()
    rate = simulate.event_rate(T, E, np.arange(len(E)), sim.quiet_entry)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()
    for R in REPLICATES:
        times, ev = [], None
        for r in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            ev = sim.events(lengths, R, args.seed)
            dt = time.perf_counter() - t0
            if r >= args.warmup:
                times.append(dt)
        counts = np.array([[len(p) for p in c] for c in ev["pos"]], dtype=np.int64)
        med = statistics.median(times)
        d = sim.im.describe()
        res = {"M": M, "n": n, "alphabet": len(sim.alphabet), "theta": theta, "rho": rho, "contigs": len(lengths),
               "positions_per_replicate": int(sum(lengths)), "replicates": R, "pairs": int(counts.size),
               "max_loud_share_of_a_position": rate, "events": int(counts.sum()), "events_of_the_longest_pair": int(counts.max()),
               "device_calls": int(ev["calls"]), "wavefronts_of_the_last_call": d["simulate_waves"],
               "repeats": args.repeats, "warmup": args.warmup,
               "wall_s": {"median": round(med, 4), "min": round(min(times), 4), "spread": round(max(times) - min(times), 4),
                          "all": [round(x, 4) for x in times]},
               "us_per_event_of_the_longest_pair": round(1e6 * med / max(1, int(counts.max())), 4),
               "ns_per_event_over_all_pairs": round(1e9 * med / max(1, int(counts.sum())), 3)}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
