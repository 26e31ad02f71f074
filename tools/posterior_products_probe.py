"""What the user waits for after a posterior E-step: the matrix as it is fetched today against the device-side products.

Input of `bench.py --workload posterior64` (the same `synth_posterior_contig` call and parameters: M = 64, n = 8, 10^6 un-binned
rows).  One `save_gamma` E-step, then the legs, alternating, `--repeats` times after `--warmup` rounds; wall clock around calls that
end in a device synchronise (every leg copies its result to the host).  Reported per leg: the minimum and the spread (max - min).

  leg A   `im.gammas[0]` followed by the numpy normalisation - the matrix product as `posterior()` forms it
  leg B   `posterior_columns` in fp64 / in fp32
  leg C   `posterior_summary` with weights (average coalescence times) and three levels
  leg D   `posterior_windows` at W = 10^4

A build without the products (a checkout of an older commit given with --root) reports legs B - D as "absent"; leg A there is the
baseline.  `sha256_A` is the digest of leg A's un-normalised matrix: equal between two builds = the same bits.

    python tools/posterior_products_probe.py [--root DIR] [--rows N] [--repeats K] [--warmup W] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose smcpp_amd is measured")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from smcpp_amd import _engine, _smcpp, synth
    from smcpp_amd.model import PiecewiseModel

    M, n = 64, 8
    hs = synth.hidden_states(M)
    a, s_ = synth.model_pieces()
    theta, rho, alpha, pol = 1e-4 * 2, 6e-5, 1.0, 0.5
    contig = synth.synth_posterior_contig(args.rows, n, seed=7)
    im = _smcpp.PyOnePopInferenceManager(n, [contig], hs, ("pop1",), pol, device=0)
    im.model = PiecewiseModel(a, s_, 1e4, pid="pop1")
    im.theta = theta; im.rho = rho; im.alpha = alpha
    im.save_gamma = True
    im.E_step()
    im.E_step()
    estep_ms = im.last_timing()
    have = hasattr(im, "posterior_columns")
    _, w = _engine.host_rate_function(a, s_, [0.0], hs=hs)
    digest = {}

    def leg_a():
        g = im.gammas[0]
        if "A" not in digest:
            digest["A"] = hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest()
        return g / g.sum(axis=0, keepdims=True)

    legs = {"A_gammas_then_numpy_normalise": leg_a}
    if have:
        legs["B_columns_fp64"] = lambda: im.posterior_columns(0)
        legs["B_columns_fp32"] = lambda: im.posterior_columns(0, dtype=np.float32)
        legs["C_summary_weights_3_levels"] = lambda: im.posterior_summary(0, weights=w, quantiles=(0.025, 0.5, 0.975))
        legs["D_windows"] = lambda: im.posterior_windows(0, args.window)
    times = {k: [] for k in legs}
    shapes = {}
    for r in range(args.warmup + args.repeats):
        for k, f in legs.items():
            t0 = time.perf_counter()
            out = f()
            dt = 1e3 * (time.perf_counter() - t0)
            shapes[k] = list(out.shape) if hasattr(out, "shape") else sorted(out)
            del out
            if r >= args.warmup:
                times[k].append(dt)
    res = {"root": os.path.abspath(args.root), "M": M, "rows": len(contig), "base_pairs": int(contig[:, 0].astype(np.int64).sum()),
           "window": args.window, "repeats": args.repeats, "estep_timing": {k: round(float(v), 3) for k, v in estep_ms.items()},
           "sha256_A": digest["A"], "legs": {}}
    for k, v in times.items():
        res["legs"][k] = {"min_ms": round(min(v), 3), "spread_ms": round(max(v) - min(v), 3), "all_ms": [round(x, 3) for x in v],
                          "result": shapes[k]}
    if not have:
        for k in ("B_columns_fp64", "B_columns_fp32", "C_summary_weights_3_levels", "D_windows"):
            res["legs"][k] = "absent"
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
