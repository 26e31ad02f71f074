"""What the score track costs, in both forms of its row walk, beside the `save_gamma` E-step and the posterior transition products
of the same run.

Three inputs, one manager each, in one process, the model differentiable in every piece (16 directions):

  binned100M_M64   the binned 100 Mbp contig at M = 64, n = 20 (rows of 100 bp bins): short rows, the per-row contraction dominates
  posterior64      the input of `bench.py --workload posterior64` cut to --rows rows: M = 64, n = 8, un-binned
                   (`synth_posterior_contig`): rows of up to 10^5 positions, the walk dominates
  binned100M_M256  the binned contig at M = 256 (four states per lane): the vectors form alone, the matrix form stops at 64 states

Per input: two `save_gamma` E-steps to settle, then `--repeats` rounds after `--warmup` of (a) the E-step (with its 16-direction
preparation), wall clock up to the log-likelihood on the host, (b) `posterior_transitions(0)`, and per form (SMCPP_SCORE_FORM set
through `_engine.set_option` around the leg) (c) `score_rows(0)`, (d) `score_rows(0, parts=True)`, (e) `score_windows(0, W)`, in
the vectors form also (f) `score_windows_exact(0, W)` - the windows exact on rows a boundary cuts - and, at M <= 64, its neighbours
`posterior_windows_exact(0, W)` and `loglik_windows(0, W)` as yardsticks; every call ends in a device synchronise and a copy to the
host.  The forms alternate inside every round, so they see the same machine.  The
first score call of a form behind an E-step also builds and uploads its tables; it is timed apart as `first_call_ms`.  Reported per
leg: the minimum, the median and the spread (max - min); per form the launch shape (`score_items`, `score_waves`, `score_park`; read
once, outside the timed rounds), the ratios of (c) to (b), to (a) and to the matrix form's (c) of the same run, and how far the
score's sum lies from Q's gradient; for the exact windows the rows a boundary cut (`score_exact_items`), their segments and the
wavefronts of the segment walk (0: it was not launched), and the ratio of (f) to (e) of the same run.  One JSON line per input, to stdout and appended to --out.

    python tools/score_track_probe.py [--rows N] [--repeats K] [--warmup W] [--window BP] [--only NAME] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_track.log"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel

    a, s_ = synth.model_pieces()

    def posterior64():
        return 64, 8, synth.synth_posterior_contig(args.rows, 8, seed=7), 2e-4, 6e-5

    def binned(M):
        return lambda: (M, 20, np.ascontiguousarray(synth.synth_contig(0, 100_000_000, 20), dtype=np.int32), synth.THETA, synth.RHO)

    from smcpp_amd import _engine
    inputs = {"binned100M_M64": binned(64), "posterior64": posterior64, "binned100M_M256": binned(256)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if not args.only:                  # (a run of one input appends its line)
            open(args.out, "w").close()
    for name, make in inputs.items():
        if args.only and name != args.only:
            continue
        M, n, contig, theta, rho = make()
        im = _smcpp.PyOnePopInferenceManager(n, [contig], synth.hidden_states(M), ("pop1",), 0.5, device=0)
        model = PiecewiseModel(a, s_, 1e4, pid="pop1")
        model.differentiable = True
        im.model = model
        im.theta = theta; im.rho = rho; im.alpha = 1.0
        im.save_gamma = True
        im.E_step()
        im.E_step()
        im.loglik()
        forms = ("matrix", "vectors") if M <= 64 else ("vectors",)

        def in_form(form, f):
            def call():
                _engine.set_option("SMCPP_SCORE_FORM", form)
                try:
                    return f()
                finally:
                    _engine.set_option("SMCPP_SCORE_FORM", None)
            return call

        first = {}
        for form in forms:
            t0 = time.perf_counter()
            in_form(form, lambda: im.score_rows(0))()
            first[form] = 1e3 * (time.perf_counter() - t0)

        legs = {"estep_save_gamma": None, "posterior_transitions": lambda: im.posterior_transitions(0)}
        for form in forms:
            legs[form + ":score_rows"] = in_form(form, lambda: im.score_rows(0))
            legs[form + ":score_rows_parts"] = in_form(form, lambda: im.score_rows(0, parts=True))
            legs[form + ":score_windows"] = in_form(form, lambda: im.score_windows(0, args.window))
        legs["vectors:score_windows_exact"] = in_form("vectors", lambda: im.score_windows_exact(0, args.window))
        if M <= 64:
            legs["posterior_windows_exact"] = lambda: im.posterior_windows_exact(0, args.window)
            legs["loglik_windows"] = lambda: im.loglik_windows(0, args.window)
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.repeats):
            for k, f in legs.items():
                t0 = time.perf_counter()
                if f is None:
                    im.E_step()
                    im.loglik()
                else:
                    f()
                dt = 1e3 * (time.perf_counter() - t0)
                if f is None:
                    for form in forms:      # (the tables of this E-step: built here, outside the score legs)
                        in_form(form, lambda: im.score_rows(0, 0, 1))()
                if r >= args.warmup:
                    times[k].append(dt)
        _, jac = im.Q_with_gradient()
        m0 = float(im.posterior_columns(0, 0, 1, normalize=False).sum())       # (Q weighs log pi with the stored, unnormalised column 0)
        want = np.stack([jac[0] / m0, jac[1] + jac[2], jac[3]])
        best = {k: min(v) for k, v in times.items()}
        per_form = {}
        for form in forms:
            rows = in_form(form, lambda: im.score_rows(0, parts=True))()
            d = im.describe()               # (the launch shape of the last score call; the route of the Q behind it)
            per_form[form] = {
                "launch": {"score_items": d["score_items"], "score_waves": d["score_waves"], "score_park": d["score_park"], "score_form": d["score_form"]},
                "first_call_ms": round(first[form], 3),
                "score_rows_over_posterior_transitions": round(best[form + ":score_rows"] / best["posterior_transitions"], 3),
                "score_rows_over_estep": round(best[form + ":score_rows"] / best["estep_save_gamma"], 3),
                "score_rows_over_matrix_form": round(best[form + ":score_rows"] / best["matrix:score_rows"], 3) if "matrix" in forms else None,
                "parts_sum_off_q_jacobian_rel": float(np.max(np.abs(rows.sum(axis=2) - want) / np.maximum(np.abs(rows).sum(axis=2), 1e-300)))}
        exact = in_form("vectors", lambda: im.score_windows_exact(0, args.window))()
        d = im.describe()
        plain = in_form("vectors", lambda: im.score_windows(0, args.window))()
        per_form["vectors"]["exact_windows"] = {
            "score_exact_items": d["score_exact_items"], "score_exact_segments": d["score_exact_segments"], "score_exact_waves": d["score_exact_waves"],
            "exact_over_score_windows": round(best["vectors:score_windows_exact"] / best["vectors:score_windows"], 3),
            "max_abs_exact_minus_apportioned": float(np.max(np.abs(exact - plain))), "max_abs_window": float(np.max(np.abs(exact)))}
        plan = d["plan"]
        res = {"input": name, "M": M, "directions": int(rows.shape[1]), "rows": len(contig), "positions": int(contig[:, 0].astype(np.int64).sum()),
               "longest_row": int(contig[:, 0].max()), "window": args.window, "repeats": args.repeats,
               "plan": {k: plan[k] for k in ("chain_family", "states_per_lane", "long_rows_cut", "hybrid_rows")},
               "q_route": d["q_route"], "forms": per_form,
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
