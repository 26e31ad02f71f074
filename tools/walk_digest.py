"""The bits of every product that walks an engine row, as one sha256 per product and case: two builds that print the same lines
compute the same bits.

The row walks of the posterior transitions, the sampled paths, the per-position posteriors, the log-likelihood track and the score
track with its exact windows (smcpp_amd/csrc/*_dev.hpp over walk_dev.hpp) are run on small seeded inputs: three ragged contigs of a few hundred un-binned
rows with spans 1, 2, 63, 64, 65, 128, 129 and 200 placed by hand (rows of one, two and three blocks of 64 positions, and a last
block of one position), at M = 5, 64, 65, 130, 200, 256, 300 and 520 hidden states (padding states; 1, 2, 3, 4, 8 and 16 states per
lane).  SMCPP_SPLIT_SPANS=0 keeps the long rows un-cut beyond 64 states, so the checkpoint pass runs; beyond 256 states the engine
only takes rows cut into pieces, so there the switch is left unset.  Every case runs twice: with
the engine's own launch shape, and with SMCPP_LL_WAVES / SMCPP_SCORE_WAVES / SMCPP_PATH_BATCH set so that every wavefront gets a
second unit of work.  A product the build refuses at a state count prints `refused`.

The tool computes no tolerance and holds no expected values: run it on two checkouts and compare the output.

    python tools/walk_digest.py [--root DIR] [--states 5,64,...]
"""
import argparse
import hashlib
import os
import sys

SPANS = (1, 2, 63, 64, 65, 128, 129, 200)
STATES = (5, 64, 65, 130, 200, 256, 300, 520)
ROWS = (300, 170, 90)
THETA, RHO = 2e-4, 6e-5                # per base pair (un-binned rows)
N = 8
WINDOW = 97
CAPS = {"SMCPP_LL_WAVES": "3", "SMCPP_SCORE_WAVES": "3", "SMCPP_PATH_BATCH": "2"}


def contigs(np, synth):
    out = []
    for i, rows in enumerate(ROWS):
        c = synth.synth_posterior_contig(rows, N, seed=21 + i).copy()
        c[:, 0] = np.minimum(c[:, 0], 40)
        mono = np.nonzero((c[:, 0] > 1) & (c[:, 1] == 0))[0]
        for j, s in enumerate(SPANS[i:] + SPANS[:i]):          # (every contig holds every span, in another order)
            c[mono[1 + 3 * j], 0] = s
        edge = np.zeros((1, 4), dtype=np.int32)
        edge[0, 0] = 1; edge[0, 3] = N
        out.append(np.ascontiguousarray(np.vstack([edge, c, edge]), dtype=np.int32))
    return out


def digest(np, v):
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode())
                feed(x[k])
        elif isinstance(x, (tuple, list)):
            for y in x:
                feed(y)
        else:
            a = np.ascontiguousarray(x)
            h.update(f"{a.dtype}{a.shape}".encode())
            h.update(a.tobytes())
    feed(v)
    return h.hexdigest()


def products(np, im, c, w, set_option):
    """name -> call, in the order they are run"""
    def score(form, what):
        def f():
            set_option("SMCPP_SCORE_FORM", form)
            try:
                if what == "exact":
                    return [im.score_windows_exact(c, W) for W in (WINDOW, 7, 1)]
                return im.score_rows(c, parts=True) if what == "rows" else im.score_windows(c, WINDOW)
            finally:
                set_option("SMCPP_SCORE_FORM", None)
        return f
    q = (0.025, 0.5, 0.975)
    return {
        "transitions": lambda: im.posterior_transitions(c),
        "transition_windows": lambda: im.posterior_transition_windows(c, WINDOW),
        "sample_rows": lambda: im.posterior_sample_rows(c, n_paths=5, seed=1234),
        "sample_positions": lambda: im.posterior_sample_positions(c, n_paths=5, seed=1234),
        "positions": lambda: im.posterior_positions(c),
        "positions_step3": lambda: im.posterior_positions(c, 2, None, 3),
        "position_summary": lambda: im.posterior_position_summary(c, weights=w, quantiles=q),
        "windows_exact": lambda: im.posterior_windows_exact(c, WINDOW),
        "loglik_rows": lambda: im.loglik_rows(c),
        "loglik_positions": lambda: im.loglik_positions(c),
        "loglik_positions_step3": lambda: im.loglik_positions(c, 2, None, 3),
        "loglik_windows": lambda: im.loglik_windows(c, WINDOW),
        "score_rows_matrix": score("matrix", "rows"),
        "score_windows_matrix": score("matrix", "windows"),
        "score_rows_vectors": score("vectors", "rows"),
        "score_windows_vectors": score("vectors", "windows"),
        # (behind every earlier line, so that those run in the order they always ran in)
        "score_windows_exact_vectors": score("vectors", "exact"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose smcpp_amd is run")
    ap.add_argument("--states", default=",".join(str(m) for m in STATES))
    args = ap.parse_args()
    for k in list(CAPS) + ["SMCPP_SCORE_FORM", "SMCPP_SPLIT_SPANS"]:
        os.environ.pop(k, None)
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from smcpp_amd import _engine, _smcpp, synth
    from smcpp_amd.model import PiecewiseModel

    obs = contigs(np, synth)
    a, s_ = synth.model_pieces()
    print(f"# root {os.path.abspath(args.root)}; contigs of {[len(c) for c in obs]} rows, {[int(c[:, 0].sum()) for c in obs]} positions")
    for M in (int(m) for m in args.states.split(",")):
        hs = synth.hidden_states(M)
        _engine.set_option("SMCPP_SPLIT_SPANS", "0" if M <= 256 else None)     # (read when a manager is built)
        im = _smcpp.PyOnePopInferenceManager(N, obs, hs, ("pop1",), 0.5, device=0)
        model = PiecewiseModel(a, s_, 1e4, pid="pop1")
        model.differentiable = True
        im.model = model
        im.theta = THETA; im.rho = RHO; im.alpha = 1.0
        im.save_gamma = True
        im.E_step()
        plan = im.describe()["plan"]
        print(f"# M {M}: states per lane {plan['states_per_lane']}, long rows cut {plan['long_rows_cut']}")
        w = np.linspace(0.5, 2.0, M)
        for shape in ("free", "capped"):
            for k, v in CAPS.items():
                _engine.set_option(k, v if shape == "capped" else None)
            for c in range(len(obs)):
                for name, call in products(np, im, c, w, _engine.set_option).items():
                    try:
                        line = digest(np, call())
                    except RuntimeError as e:
                        line = "refused: " + " ".join(str(e).split())[:60]
                    print(f"M{M} {shape} contig{c} {name} {line}", flush=True)
        for k in CAPS:
            _engine.set_option(k, None)
        del im


if __name__ == "__main__":
    main()
