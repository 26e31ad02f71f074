"""Golden G26: the reference's own pure-Python `SMCTwoPopulationModel` (smcpp/model.py:260-333) over two `SMCModel`s with
different knots, imported where it lies under /root/reference the way make_golden_model.py does (build container only):

    python tests/golden/make_golden_split_model.py

For every split of a fixed list - below model1's first knot, between knots, exactly on a knot of either model, at
max_split = model2's last knot - it records what the inference managers read (`for_pop(None | pid1 | pid2)`: stepwise values
and piece lengths, and the dict of the merged model of pid2), `split_ind`, `regularizer()` and `to_dict()`.  Data only."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    from make_golden_model import load_reference
    model, spline = load_reference()
    rng = np.random.default_rng(26)
    k1 = np.sort(0.004 * 400.0 ** rng.random(6))
    k2 = np.sort(0.002 * 300.0 ** rng.random(5))
    y1, y2 = rng.normal(0.0, 1.0, size=6), rng.normal(0.0, 1.0, size=5)
    m1 = model.SMCModel(k1, 1e4, spline.Piecewise, "pop1")
    m2 = model.SMCModel(k2, 1e4, spline.Piecewise, "pop2")
    m1[:] = y1
    m2[:] = y2
    splits = [k1[0] / 3, 0.5 * (k1[1] + k1[2]), 0.5 * (k2[2] + k2[3]), k1[2], k2[1], k1[0], k2[-1]]
    out = {"k1": k1, "k2": k2, "y1": y1, "y2": y2, "N0": np.array(1e4), "splits": np.array(splits)}
    for i, sp in enumerate(splits):
        tm = model.SMCTwoPopulationModel(m1, m2, sp)
        for tag, pid in (("none", None), ("p1", "pop1"), ("p2", "pop2")):
            m = tm.for_pop(pid)
            out[f"s{i}_{tag}_a"] = np.asarray(m.stepwise_values(), dtype=float)
            out[f"s{i}_{tag}_s"] = np.asarray(m.s, dtype=float)
        out[f"s{i}_p2_dict"] = np.array(json.dumps(tm.for_pop("pop2").to_dict()))
        out[f"s{i}_split_ind"] = np.array(int(tm.split_ind))
        out[f"s{i}_regularizer"] = np.array(float(tm.regularizer()))
        out[f"s{i}_dict"] = np.array(json.dumps(tm.to_dict()))
    path = os.path.join(HERE, "G26_split_model.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
