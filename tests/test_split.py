"""The two-population model of `smc++ split` and the refusals of SplitAnalysis - no GPU needed."""
import copy
import json
import os

import numpy as np
import pytest

from smcpp_amd import analysis as A
from smcpp_amd import data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300), initial=0.0))


def _g26():
    z = np.load(os.path.join(GOLDEN, "G26_split_model.npz"))
    m1 = A.SMCModel(z["k1"], float(z["N0"]), "pop1")
    m2 = A.SMCModel(z["k2"], float(z["N0"]), "pop2")
    m1[:] = z["y1"]
    m2[:] = z["y2"]
    return z, m1, m2


def _same_dict(a, b, path=""):
    assert type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))), (path, a, b)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same_dict(a[k], b[k], path + "/" + k)
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_dict(x, y, f"{path}[{i}]")
    elif isinstance(a, float):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_two_population_model_matches_the_reference():
    """Golden G26 (tests/golden/make_golden_split_model.py): the reference's `SMCTwoPopulationModel` at splits below model1's
    first knot, between knots, on a knot of each model and at max_split - what every manager reads, to 1e-12 relative."""
    z, m1, m2 = _g26()
    assert len(z["splits"]) >= 5 and z["splits"][-1] == z["k2"][-1]
    for i, sp in enumerate(z["splits"]):
        tm = A.SMCTwoPopulationModel(m1, m2, float(sp))
        for tag, pid in (("none", None), ("p1", "pop1"), ("p2", "pop2")):
            m = tm.for_pop(pid)
            assert _rel(m.stepwise_values(), z[f"s{i}_{tag}_a"]) <= 1e-12, (i, tag)
            assert _rel(m.s, z[f"s{i}_{tag}_s"]) <= 1e-12, (i, tag)
        _same_dict(tm.for_pop("pop2").to_dict(), json.loads(str(z[f"s{i}_p2_dict"])))
        assert tm.split_ind == int(z[f"s{i}_split_ind"]), i
        assert abs(tm.regularizer() - float(z[f"s{i}_regularizer"])) <= 1e-12 * max(abs(float(z[f"s{i}_regularizer"])), 1e-300)
        _same_dict(tm.to_dict(), json.loads(str(z[f"s{i}_dict"])))


def test_two_population_model_dict_round_trips_and_loads_the_reference_dict():
    z, m1, m2 = _g26()
    for i, sp in enumerate(z["splits"]):
        tm = A.SMCTwoPopulationModel(m1, m2, float(sp))
        back = A.SMCTwoPopulationModel.from_dict(json.loads(json.dumps(tm.to_dict())))
        assert back.to_dict() == tm.to_dict()
        ref = A.model_from_dict(json.loads(str(z[f"s{i}_dict"])))       # written by the reference
        assert isinstance(ref, A.SMCTwoPopulationModel)
        for pid in (None, "pop1", "pop2"):
            assert np.array_equal(ref.for_pop(pid).stepwise_values(), tm.for_pop(pid).stepwise_values())
            assert np.array_equal(ref.for_pop(pid).s, tm.for_pop(pid).s)
        assert ref.split == tm.split and ref.pids == ["pop1", "pop2"] and ref.N0 == 1e4
        assert ref.distinguished_model.to_dict() == tm.model1.to_dict()


def test_two_population_model_notifies_and_sets_coordinates():
    _, m1, m2 = _g26()
    tm = A.SMCTwoPopulationModel(m1, m2, 0.5)
    seen = []

    class Obs:
        def update(self, message, *a, **k):
            seen.append(message)
    ob = Obs()
    tm.register(ob)
    tm.split = 0.7
    m1[0] = 0.1
    m2[1] = 0.2
    assert seen == ["model update"] * 3
    x = tm[:]
    assert np.array_equal(x, np.r_[m1[:], m2[:]])
    tm[:] = x + 0.25
    assert np.allclose(m1[:], x[:len(m1)] + 0.25) and np.allclose(m2[:], x[len(m1):] + 0.25)
    assert tm[(1, 1)] == m2[1]
    assert tm.dlist == []


# ---- refusals (all raised before any inference manager exists) ----

def _contig(pid, n, a, rng, L=300000):
    k = len(pid)
    rows = []
    pos = 0
    while pos < L:
        sp = int(rng.integers(100, 5000))
        rows.append([sp] + [x for j in range(k) for x in (0, 0, n[j])])
        row = [1]
        for j in range(k):
            row += [int(rng.integers(0, a[j] + 1)), int(rng.integers(0, n[j] + 1)), n[j]]
        rows.append(row)
        pos += sp + 1
    return D.Contig(data=np.array(rows, dtype=np.int32), pid=tuple(pid), n=list(n), a=list(a))


def _fits(theta=1e-4, N0=1e4):
    m1 = A.SMCModel([0.01, 0.1, 1.0], N0, "pop1")
    m2 = A.SMCModel([0.02, 0.2, 2.0], N0, "pop2")
    hs = [0.0, 0.5, np.inf]
    d1 = {"theta": theta, "rho": theta, "alpha": 1, "model": m1.to_dict(), "hidden_states": {"pop1": hs}}
    d2 = {"theta": theta, "rho": theta, "alpha": 1, "model": m2.to_dict(), "hidden_states": {"pop2": hs}}
    return d1, d2


def test_split_analysis_refuses_data_without_a_joint_spectrum():
    rng = np.random.default_rng(1)
    d1, d2 = _fits()
    cs = [_contig(("pop1",), [4], [2], rng), _contig(("pop2",), [4], [2], rng)]
    with pytest.raises(RuntimeError, match="no joint frequency spectrum"):
        A.SplitAnalysis(cs, A.SplitArgs(pop1=d1, pop2=d2))


def test_split_analysis_refuses_fits_with_different_theta_or_N0(tmp_path):
    rng = np.random.default_rng(2)
    cs = lambda: [_contig(("pop1",), [4], [2], rng), _contig(("pop1", "pop2"), [2, 3], [2, 0], rng)]  # noqa: E731
    d1, d2 = _fits()
    d2["theta"] = 2e-4
    with pytest.raises(RuntimeError, match="different theta"):
        A.SplitAnalysis(cs(), A.SplitArgs(pop1=d1, pop2=d2))
    d1, d2 = _fits()
    d2["model"]["N0"] = 2e4
    # the files work as well as the dicts
    for nm, d in (("p1", d1), ("p2", d2)):
        with open(tmp_path / (nm + ".final.json"), "wt") as f:
            json.dump(d, f)
    with pytest.raises(RuntimeError, match="different N0"):
        A.SplitAnalysis(cs(), A.SplitArgs(pop1=str(tmp_path / "p1.final.json"), pop2=str(tmp_path / "p2.final.json")))


def test_split_analysis_refuses_a_population_pair_with_mixed_distinguished_lineages():
    rng = np.random.default_rng(3)
    d1, d2 = _fits()
    cs = [_contig(("pop1", "pop2"), [2, 3], [2, 0], rng), _contig(("pop1", "pop2"), [1, 3], [1, 1], rng)]
    with pytest.raises(RuntimeError, match="different distinguished lineages"):
        A.SplitAnalysis(cs, A.SplitArgs(pop1=d1, pop2=d2))


def test_estimate_still_refuses_two_population_data():
    rng = np.random.default_rng(4)
    cs = [_contig(("pop1",), [4], [2], rng), _contig(("pop1", "pop2"), [2, 3], [2, 0], rng)]
    with pytest.raises(RuntimeError, match="Please use 'smc\\+\\+ split' to estimate two-population models"):
        A.Analysis(cs, A.EstimateArgs())
