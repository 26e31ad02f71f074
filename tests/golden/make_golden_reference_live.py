"""Emit golden G25: the compiled reference's answers for the CPU tests that used to call it live, so that they run wherever
the repository is checked out (the compiled reference, oracle/_ref, exists only where the reference sources lie).

BUILD CONTAINER ONLY (needs oracle/_ref: `make -C oracle ref`).  Every input is fixed here and stored beside the answer:

  oracle_*   tests/test_oracle.py::test_oracle_vs_compiled_reference_live - `HMM::Estep` with save_gamma on
             synth.synth_contig(5, 600 kbp, n = 10) under G3's parameters (loglik, float alpha, xisum, argmax of gamma)
  g4_*       tests/test_oracle.py::test_emission_assembly_reproduces_golden_tables - `ref_prep` of G4's model
  edge{i}_*  tests/test_prep.py::test_prep_vs_reference_live_edge_sizes - `ref_prep` at the edge sizes (M, n)
  jac{i}_*   tests/test_prep.py::test_jacobians_vs_reference_autodiff - `ref_prep_jac` (adouble) values and Jacobians
  apart{i}_* tests/test_jcsfs.py::test_apart_matches_live_oracle_on_other_models - oracle/jcsfs_apart_oracle.py

    python tests/golden/make_golden_reference_live.py     # writes tests/golden/G25_reference_live.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from conftest import load_golden   # noqa: E402
from oracle import jcsfs_apart_oracle as JA, ref   # noqa: E402
from smcpp_amd import synth   # noqa: E402

EDGE_SIZES = [(8, 0), (8, 1), (8, 2), (24, 3), (51, 28)]
JAC_SIZES = [(8, 3), (32, 10)]


def main():
    assert ref.available(), "oracle/_ref is not built"
    out = {}
    g = load_golden("G3_M32_n10_2Mbp")
    obs = synth.synth_contig(5, 600_000, 10)
    r = ref.estep(g["pi"], g["T"], g["keys"], g["E"], obs, save_gamma=True, want_alpha=True)
    out.update(oracle_obs=obs, oracle_loglik=np.array(r["loglik"]), oracle_alpha_hat=r["alpha_hat"], oracle_xisum=r["xisum"],
               oracle_gamma_argmax=r["gamma"].argmax(0).astype(np.int32))

    g = load_golden("G4_M64_n20_2Mbp")
    p = ref.prep(g["a"], g["s"], g["hs"], float(g["rho"]), float(g["theta"]), int(g["n"]))
    out.update({"g4_" + k: v for k, v in p.items()})

    for i, (M, n) in enumerate(EDGE_SIZES):
        hs = np.r_[0., np.logspace(-2, 1, M - 1), np.inf]
        a = np.array([1.0, 2.0, 0.5, 1.0, 3.0]); s = np.array([0.05, 0.2, 1.0, 1.0, 1.0])
        p = ref.prep(a, s, hs, 6e-3, 2.5e-2, n)
        out.update({f"edge{i}_{k}": v for k, v in p.items()})
        out.update({f"edge{i}_M": np.array(M), f"edge{i}_n": np.array(n), f"edge{i}_hs": hs, f"edge{i}_a": a, f"edge{i}_s": s})

    for i, (M, n) in enumerate(JAC_SIZES):
        hs = synth.hidden_states(M)
        a, s = synth.model_pieces(6)
        da = np.eye(6)[:, :4] + 0.25
        r = ref.prep_jac(a, da, s, hs, 6.25e-3, 2.5e-2, n)
        out.update({f"jac{i}_{k}": v for k, v in r.items()})
        out.update({f"jac{i}_M": np.array(M), f"jac{i}_n": np.array(n), f"jac{i}_hs": hs, f"jac{i}_a": a, f"jac{i}_s": s,
                    f"jac{i}_da": da})

    rng = np.random.default_rng(5)
    i = 0
    for n1, n2 in ((2, 7), (5, 1)):
        a1 = np.exp(rng.normal(0, 0.7, 5)); a2 = np.exp(rng.normal(0, 0.7, 3))
        s1 = np.exp(rng.normal(-2, 0.8, 5)); s2 = np.exp(rng.normal(-2, 0.8, 3))
        hs = np.r_[0.0, np.sort(np.exp(rng.normal(-1.5, 1.2, 7))), np.inf]
        for split in (0.0, float(hs[2]), 0.33):
            out.update({f"apart{i}_n": np.array([n1, n2]), f"apart{i}_a1": a1, f"apart{i}_s1": s1, f"apart{i}_a2": a2,
                        f"apart{i}_s2": s2, f"apart{i}_hs": hs, f"apart{i}_split": np.array(split),
                        f"apart{i}_J": JA.joint_csfs_apart(n1, n2, hs, (a1, s1), (a2, s2), split)})
            i += 1
    out["apart_ncases"] = np.array(i)

    path = os.path.join(HERE, "G25_reference_live.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
