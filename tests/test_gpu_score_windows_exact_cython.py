"""The score track's exact windows through the compiled Cython binding (`smcpp_amd/_smcpp_cy.pyx`): `score_windows_exact` returns the
arrays of the ctypes binding, bit for bit, and raises where it raises.  The model is an `AdPiecewiseModel` whose `dlist` names the same
directions, in the same order, as `PiecewiseModel.differentiable = True` does (tests/test_gpu_score_track_cython.py)."""
import numpy as np
import pytest

import test_gpu_gamma as tg
import test_gpu_score_vectors as sv

pytestmark = pytest.mark.gpu


def test_cython_manager_gives_the_same_bits(engine_opt):
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    engine_opt("SMCPP_SCORE_WAVES", None)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    case = "cut:M65"
    im, contigs = sv.big_manager(case)
    _, M, _, theta, rho = sv.big_inputs(case)
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(tg.N, contigs, synth.hidden_states(M), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1")                     # (every piece a variable: 16 directions)
    im2.theta = theta; im2.rho = rho; im2.alpha = 1.0
    im2.save_gamma = True
    im2.E_step()
    for c, ob in enumerate(contigs):
        N = int(ob[:, 0].sum())
        for W in sorted({1, 7, min(100, N), N}):
            got, want = im2.score_windows_exact(c, W), im.score_windows_exact(c, W)
            assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (len(a), -(-N // W)) and np.array_equal(got, want), (c, W)
    with pytest.raises(RuntimeError, match="contig"):
        im2.score_windows_exact(len(contigs), 100)
    with pytest.raises(RuntimeError, match="window_bp"):
        im2.score_windows_exact(0, 0)
    engine_opt("SMCPP_SCORE_FORM", None)
    with pytest.raises(RuntimeError, match="SMCPP_SCORE_FORM=vectors"):
        im2.score_windows_exact(0, 100)
    engine_opt("SMCPP_SCORE_FORM", "vectors")
    assert np.array_equal(im2.score_windows_exact(0, 100), im.score_windows_exact(0, 100))
