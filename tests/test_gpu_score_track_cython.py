"""The score track through the compiled Cython binding (`smcpp_amd/_smcpp_cy.pyx`): `score_rows` / `score_windows` return the arrays
of the ctypes binding, bit for bit, and raise where it raises.  The model is an `AdPiecewiseModel` whose `dlist` names the same
directions, in the same order, as `PiecewiseModel.differentiable = True` does."""
import numpy as np
import pytest

import test_gpu_gamma as tg
import test_gpu_score_track as ts

pytestmark = pytest.mark.gpu


def test_cython_manager_gives_the_same_bits(engine_opt):
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    engine_opt("SMCPP_SCORE_WAVES", None)
    case = "binned:M5"
    im, contigs = ts.manager(case)
    _, M, _, theta, rho = ts.inputs(case)
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(tg.N, contigs, synth.hidden_states(M), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1")                     # (every piece a variable: 16 directions)
    im2.theta = theta; im2.rho = rho; im2.alpha = 1.0
    im2.save_gamma = True
    im2.E_step()
    for c in range(len(contigs)):
        ts.same_bits(ts.products(im2, c), ts.products(im, c))
        L = len(contigs[c])
        assert np.array_equal(im2.score_rows(c, 0, L + 1, 2), im.score_rows(c, 0, L + 1, 2))
        assert np.array_equal(im2.score_rows(c, 1, L + 1, 1, parts=True), im.score_rows(c, 1, L + 1, 1, parts=True))
    assert im2.score_rows(0).shape == (len(a), len(contigs[0]) + 1) and im2.score_rows(0, parts=True).shape == (3, len(a), len(contigs[0]) + 1)
    with pytest.raises(RuntimeError):
        im2.score_rows(0, start=-1)
    with pytest.raises(RuntimeError, match="contig"):
        im2.score_windows(len(contigs), 100)
    with pytest.raises(RuntimeError, match="window_bp"):
        im2.score_windows(0, 0)
    # a model without variables: no seeds, refused; the manager stays usable
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1", differentiable=[])
    im2.E_step()
    with pytest.raises(RuntimeError, match="no derivative seeds"):
        im2.score_rows(0)
    assert im2.loglik_rows(0).shape == (len(contigs[0]) + 1,)
