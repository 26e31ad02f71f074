"""The row-descriptor stream of the scan chains (smcpp_amd/csrc/chains_ss.hpp: ss_desc_stream, ss_desc_fetch).

Every row loop of the scan chains reads its {key slot, span} descriptors through scalar loads, one per row and two rows ahead of the
row it walks: three rotating scalar pairs instead of 64 descriptors per lane load.  What can go wrong is the bookkeeping at the ends:
the first two descriptors of a chunk, the request two rows past its last row (the next chunk's rows, the next contig's, or the pad in
front of the first and behind the last contig), and the rotation when a chunk has fewer rows than the look-ahead.  So the cases cut

  * two contigs that lie back to back - 8 000 and 3 000 positions, about 1 900 and 700 rows; the first ends on a span-1 row of the
    monomorphic key, the second begins with a span-17 row of the missing key, so a descriptor consumed across the seam shows -
  * into chunks of 1, 2, 3 (shorter than, as long as, one longer than the look-ahead), 63, 64, 65 (the block edge of the 64-descriptor
    lane loads this replaced) and 129 rows with set_chunking; a contig's first chunk starts at its first row and its last chunk ends
    at its last row (asserted from the getter), so the look-ahead reads the pad on both sides,

and hold every E-step against the C restatement (LL_TOL, STAT_TOL, check_gamma_columns: the bars of tests/test_gpu_parity.py) and
against the run of the same kernels on ONE chunk per contig and direction (set_chunking(10**9): no history, no fixed point):

  * M = 64 with per-row posteriors (save_gamma), every column of every contig by test_gpu_seams.check_rows:
      - with the certificate's tolerances EPS_F / EPS_B at all seven chunk lengths against the restatement, and at 63 rows and more
        (a chunk then averages an e-fold of positions, 4.25 per row) against the one-chunk run with the bound of
        tests/test_gpu_seams.py as it stands, seq_bound("A", "fast") = 2 (EPS_F + EPS_B).  That bound takes the changes the certificate
        accepts at successive seams as not adding up; at chunks of 1, 2, 3 rows hundreds of seams lie within one forgetting length and
        they do (measured: 4.6e-6, 6.6e-6, 6.6e-6 against 6e-6), so there the distance is printed and the restatement's bars bind;
      - at 1, 2 and 3 rows also with the tolerances of tests/test_gpu_ss.py's "second_round" case (EXACT = 1e-30: a chunk re-runs until
        its input is bitwise what it last ran from, the fixed point degenerates to the sequential algorithm), against the restatement
        and against the one-chunk run with the same unmodified bound;
  * statistics only (log-likelihood, xi sums, gamma sums, gamma_0; the four measures of tests/test_gpu_ss_jumps.py): M = 64 with
    span-1 rows only, M = 16 (two-row scans), M = 65 (two states per lane), and M = 64 with the power jumps forced (SMCPP_SS_JUMP=8)
    in two light passes per direction - all seven chunk lengths under EXACT (with EPS_F / EPS_B and chunks of one span-1 row the xi sums
    come out 5.9e-6 from the restatement, bar 5e-6: what the certificate accepts at a thousand seams in a row), and chunks of 65 and 129
    rows under EPS_F / EPS_B, so that the certificate decides at the tolerances the other tests use.  Both the chunked and the one-chunk
    run are held to the restatement by LL_TOL / STAT_TOL, and so is their distance from each other.  The light passes can only change
    how fast the fixed point is reached, so every case also caps passes_to_certificate at what the sequential algorithm needs: the
    light passes, one stored pass per chunk of the longest contig, and two (the certifying pass and a second round's first);
  * the halo (SMCPP_SS_HALO=1 with the short halo of tests/test_gpu_seams.py, automatic chunks), with and without jumps: per-row
    posteriors as in the first item;
  * SMCPP_DEBUG_POISON=nan on chunks of 3 rows: every output finite and bitwise what the clean run gives.

Measured on one MI355X (49 cases, 4 s; the restatement is run once per configuration and contig).  Per-row posteriors, worst column
against the restatement (bar 2e-5 of its span) / against the one-chunk run (bound 6e-6 relative): EPS_F / EPS_B at 63, 64, 65, 129 rows
7.7e-7 / 3.4e-6, 6.4e-7 / 3.4e-6, 6.4e-7 / 3.4e-6, 7.0e-7 / 2.7e-6 (16, 15, 15, 8 passes to the certificate); at 1, 2, 3 rows 1.0e-6,
1.4e-6, 1.6e-6 against the restatement (917, 450, 314 passes); EXACT at 1, 2, 3 rows 3.4e-7 / 6.4e-7, 3.1e-7 / 7.5e-7, 3.3e-7 / 6.5e-7
(1 911, 958, 640 passes).  Statistics, worst of the four configurations (log-likelihood, xi sums, gamma sums, gamma_0): EXACT, seven
chunk lengths, 9.0e-9, 1.4e-6, 8.9e-7, 2.0e-7 against the restatement and 7.5e-9, 4.6e-7, 5.2e-7, 1.8e-7 against one chunk, passes =
chunks of the longest contig + light passes; EPS_F / EPS_B at 65 and 129 rows 5.9e-9, 1.8e-6, 2.2e-6, 1.2e-6 and 2.6e-9, 1.7e-6, 2.2e-6,
1.2e-6, passes 30 / 14 (span-1 rows), 11 / 6 (M = 16), 16 / 8 (M = 65), 15 / 8 (jumps) against caps of 36 / 21 (jumps: 34 / 19).
Halo: 5.7e-7 of the span against the restatement, 2.1e-6 against the one-chunk run, 4 passes.
"""
import numpy as np
import pytest

from test_gpu_gamma import RH_B, TH_B, _onepop
from test_gpu_parity import LL_TOL, STAT_TOL, oracle_estep
from test_gpu_seams import EPS_B, EPS_F, SHORT, _rows, check_rows, seq_bound

pytestmark = pytest.mark.gpu

CHUNKS = [1, 2, 3, 63, 64, 65, 129]
ONE = 10 ** 9
JUMP = {"SMCPP_SS_JUMP": "8", "SMCPP_SS_LIGHT_F": "2", "SMCPP_SS_LIGHT_B": "2"}
# id -> (M, span-1 rows only?, switches, states per lane)
CONFIGS = {"M64": (64, False, {}, 1), "M64_span1": (64, True, {}, 1), "M16": (16, False, {}, 1), "M65": (65, False, {}, 2),
           "M64_jump": (64, False, JUMP, 1)}
EXACT = (1e-30, 1e-30)    # tolerances of tests/test_gpu_ss.py's "second_round" case: a chunk re-runs until its input is bitwise what it last ran from
TOLS = {"cert": (EPS_F, EPS_B), "exact": EXACT}
_CONTIGS = {}
_RUNS = {}


def _contigs(span1):
    if span1 not in _CONTIGS:
        a = _rows(201, 8_000, 64)
        b = _rows(202, 3_000, 64).copy()
        b[0] = (17, -1, 0, 0)                                   # the missing key, 17 positions: neither the key nor the span of a's last row
        assert tuple(a[-1]) == (1, 0, 0, 0) and a[0, 0] == 1 and b[-1, 0] == 1
        if span1:
            a, b = a.copy(), b.copy()
            a[:, 0] = 1
            b[:, 0] = 1
        else:
            assert (a[:, 0] > 8).sum() > 100 and (a[:, 0] == 1).sum() > 100
        _CONTIGS[span1] = [np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)]
    return _CONTIGS[span1]


def _manager(config, chunk, engine_opt, save_gamma, extra=None, eps=(EPS_F, EPS_B)):
    M, span1, switches, _ = CONFIGS[config]
    for k, v in dict(switches, **(extra or {})).items():
        engine_opt(k, v)
    contigs = _contigs(span1)
    im = _onepop(M, contigs, TH_B, RH_B)
    im.set_chunking(chunk, *eps)
    im.save_gamma = save_gamma
    return im, contigs


def _assert_plan(config, chunk, im, contigs):
    plan = im.describe()["plan"]
    _, _, switches, npl = CONFIGS[config]
    assert im.chain_mode() == 5 and plan["scan_chains"] and plan["states_per_lane"] == npl, plan
    assert plan["power_jumps"]["run"] == ("SMCPP_SS_JUMP" in switches), plan["power_jumps"]
    if switches and chunk < ONE:
        assert plan["light_passes_forward"] == 2 == plan["light_passes_backward"], plan
    if chunk:
        want = sum(max(1, -(-len(c) // chunk)) for c in contigs)
        assert plan["chunks_forward"] == want == plan["chunks_backward"] and not plan["halo_pass"], (plan, want)
    for back in (False, True):
        ch = im.chunks(back)
        for c, ob in enumerate(contigs):
            mine = ch[ch[:, 0] == c]
            assert mine[:, 1].min() == 0 and mine[:, 2].max() == len(ob), (config, chunk, c, mine[:, 1].min(), mine[:, 2].max())
            if 0 < chunk < ONE:
                assert (mine[:, 2] - mine[:, 1]).max() <= chunk and (mine[:, 2] - mine[:, 1]).min() >= max(1, chunk // 2), (config, chunk, c)
    if 0 < chunk < ONE:
        # the sequential algorithm: chunk c of a contig is exact after the light passes and c stored passes; then the certifying pass
        longest = max(-(-len(c) // chunk) for c in contigs)
        cap = max(plan["light_passes_forward"], plan["light_passes_backward"]) + longest + 2
        assert plan["passes_to_certificate"] <= cap, (config, chunk, plan["passes_to_certificate"], cap)
    return plan


def _stats(im, contigs):
    keys = im.keys
    ep = im.emission_probs
    return dict(ll=list(im.logliks()), xis=[x.copy() for x in im.xisums], gs=[{k: v.copy() for k, v in d.items()} for d in im.gamma_sums],
                g0=[g[:, 0].copy() for g in im.gammas], pi=np.array(im.pi), T=np.array(im.transition), keys=np.array(keys),
                E=np.array([ep[tuple(k)] for k in keys.tolist()]))


def _run(config, chunk, engine_opt, tol="exact"):
    """Statistics of one E-step of `config` cut into chunks of `chunk` rows, shared by the tests of the process."""
    key = (config, chunk, tol)
    if key not in _RUNS:
        im, contigs = _manager(config, chunk, engine_opt, False, None, TOLS[tol])
        im.E_step()
        out = _stats(im, contigs)
        out["plan"] = _assert_plan(config, chunk, im, contigs)
        _RUNS[key] = out
    return _RUNS[key]


def _diff(a, b, c):
    """Contig c -> (log-likelihood, xi sums, gamma sums, gamma_0): relative differences in the metric of the bars."""
    dl = abs(a["ll"][c] - b["ll"][c]) / abs(b["ll"][c])
    dx = float(np.max(np.abs(a["xis"][c] - b["xis"][c]) / np.abs(b["xis"][c])))
    assert sorted(a["gs"][c]) == sorted(b["gs"][c])
    dg = max(float(np.max(np.abs(a["gs"][c][k] - v)) / max(np.abs(v).max(), 1e-300)) for k, v in b["gs"][c].items())
    d0 = float(np.max(np.abs(a["g0"][c] - b["g0"][c]) / np.maximum(np.abs(b["g0"][c]), 1e-300)))
    return dl, dx, dg, d0


def _restatement(r, contigs):
    os_ = [oracle_estep(r["pi"], r["T"], r["keys"], r["E"], ob, save_gamma=False) for ob in contigs]
    return dict(ll=[o["loglik"] for o in os_], xis=[o["xisum"] for o in os_], gs=[o["gamma_sums"] for o in os_], g0=[o["gamma"][:, 0] for o in os_])


@pytest.mark.parametrize("chunk,tol", [(c, "cert") for c in CHUNKS] + [(c, "exact") for c in (1, 2, 3)])
def test_per_row_posteriors_at_every_chunk_length(engine_opt, chunk, tol):
    im, contigs = _manager("M64", chunk, engine_opt, True, None, TOLS[tol])
    im.E_step()
    plan = _assert_plan("M64", chunk, im, contigs)
    assert plan["save_gamma"], plan
    print(f"M64, chunks of {chunk} rows, {tol}: {plan['chunks_forward']} chunks per direction, light passes {plan['light_passes_forward']} / "
          f"{plan['light_passes_backward']}, passes to the certificate {plan['passes_to_certificate']}, launched {plan['passes_launched']}")
    if "seq" not in _RUNS:
        one, _ = _manager("M64", ONE, engine_opt, True)
        one.E_step()
        assert one.describe()["plan"]["chunks_forward"] == len(contigs) == one.describe()["plan"]["chunks_backward"]
        _RUNS["seq"] = ([g.copy() for g in one.gammas], list(one.logliks()))
    bound = seq_bound("A", "fast") if tol == "exact" or chunk >= 63 else None
    check_rows(f"M64, chunks of {chunk} rows, {tol}", im, contigs, _RUNS["seq"], bound, False)


@pytest.mark.parametrize("chunk,tol", [(c, "exact") for c in CHUNKS] + [(c, "cert") for c in (65, 129)])
@pytest.mark.parametrize("config", ["M64_span1", "M16", "M65", "M64_jump"])
def test_statistics_at_every_chunk_length(engine_opt, config, chunk, tol):
    contigs = _contigs(CONFIGS[config][1])
    r = _run(config, chunk, engine_opt, tol)
    one = _run(config, ONE, engine_opt)
    ref = _restatement(r, contigs)
    plan = r["plan"]
    print(f"{config}, chunks of {chunk} rows, {tol}: {plan['chunks_forward']} chunks per direction, light passes {plan['light_passes_forward']} / "
          f"{plan['light_passes_backward']}, passes to the certificate {plan['passes_to_certificate']}, launched {plan['passes_launched']}")
    for c in range(len(contigs)):
        for name, other in (("the restatement", ref), ("one chunk", one)):
            dl, dx, dg, d0 = _diff(r, other, c)
            print(f"{config}, chunks of {chunk} rows, {tol}, contig {c} against {name}: loglik {dl:.2e}, xi sums {dx:.2e}, gamma sums {dg:.2e}, gamma_0 {d0:.2e}")
            assert dl <= LL_TOL and dx <= STAT_TOL and dg <= STAT_TOL and d0 <= STAT_TOL, (config, chunk, tol, c, name)


@pytest.mark.parametrize("jump", [False, True])
def test_per_row_posteriors_through_the_halo(engine_opt, jump):
    extra = dict(SHORT, **({"SMCPP_SS_JUMP": "8"} if jump else {}))
    im, contigs = _manager("M64", 0, engine_opt, True, extra)
    im.E_step()
    plan = im.describe()["plan"]
    print(f"halo, jumps {'forced' if jump else 'off'}: chunks {plan['chunks_forward']} / {plan['chunks_backward']}, power_jumps {plan['power_jumps']}, "
          f"passes to the certificate {plan['passes_to_certificate']}")
    assert im.chain_mode() == 5 and plan["halo_pass"] and plan["chunks_forward"] > len(contigs), plan
    for k in extra:
        engine_opt(k, None)
    if "seq" not in _RUNS:
        one, _ = _manager("M64", ONE, engine_opt, True)
        one.E_step()
        _RUNS["seq"] = ([g.copy() for g in one.gammas], list(one.logliks()))
    check_rows(f"M64, halo, jumps {'forced' if jump else 'off'}", im, contigs, _RUNS["seq"], seq_bound("A", "fast"), False)


def test_no_poison_reaches_the_outputs(engine_opt):
    engine_opt("SMCPP_DEBUG_POISON", None)
    outs = []
    for poison in (None, "nan"):
        engine_opt("SMCPP_DEBUG_POISON", poison)
        im, contigs = _manager("M64", 3, engine_opt, True)
        im.E_step()
        s = _stats(im, contigs)
        s["gam"] = [g.copy() for g in im.gammas]
        outs.append(s)
        del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    clean, poisoned = outs
    for k in ("ll", "xis", "g0", "gam"):
        for c in range(2):
            assert np.all(np.isfinite(poisoned[k][c])), (k, c)
            assert np.array_equal(np.asarray(clean[k][c]), np.asarray(poisoned[k][c])), (k, c)
    for c in range(2):
        for key, v in clean["gs"][c].items():
            assert np.all(np.isfinite(poisoned["gs"][c][key])) and np.array_equal(v, poisoned["gs"][c][key]), (c, key)
