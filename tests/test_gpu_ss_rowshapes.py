"""The control flow of the scan chains' row loops (smcpp_amd/csrc/chains_ss.hpp: ss_positions, ss_light_walk, the stored loops of
ss_forward_wave / ss_backward_wave).

The loops are laid out for the branches a row takes: the light walks run through span-1 rows in an inner loop and do the further
positions of a longer row behind it, four per trip and the span - 1 mod 4 left over in a nest of ifs; the stored loops keep what a row
rarely does out of line, and a merge leaves through the loop's own test with its stores turned off.  None of it may move a bit, and
what can go wrong is which row's emission vector a position is stepped with, a position too many or too few at some remainder, the
row behind a run of span-1 rows, the walk's first and last row, and the row on which a re-run merges.  So the input - two contigs back
to back, about 6 000 and 3 000 positions - holds, beside synthetic rows,

  * every ordered pair of spans 1 .. 11 as neighbours (asserted), so every remainder of the four-position trip follows and precedes
    every other, with the keys alternating between the monomorphic one and a heterozygous one,
  * runs of 1, 2, 3 and 40 span-1 rows between rows of span 5,
  * rows of the jump key with span - 1 = 7, 8, 9, 15, 16, 17, 24 (one below, at, one above one and two jumps of 8, and three),
  * a span-1 first row and a span-11 last row on the first contig, a span-11 first row and a span-1 last row on the second,

and is cut into chunks of 1, 2, 3, 5, 17 and 33 rows (at 33 a re-run reaches its merge test on iteration 16 and 32) and into one chunk
per contig, at M = 64 (float scans, and fp64 scans with SMCPP_SS_MIXED=0), M = 64 with the power jumps forced in two light passes per
direction, M = 16 (two-row scans) and M = 65 (two states per lane: the instantiations that keep the one-level loops and two positions
per trip, because their bits follow the loop shape - held here to the same input and the same pass counts); and, automatically
cut, run through the halo with jumps on and off.
Every case runs with per-row posteriors and is held by test_gpu_seams.check_rows to the C restatement - every column at the bars of
tests/test_gpu_parity.py, log-likelihood, xi sums and gamma sums by LL_TOL / STAT_TOL - with the certificate's tolerances EPS_F / EPS_B;
at chunks of 1, 2 and 3 rows M = 64 also runs with the tolerances of tests/test_gpu_ss.py's "second_round" case (a chunk re-runs until
its input is bitwise what it last ran from), where every column is also within seq_bound("A", "fast") of the one-chunk run - the rule
of tests/test_gpu_ss_rowstream.py for when that bound applies (chunks under 63 rows put hundreds of seams within one forgetting
length, and what the certificate accepts at each adds up).  SMCPP_DEBUG_POISON=nan on chunks of 3 rows gives finite outputs, bitwise
those of the clean run.

The loops' layout can change how many passes the fixed point takes only by changing a bit, so passes_to_certificate is capped, case by
case, at what the loops had before the change (PASSES below: recorded from the parent of the commit that introduced this file, same
input, one MI355X).

Measured on one MI355X (44 cases, 4 s).  Worst column against the restatement (bar 2e-5 of its span) / against the one-chunk run,
over the six chunk lengths under EPS_F / EPS_B: M = 64 1.1e-6 / 4.8e-6, fp64 scans 7.0e-7 / 4.7e-6, jumps 9.4e-7 / 5.9e-6, M = 16
1.8e-6 / 5.7e-6, M = 65 6.8e-7 / 5.0e-6 (no bound applies there, see above); under the bitwise fixed point at 1, 2, 3 rows 3.3e-7 /
1.4e-6 (bound 6e-6); through the halo 3.3e-7 / 2.2e-6 (bound 6e-6), 4 passes.  Passes to the certificate: those of the parent in every
case (834 at chunks of one row of M = 64 down to 27 at 33 rows; 1 336 under the bitwise fixed point).
"""
import numpy as np
import pytest

from test_gpu_gamma import RH_B, TH_B, _onepop
from test_gpu_parity import LL_TOL, STAT_TOL, oracle_estep  # noqa: F401  (check_rows applies them)
from test_gpu_seams import EPS_B, EPS_F, SHORT, _rows, check_rows, seq_bound

pytestmark = pytest.mark.gpu

CHUNKS = [1, 2, 3, 5, 17, 33]
ONE = 10 ** 9
JUMP = {"SMCPP_SS_JUMP": "8", "SMCPP_SS_LIGHT_F": "2", "SMCPP_SS_LIGHT_B": "2"}
# id -> (M, switches, states per lane)
CONFIGS = {"M64": (64, {}, 1), "M64_fp64": (64, {"SMCPP_SS_MIXED": "0"}, 1), "M64_jump": (64, JUMP, 1), "M16": (16, {}, 1), "M65": (65, {}, 2)}
EXACT = (1e-30, 1e-30)
TOLS = {"cert": (EPS_F, EPS_B), "exact": EXACT}
JUMP_M1 = (7, 8, 9, 15, 16, 17, 24)
RUNS = (1, 2, 3, 40)
# passes_to_certificate of the parent on the same case: (config, chunk rows, tolerances) -> passes
PASSES = {
    ('M64', 1, 'cert'): 834, ('M64', 2, 'cert'): 436, ('M64', 3, 'cert'): 272, ('M64', 5, 'cert'): 166, ('M64', 17, 'cert'): 50,
    ('M64', 33, 'cert'): 27, ('M64_fp64', 1, 'cert'): 834, ('M64_fp64', 2, 'cert'): 436, ('M64_fp64', 3, 'cert'): 289,
    ('M64_fp64', 5, 'cert'): 166, ('M64_fp64', 17, 'cert'): 50, ('M64_fp64', 33, 'cert'): 27, ('M64_jump', 1, 'cert'): 834,
    ('M64_jump', 2, 'cert'): 436, ('M64_jump', 3, 'cert'): 272, ('M64_jump', 5, 'cert'): 166, ('M64_jump', 17, 'cert'): 50,
    ('M64_jump', 33, 'cert'): 27, ('M16', 1, 'cert'): 731, ('M16', 2, 'cert'): 357, ('M16', 3, 'cert'): 235,
    ('M16', 5, 'cert'): 141, ('M16', 17, 'cert'): 43, ('M16', 33, 'cert'): 25, ('M65', 1, 'cert'): 871, ('M65', 2, 'cert'): 440,
    ('M65', 3, 'cert'): 276, ('M65', 5, 'cert'): 167, ('M65', 17, 'cert'): 51, ('M65', 33, 'cert'): 29,
    ('M64', 1, 'exact'): 1336, ('M64', 2, 'exact'): 670, ('M64', 3, 'exact'): 448, ('M64', 'halo', False): 4,
    ('M64', 'halo', True): 4, ('M64_fp64', 'halo', False): 4, ('M64_fp64', 'halo', True): 4,
}
_CONTIGS = []
_SEQ = {}


def _contigs():
    if _CONTIGS:
        return _CONTIGS
    from test_gpu_seams import _overwrite
    a, b = _rows(301, 6_000, 64), _rows(302, 3_000, 64)
    nk = a.shape[1] - 1
    mono = (0,) * nk
    het = tuple(int(v) for v in a[(a[:, 0] == 1) & (a[:, 1:] != 0).any(axis=1)][0, 1:])
    pairs = []
    for s in range(1, 12):
        for t in range(1, 12):
            pairs += [(s,) + mono, (t,) + het]
    jumps = []
    for s in JUMP_M1:
        jumps += [(s + 1,) + mono, (1,) + het]
    runs = [(5,) + mono]
    for n in RUNS:
        runs += [(1,) + (het if i % 2 == 0 else mono) for i in range(n)] + [(5,) + mono]
    a = _overwrite(a, 300, pairs + jumps)
    b = _overwrite(b, 200, runs + jumps)
    a[-1] = (11,) + mono
    b[0] = (11, -1) + (0,) * (nk - 1)                   # the missing key
    assert a[0, 0] == 1 and a[-1, 0] == 11 and b[0, 0] == 11 and b[-1, 0] == 1
    sp = a[:, 0]
    assert {(int(x), int(y)) for x, y in zip(sp[:-1], sp[1:])} >= {(s, t) for s in range(1, 12) for t in range(1, 12)}
    sb = "".join("1" if s == 1 else "x" for s in b[:, 0])
    assert all("x" + "1" * n + "x" in sb for n in RUNS)
    for c in (a, b):
        m1 = c[(c[:, 1:] == 0).all(axis=1), 0] - 1
        assert set(JUMP_M1) <= set(m1.tolist())
    _CONTIGS.extend([np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)])
    return _CONTIGS


def _manager(config, chunk, engine_opt, extra=None, eps=(EPS_F, EPS_B)):
    M, switches, _ = CONFIGS[config]
    for k, v in dict(switches, **(extra or {})).items():
        engine_opt(k, v)
    contigs = _contigs()
    im = _onepop(M, contigs, TH_B, RH_B)
    im.set_chunking(chunk, *eps)
    im.save_gamma = True
    return im, contigs


def _assert_plan(config, chunk, im, contigs):
    plan = im.describe()["plan"]
    _, switches, npl = CONFIGS[config]
    assert im.chain_mode() == 5 and plan["scan_chains"] and plan["states_per_lane"] == npl and plan["save_gamma"], plan
    assert plan["power_jumps"]["run"] == ("SMCPP_SS_JUMP" in switches), plan["power_jumps"]
    assert plan["float_scans_in_stored_passes"] == (npl == 1 and switches.get("SMCPP_SS_MIXED") != "0"), plan
    if chunk:
        want = sum(max(1, -(-len(c) // chunk)) for c in contigs)
        assert plan["chunks_forward"] == want == plan["chunks_backward"] and not plan["halo_pass"], (plan, want)
    return plan


def _sequential(config, engine_opt):
    """The same kernels on one chunk per contig and direction: -> (gammas, logliks), once per configuration."""
    if config not in _SEQ:
        one, contigs = _manager(config, ONE, engine_opt)
        one.E_step()
        plan = _assert_plan(config, ONE, one, contigs)
        assert plan["chunks_forward"] == len(contigs) == plan["chunks_backward"]
        _SEQ[config] = ([g.copy() for g in one.gammas], list(one.logliks()))
    return _SEQ[config]


@pytest.mark.parametrize("config,chunk,tol", [(g, c, "cert") for g in CONFIGS for c in CHUNKS] + [("M64", c, "exact") for c in (1, 2, 3)])
def test_every_row_shape_at_every_chunk_length(engine_opt, config, chunk, tol):
    seq = _sequential(config, engine_opt)
    im, contigs = _manager(config, chunk, engine_opt, None, TOLS[tol])
    im.E_step()
    plan = _assert_plan(config, chunk, im, contigs)
    print(f"PASSES ({config!r}, {chunk}, {tol!r}): {plan['passes_to_certificate']},   # chunks {plan['chunks_forward']}, light passes "
          f"{plan['light_passes_forward']} / {plan['light_passes_backward']}, launched {plan['passes_launched']}")
    check_rows(f"{config}, chunks of {chunk} rows, {tol}", im, contigs, seq, seq_bound("A", "fast") if tol == "exact" else None, False)
    assert (config, chunk, tol) in PASSES, "no recorded pass count for this case"
    assert plan["passes_to_certificate"] <= PASSES[(config, chunk, tol)], (config, chunk, tol, plan["passes_to_certificate"])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_one_chunk_per_contig(engine_opt, config):
    seq = _sequential(config, engine_opt)
    im, contigs = _manager(config, ONE, engine_opt)
    im.E_step()
    _assert_plan(config, ONE, im, contigs)
    check_rows(f"{config}, one chunk per contig", im, contigs, seq, seq_bound("A", "fast"), False)


@pytest.mark.parametrize("jump", [False, True])
@pytest.mark.parametrize("config", ["M64", "M64_fp64"])
def test_every_row_shape_through_the_halo(engine_opt, config, jump):
    seq = _sequential(config, engine_opt)
    extra = dict(SHORT, **({"SMCPP_SS_JUMP": "8"} if jump else {}))
    im, contigs = _manager(config, 0, engine_opt, extra)
    im.E_step()
    plan = im.describe()["plan"]
    print(f"PASSES ({config!r}, 'halo', {jump}): {plan['passes_to_certificate']},   # chunks {plan['chunks_forward']} / {plan['chunks_backward']}, "
          f"power_jumps {plan['power_jumps']['run']}")
    assert im.chain_mode() == 5 and plan["halo_pass"] and plan["chunks_forward"] > len(contigs), plan
    assert plan["power_jumps"]["run"] == jump, plan["power_jumps"]
    for k in extra:
        engine_opt(k, None)
    check_rows(f"{config}, halo, jumps {'forced' if jump else 'off'}", im, contigs, seq, seq_bound("A", "fast"), False)
    assert (config, "halo", jump) in PASSES, "no recorded pass count for this case"
    assert plan["passes_to_certificate"] <= PASSES[(config, "halo", jump)], (config, jump, plan["passes_to_certificate"])


@pytest.mark.parametrize("config", ["M64", "M64_jump"])
def test_no_poison_reaches_the_outputs(engine_opt, config):
    engine_opt("SMCPP_DEBUG_POISON", None)
    outs = []
    for poison in (None, "nan"):
        engine_opt("SMCPP_DEBUG_POISON", poison)
        im, contigs = _manager(config, 3, engine_opt)
        im.E_step()
        outs.append(dict(ll=list(im.logliks()), xis=[x.copy() for x in im.xisums], gam=[g.copy() for g in im.gammas],
                         gs=[{k: v.copy() for k, v in d.items()} for d in im.gamma_sums]))
        del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    clean, poisoned = outs
    for k in ("ll", "xis", "gam"):
        for c in range(2):
            assert np.all(np.isfinite(poisoned[k][c])), (k, c)
            assert np.array_equal(np.asarray(clean[k][c]), np.asarray(poisoned[k][c])), (k, c)
    for c in range(2):
        for key, v in clean["gs"][c].items():
            assert np.all(np.isfinite(poisoned["gs"][c][key])) and np.array_equal(v, poisoned["gs"][c][key]), (c, key)
