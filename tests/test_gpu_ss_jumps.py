"""Power jumps of the scan chains (smcpp_amd/csrc/chains_ss.hpp: ss_jump_run, k_ss_jump_tables).

Inside the rows of the dominant key the history walks of the chains - the light passes and the float halo, which store nothing - replace
every P = 8 scan steps behind a row's first position by one mat-vec with the P-th power of the key's operator (SMCPP_SS_JUMP = 16 / 8 / 4
picks the power on inputs of any size, 0 turns the jumps off, unset: power 8 from 200 000 positions on); the stored pass and the re-run pass keep their scan steps.  One small binned contig per
case, 4096 rows cut into 16 chunks of 256 rows by set_chunking, so that light passes, the stored pass and a merge re-run all happen.
Rows of the jump key with span - 1 in SPANS_M1 (one below, at and one above the multiples of 8 up to 33, then 40 and 63) sit
  * on the first and on the last row of a chunk,
  * on both sides of a 64-row descriptor block boundary, seen from the chunk's first row (forward) and from its last row (backward),
  * on a merge-test row (every 16th row of the walk) of either direction,
each value at each kind of place at least once; the rows between them are the synthetic contig's own (span-1 rows of many keys, short
rows of the jump key), and a few long rows of ANOTHER key stay on scan steps.

Every case checks
  1. jumps on, 16 chunks, against the C restatement: log-likelihood (LL_TOL), xi sums, gamma sums and gamma_0 (STAT_TOL) - the bars of
     tests/test_gpu_parity.py;
  2. jumps on against jumps off on ONE chunk per direction: the difference is printed and must stay below the difference between the
     jumps-off run and the restatement on the same case;
  3. the plan: `power_jumps` as expected, chunk and pass counts those of the jumps-off plan, and no more passes to the certificate
     than with scan steps, in a second E-step too;
  4. (M = 64, 48, 32) the jump product itself: with the chunk-boundary iteration told to accept every entry vector, the stored pass runs
     once from what the history passes hand it, and every per-row posterior of jumps on (powers 8, 16, 4) agrees with jumps off.
M = 64, 48, 32 (the two-row instantiation of the scans) and 16; M = 32 with spans above 64 (eigensystem statistics beside jumping
chains); M = 80 (two states per lane) must report no jumps.  With SMCPP_DEBUG_POISON=nan nothing of a fresh allocation may reach the
per-row posteriors through the tables.

Measured on one MI355X.  Check 1, 16 chunks, jumps on against the restatement: log-likelihood 2.6e-09 .. 6.6e-09, xi sums 4.5e-07 ..
6.6e-07, gamma sums 2.0e-07 .. 1.3e-06, gamma_0 1.1e-07 .. 2.1e-07.  Check 2: with one chunk per direction no history pass runs and jumps on
equals jumps off in every bit; jumps off against the restatement there: 2.5e-09 .. 6.6e-09, 2.5e-07 .. 5.1e-07, 2.1e-07 .. 6.4e-07,
7.5e-08 .. 1.6e-07.  Check 3: 6 passes to the certificate (5 with the long rows) in both E-steps, jumps on and off alike.  Check 4: worst
column of jumps on against off 6.3e-07 .. 1.8e-06 of its span over the three cases and three powers (bound 2e-4), always two or three
rows behind a seam; without history passes 0.11 .. 0.22 (must exceed 2e-2)."""
import numpy as np
import pytest

from test_gpu_gamma import RH_B, TH_B, N, _onepop
from test_gpu_parity import LL_TOL, STAT_TOL, oracle_estep

pytestmark = pytest.mark.gpu

ROWS, CHUNK = 4096, 256
SPANS_M1 = [7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 63]
CASES = {"M64": (64, False), "M48": (48, False), "M32": (32, False), "M16": (16, False), "M32_long": (32, True)}
_RUNS = {}


def _contig(long_rows):
    """-> (rows, rows of the other key that carry a long span).  Row numbers below are 1-based engine rows: chunk c holds rows
    256 c + 1 .. 256 (c + 1); the forward walk of a chunk meets row r0 + 1 + j in iteration j, the backward walk row r1 - j."""
    from smcpp_amd import synth
    c = synth.synth_contig(41, 100 * 40 * ROWS, N)[:ROWS].copy()
    assert len(c) == ROWS
    mono = np.zeros(3, dtype=np.int32)
    other = c[(c[:, 0] == 1) & (c[:, 1:] != 0).any(axis=1)][0, 1:].copy()      # a key of a span-1 row that is not the jump key
    S = SPANS_M1
    nch = ROWS // CHUNK

    def put(row, s_m1):
        c[row - 1, 0] = s_m1 + 1
        c[row - 1, 1:] = mono
    for ch in range(nch):
        r0, r1 = CHUNK * ch, CHUNK * (ch + 1)
        if ch > 0:
            put(r0 + 1, S[ch % 14])                       # first row of the chunk
        if ch < nch - 1:
            put(r1, S[(ch + 5) % 14])                     # last row of the chunk
        put(r0 + 64, S[(ch + 3) % 14]); put(r0 + 65, S[(ch + 7) % 14])          # forward iterations 63 | 64
        put(r1 - 63, S[(ch + 9) % 14]); put(r1 - 64, S[(ch + 11) % 14])         # backward iterations 63 | 64
        put(r0 + 1 + 32, S[(ch + 1) % 14])                # forward merge-test row (iteration 32)
        put(r1 - 32, S[(ch + 2) % 14])                    # backward merge-test row
        put(r0 + 1 + 112, S[(ch + 4) % 14]); put(r1 - 112, S[(ch + 6) % 14])    # ... and iteration 112 of either walk
    others = []
    for row in (150, 1200, 2500, 3900):                   # long rows of another key: scan steps
        c[row - 1, 0] = 41
        c[row - 1, 1:] = other
        others.append(row)
    if long_rows:
        for row, s in ((700, 100), (1800, 130), (3000, 200)):
            c[row - 1, 0] = s
            c[row - 1, 1:] = mono
        c[2100 - 1, 0] = 90
        c[2100 - 1, 1:] = other
        others.append(2100)
    c[0] = (1, 1, 0, 0)
    c[-1] = (1, 0, 0, 0)
    return np.ascontiguousarray(c, dtype=np.int32), others


def _run(case, jump, chunk, engine_opt, save_gamma=False, eps=None, light=None):
    """One manager, two E-steps on the same parameters: the outputs and the plan of the first, the plan of the second (`plan2`: its
    launch count follows the passes the first one needed).  eps: the tolerance of the chunk-boundary iteration; light: the number of
    history passes of either direction (None: the engine's own)."""
    key = (case, jump, chunk, save_gamma, eps, light)
    if key in _RUNS:
        return _RUNS[key]
    M, long_rows = CASES[case]
    contig, _ = _contig(long_rows)
    engine_opt("SMCPP_SS_JUMP", jump)
    engine_opt("SMCPP_SS_LIGHT_F", light)
    engine_opt("SMCPP_SS_LIGHT_B", light)
    im = _onepop(M, [contig], TH_B, RH_B)
    if eps is None:
        im.set_chunking(chunk)
    else:
        im.set_chunking(chunk, eps, eps)
    im.save_gamma = save_gamma
    im.E_step()
    assert im.chain_mode() == 5
    keys = im.keys
    ep = im.emission_probs
    out = dict(ll=im.loglik(), xis=im.xisums[0].copy(), gs={k: v.copy() for k, v in im.gamma_sums[0].items()}, g0=im.gammas[0][:, 0].copy(),
               gam=im.gammas[0].copy() if save_gamma else None, plan=im.describe()["plan"], pi=np.array(im.pi), T=np.array(im.transition),
               keys=np.array(keys), E=np.array([ep[tuple(k)] for k in keys.tolist()]), contig=contig)
    im.E_step()
    out["plan2"] = im.describe()["plan"]
    for name in ("SMCPP_SS_JUMP", "SMCPP_SS_LIGHT_F", "SMCPP_SS_LIGHT_B"):
        engine_opt(name, None)
    _RUNS[key] = out
    return out


def _diff(a, b):
    """-> (log-likelihood, xi sums, gamma sums, gamma_0): relative differences in the metric of the bars."""
    dl = abs(a["ll"] - b["ll"]) / abs(b["ll"])
    dx = float(np.max(np.abs(a["xis"] - b["xis"]) / np.abs(b["xis"])))
    dg = max(float(np.max(np.abs(a["gs"][k] - v)) / max(np.abs(v).max(), 1e-300)) for k, v in b["gs"].items())
    d0 = float(np.max(np.abs(a["g0"] - b["g0"]) / np.maximum(np.abs(b["g0"]), 1e-300)))
    return dl, dx, dg, d0


def _oracle(r):
    o = oracle_estep(r["pi"], r["T"], r["keys"], r["E"], r["contig"], save_gamma=False)
    return dict(ll=o["loglik"], xis=o["xisum"], gs=o["gamma_sums"], g0=o["gamma"][:, 0])


@pytest.mark.parametrize("case", sorted(CASES))
def test_jumps_against_restatement_and_against_scan_steps(engine_opt, case):
    M, long_rows = CASES[case]
    on = _run(case, "8", CHUNK, engine_opt)          # (named: these contigs are below the size from which jumps are the default)
    off = _run(case, "0", CHUNK, engine_opt)
    # 3. the plan
    pj, plan = on["plan"]["power_jumps"], on["plan"]
    jk = [int(i) for i in np.nonzero((on["keys"] == 0).all(axis=1))[0]]
    assert pj["eligible"] and pj["run"] and pj["powers"] == [8] and [pj["key"]] == jk, pj
    assert not off["plan"]["power_jumps"]["eligible"] and not off["plan"]["power_jumps"]["run"], off["plan"]["power_jumps"]
    assert plan["chunks_forward"] == ROWS // CHUNK == plan["chunks_backward"], plan
    for k in ("chunks_forward", "chunks_backward", "light_passes_forward", "light_passes_backward", "passes_launched", "wavefronts_per_simd",
              "halo_pass", "positions", "eigen_free_statistics"):
        assert plan[k] == off["plan"][k], (k, plan[k], off["plan"][k])
    assert plan["light_passes_forward"] > 0 and plan["light_passes_backward"] > 0 and plan["passes_launched"] >= 4, plan
    # ... and the fixed point is reached no later than with scan steps: the passes to the certificate of the first E-step (whose launch
    # count is fixed up front) and of the second, and the launch count of the second, which follows what the first one needed
    print(f"{case}: passes to the certificate, first / second E-step: jumps on {plan['passes_to_certificate']} / "
          f"{on['plan2']['passes_to_certificate']}, off {off['plan']['passes_to_certificate']} / {off['plan2']['passes_to_certificate']}; "
          f"launched by the second: {on['plan2']['passes_launched']} / {off['plan2']['passes_launched']}")
    assert plan["passes_to_certificate"] <= off["plan"]["passes_to_certificate"], (plan, off["plan"])
    assert on["plan2"]["passes_to_certificate"] <= off["plan2"]["passes_to_certificate"], (on["plan2"], off["plan2"])
    assert on["plan2"]["passes_launched"] <= off["plan2"]["passes_launched"], (on["plan2"], off["plan2"])
    if long_rows:
        assert plan["max_span"] == 200, plan
        print(f"{case}: eigen-free statistics {plan['eigen_free_statistics']}")
    # 1. against the restatement
    assert sorted(on["gs"]) == sorted(_oracle(on)["gs"])
    dl, dx, dg, d0 = _diff(on, _oracle(on))
    print(f"{case}: jumps on, {ROWS // CHUNK} chunks, against the restatement: loglik {dl:.2e}, xi sums {dx:.2e}, gamma sums {dg:.2e}, gamma_0 {d0:.2e}")
    assert dl <= LL_TOL and dx <= STAT_TOL and dg <= STAT_TOL and d0 <= STAT_TOL
    # 2. one chunk: jumps on against jumps off, and jumps off against the restatement.  (One chunk runs no history pass, so this holds
    # with 0 on the left: it pins that the stored passes are the scan steps' own.  The yardstick of the jump product itself is
    # test_entry_vectors_of_the_jumping_history_against_scan_steps below.)
    on1 = _run(case, "8", 10 ** 9, engine_opt)
    off1 = _run(case, "0", 10 ** 9, engine_opt)
    assert on1["plan"]["chunks_forward"] == 1 and on1["plan"]["power_jumps"]["run"] and not off1["plan"]["power_jumps"]["run"]
    d_on = _diff(on1, off1)
    d_off = _diff(off1, _oracle(off1))
    print(f"{case}: one chunk, jumps on against off: loglik {d_on[0]:.2e}, xi sums {d_on[1]:.2e}, gamma sums {d_on[2]:.2e}, gamma_0 {d_on[3]:.2e}; "
          f"off against the restatement: {d_off[0]:.2e}, {d_off[1]:.2e}, {d_off[2]:.2e}, {d_off[3]:.2e}")
    for name, a, b in zip(("loglik", "xi sums", "gamma sums", "gamma_0"), d_on, d_off):
        assert a < b, (case, name, a, b)


def test_small_inputs_jump_only_when_asked(engine_opt):
    unset = _run("M64", None, CHUNK, engine_opt)
    assert not unset["plan"]["power_jumps"]["eligible"] and unset["plan"]["positions"] < 200000, unset["plan"]


def test_two_states_per_lane_never_jump(engine_opt):
    from smcpp_amd import synth
    engine_opt("SMCPP_SS_JUMP", "8")
    contig = np.ascontiguousarray(synth.synth_contig(41, 100 * 40 * 1500, N)[:1500], dtype=np.int32)
    im = _onepop(80, [contig], TH_B, RH_B)
    im.E_step()
    plan = im.describe()["plan"]
    assert plan["states_per_lane"] == 2 and plan["scan_chains"], plan
    assert plan["power_jumps"] == dict(eligible=False, run=False, key=-1, key_slot=-1, powers=[])


ENTRY_BOUND = 2e-4
ENTRY_SENSITIVE = 2e-2


@pytest.mark.parametrize("case", ["M64", "M48", "M32"])
def test_entry_vectors_of_the_jumping_history_against_scan_steps(engine_opt, case):
    """The jump product itself.  With a tolerance of 1e3 the chunk-boundary iteration accepts every entry vector as it comes: the re-run
    pass skips every chunk, so the stored pass runs ONCE, from the end vectors the two history passes handed it, and nothing corrects
    them afterwards.  Every per-row posterior then shows its chunk's entry vectors, forward and backward, most of all in the rows next
    to a seam.  Jumps on (powers 8, 16 and 4: other tables, other counts of jumps and of scan steps left over) against jumps off, every
    entry of every column, relative to the column's mass (its span):
      * both sides walk the same 2 x 1 400 positions of history from the same start, so what differs is the arithmetic of the history
        alone: float steps against float jumps.  A float step rounds at 6e-8 some ten times, and the chains forget with an e-fold of
        240 / 340 positions, so at most ~300 steps' worth of rounding is alive in an entry vector: 300 x 6e-7 = 2e-4 if every rounding
        pulled the same way - ENTRY_BOUND;
      * a wrong table entry, column order or diagonal, or a jump that advances by the wrong number of positions, moves an entry vector
        by 1e-2 and more (one position too many or too few in each of the ~20 jump rows of the last e-fold is 20 / 240);
      * that the posteriors do show their entry vectors is itself checked: without history passes (entry = pi / the uniform vector) the
        same comparison must come out above ENTRY_SENSITIVE."""
    EPS = 1e3
    off = _run(case, "0", CHUNK, engine_opt, save_gamma=True, eps=EPS, light="2")
    assert off["plan"]["light_passes_forward"] == 2 == off["plan"]["light_passes_backward"], off["plan"]
    print(f"{case}: tolerance {EPS:g}: passes to the certificate {off['plan']['passes_to_certificate']}, launched {off['plan']['passes_launched']}")
    span = np.concatenate([[1.0], off["contig"][:, 0].astype(float)])
    for power in ("8", "16", "4"):
        on = _run(case, power, CHUNK, engine_opt, save_gamma=True, eps=EPS, light="2")
        assert on["plan"]["power_jumps"]["run"] and on["plan"]["power_jumps"]["powers"] == [int(power)], on["plan"]
        assert on["plan"]["light_passes_forward"] == 2 == on["plan"]["light_passes_backward"], on["plan"]
        d = np.abs(on["gam"] - off["gam"]).max(axis=0) / span
        j = int(d.argmax())
        print(f"{case}, power {power}: entry vectors of the jumping history against the scan steps': worst column {j} "
              f"({j % CHUNK} rows behind a seam): {d[j]:.2e} of its span (bound {ENTRY_BOUND:.0e})")
        assert d[j] <= ENTRY_BOUND, (case, power, j, d[j])
    bare = _run(case, "0", CHUNK, engine_opt, save_gamma=True, eps=EPS, light="0")
    assert bare["plan"]["light_passes_forward"] == 0 == bare["plan"]["light_passes_backward"], bare["plan"]
    d = np.abs(bare["gam"] - off["gam"]).max(axis=0) / span
    print(f"{case}: no history passes against two: worst column {int(d.argmax())}: {d.max():.2e} of its span (must exceed {ENTRY_SENSITIVE:.0e})")
    assert d.max() >= ENTRY_SENSITIVE, (case, d.max())


@pytest.mark.parametrize("power", ["16", "4"])
def test_other_powers(engine_opt, power):
    """SMCPP_SS_JUMP = 16 and 4 on the M = 64 case: the restatement's bars."""
    on = _run("M64", power, CHUNK, engine_opt)
    assert on["plan"]["power_jumps"]["powers"] == [int(power)] and on["plan"]["power_jumps"]["run"]
    dl, dx, dg, d0 = _diff(on, _oracle(on))
    print(f"M64, power {power}: loglik {dl:.2e}, xi sums {dx:.2e}, gamma sums {dg:.2e}, gamma_0 {d0:.2e}")
    assert dl <= LL_TOL and dx <= STAT_TOL and dg <= STAT_TOL and d0 <= STAT_TOL


def test_no_poison_reaches_the_posteriors_through_the_tables(engine_opt):
    """SMCPP_DEBUG_POISON=nan fills the fresh power tables (and alpha, beta) with NaN: every per-row posterior of a save_gamma E-step -
    a product of a stored alpha and beta row - is finite and bitwise what the clean run gives."""
    engine_opt("SMCPP_DEBUG_POISON", None)
    clean = _run("M48", "8", CHUNK, engine_opt, save_gamma=True)
    engine_opt("SMCPP_DEBUG_POISON", "nan")
    _RUNS.pop(("M48", "8", CHUNK, True, None, None))
    poisoned = _run("M48", "8", CHUNK, engine_opt, save_gamma=True)
    engine_opt("SMCPP_DEBUG_POISON", None)
    _RUNS.pop(("M48", "8", CHUNK, True, None, None))
    assert poisoned["plan"]["power_jumps"]["run"]
    for k in ("ll", "xis", "g0", "gam"):
        assert np.all(np.isfinite(poisoned[k])), k
        assert np.array_equal(np.asarray(clean[k]), np.asarray(poisoned[k])), k
