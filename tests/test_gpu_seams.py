"""Per-row posteriors at the chunk seams of the scan chains (chain families 5 and 6), under every plan that cuts a contig.

The scan chains are the one approximately parallel part of an E-step: a contig is cut into chunks, one per wavefront and direction,
and every chunk but the first starts from a vector that is only known once its neighbour has run.  What makes the seams exact is
a stack of cooperating pieces (float light passes, the halo, the per-entry certificate eps_f / eps_b, the merge re-run, the second
round of run_chains_ss).  Every case below

  1. builds its input ONCE per family with hand-placed features ON the seams it will have: the seams are read back from the engine
     (`im.chunks()`, smcpp_debug_chunks) on a first construction, and the features are then written over the positions around
     them (`_overwrite` keeps every position outside its window where it was, so the seams of all plans - which are targets in
     POSITIONS - stay put and one input, one run of the restatement, serves every plan of the family);
  2. asserts from the getter that the features are where the case needs them, and from describe()["plan"] the plan it ran;
  3. checks every column of every contig against the C restatement (check_gamma_columns, LL_TOL, STAT_TOL: the project's bars);
  4. checks every entry of every column against the SEQUENTIAL run of the same kernels (set_chunking(10**9): one chunk per contig,
     no history, no fixed point):  |g_plan - g_seq| <= 2 (eps_f + eps_b) / (1 - kappa) * max(g_seq, 1e-3 span).
     The certificate accepts an entering vector whose entries moved by at most eps_f (forward) / eps_b (backward) relative; a
     column is alpha o beta over its own sum, which carries the same error once more.  kappa is the contraction of a
     perturbation over one chunk (1 024 positions, the floor): accepted changes of successive chunks add up to eps / (1 - kappa).
     Fast model: kappa < 0.05, taken as 0.  Slow models: KAPPA_SLOW, measured from the restatement alone (below).

Models.  Fast: theta, rho of the synthetic benchmark per 100 bp bin.  Slow, A: the same theta and 0.3 rho; B (rows four times as
long: the same data on a four times finer scale of positions): theta / 4 and 0.04 rho.  (Scaling theta down with rho makes these
inputs forget FASTER - A: 3 231 positions at 0.1 theta, 0.1 rho - because the heterozygous sites of the fixed data then say more
than the transitions; and rows with spans drawn at random forget within ~4 000 positions whatever rho is, so the rows keep the
spans the generator gave them.)  Measured by test_inputs_forget_as_claimed from two runs of the restatement, one on the contig
and one on the contig without its first 500 rows: positions until alpha_hat agrees to 1e-6 relative per entry on 200 rows in a
row; kappa = the worst ratio of the largest relative difference one chunk (1 024 positions) further on to the difference where
it is taken, over the rows where that is above 1e-4:

  input                  model   forgetting length (positions)   kappa over 1 024 positions
  A (M = 64, n = 8)      fast     3 896                          0.046
  A (M = 64, n = 8)      slow    20 385                          0.705
  B (M = 100, n = 8)     fast     1 385                          0.0001
  B (M = 100, n = 8)     slow    17 799                          1.03 (no contraction over one chunk: the derived bound is void)

The full forward halo is 2 800 + 800 = 3 600 positions: the slow inputs must not forget within 3 x 3 600 = 10 800.

One chunk count serves both directions of these inputs: at 60 000 positions the 1 024-position floor, not the wavefront count, sets
the number of chunks, so SMCPP_SS_FWD_SHARE = 0.3 leaves the two lists' seams on the same rows (the case stays, as a plan of its own);
the case with 0.03 has 26 forward seams against 62 backward ones and is the one where the seams of the two directions differ.

The module takes about 75 s on one MI355X: 66 s of restatement (shared per family and model), 0.1 s of E-steps, the rest inputs.
"""
import time

import numpy as np
import pytest

from test_gpu_gamma import RH_B, TH_B, N, _edged, _het_run, _onepop, _tiny, _twopop
from test_gpu_parity import LL_TOL, STAT_TOL, check_gamma_columns, oracle_estep

EPS_F, EPS_B = 2e-6, 1e-6          # the certificate's tolerances, handed to the engine by every case (set_chunking(0, EPS_F, EPS_B))
FLOOR = 1024                       # positions: no chunk of the automatic plan is shorter
HALO = dict(LF=2800, DF=800, LB=3900, DB=1100)           # the engine's default halo lengths (make_chunks)
FAST = (TH_B, RH_B)
SLOW = {"A": (TH_B, 0.3 * RH_B), "B": (TH_B / 4, 0.04 * RH_B)}
R0 = 500                           # rows removed in front for the forgetting measurement
FORGET_MIN_SLOW = 3 * (HALO["LF"] + HALO["DF"])
KAPPA_FAST_MAX = 0.1
# contraction over one chunk that the slow cases' bound against the sequential run divides by; None: the restatement shows no
# contraction below 1 over 1 024 positions (B: 1.03), the derived bound is void and the restatement's bars are what binds
KAPPA_SLOW = {"A": 0.75, "B": None}
HET = 60                           # heterozygous run: long enough that the stored vector touches the 1e-10 floor


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(seed, positions, max_span, n=N, twopop=False, stretch=1):
    """Binned synthetic rows cut to about `positions` positions, spans capped at max_span; first and last row span 1.  stretch > 1:
    the span > 1 rows that many times as long (the same data at a coarser scale of positions: few rows, many chunks, rows to cut)."""
    from smcpp_amd import synth
    bp = 100 * positions + 4000
    c = (synth.synth_contig_twopop(seed, bp, 4, 3) if twopop else synth.synth_contig(seed, bp, n)).copy()
    c[:, 0] = np.minimum(np.where(c[:, 0] > 1, c[:, 0] * stretch, 1), max_span)
    cut = int(np.searchsorted(np.cumsum(c[:, 0]), positions))
    assert 0 < cut < len(c), (cut, len(c))
    return _edged(c[:cut], ncol=c.shape[1])


def _overwrite(c, start, rows):
    """Positions start + 1 .. start + sum(spans of rows) of contig c replaced by `rows`; the rows they cut keep their key and
    what is left of their span.  Every position outside the window stays where it was."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.int32))
    cum = np.concatenate([[0], np.cumsum(c[:, 0])])
    end = start + int(rows[:, 0].sum())
    assert 1 <= start and end < cum[-1] - 1, (start, end, cum[-1])
    i = int(np.searchsorted(cum, start, "right")) - 1        # row i (0-based) holds position start + 1
    j = int(np.searchsorted(cum, end, "left")) - 1           # row j holds position end
    head, tail = c[i].copy(), c[j].copy()
    head[0] = start - cum[i]
    tail[0] = cum[j + 1] - end
    parts = [c[:i]] + ([head[None]] if head[0] > 0 else []) + [rows] + ([tail[None]] if tail[0] > 0 else []) + [c[j + 1:]]
    out = np.ascontiguousarray(np.vstack(parts), dtype=np.int32)
    assert out[:, 0].sum() == cum[-1]
    return out


def _mono(span, ncol):
    r = np.zeros((1, ncol), dtype=np.int32)
    r[0, 0] = span
    return r


def engine_spans(contig, cut):
    """Spans of the engine's own rows: a caller's row of span s is ceil(s / 64) rows where long rows are cut."""
    if not cut:
        return contig[:, 0].astype(np.int64)
    out = []
    for s in contig[:, 0].tolist():
        out += [64] * (s // 64) + ([s % 64] if s % 64 else [])
    return np.array(out, dtype=np.int64)


def seam_rows(ch, contig):
    """Seams of contig `contig` in a chunk list of the getter: the r0 of every chunk but the first (engine rows)."""
    ch = ch[ch[:, 0] == contig]
    return ch[1:, 1].astype(np.int64)


def seam_targets(ch, contig, total):
    """make_chunks' own targets in positions: seam j of nc chunks sits at the first row whose cumulative cost reaches total (j+1) / nc."""
    nc = int(np.sum(ch[:, 0] == contig))
    return [total * (j + 1) // nc for j in range(nc - 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# families: id -> (M, builder of the base contigs, manager, switches that decide the cut of long rows / the family)
# ---------------------------------------------------------------------------------------------------------------------------------
def _base_A():
    # a 60 000-position contig (58 chunks per direction at the floor), one shorter than the forward halo between it and a second
    # long one (its halos clamp at its first and last row), a single-chunk contig, a one-row and a two-row contig
    return [_rows(101, 60_000, 64), _rows(102, 2_500, 64), _rows(103, 6_000, 64), _rows(104, 1_100, 64)] + _tiny(64)


def _base_B(M):
    return [_rows(111, 120_000 if M <= 100 else 24_000, 300, stretch=4), _rows(112, 2_500, 300, stretch=4)] + _tiny(300)


def _base_C():
    from smcpp_amd import synth
    return [_edged(synth.synth_posterior_contig(3000, N, seed=31).copy(), nb=N)] + _tiny(100_000, nb=N)


def _base_D():
    return [_rows(121, 40_000, 64, twopop=True), _rows(122, 2_500, 64, twopop=True)] + _tiny(40, ncol=7)


FAMILIES = {"A": 64, "A32": 32, "A13": 13, "B100": 100, "B256": 256, "C": 64, "D": 48}
SHARE = {"SMCPP_SS_FWD_SHARE": "0.03"}        # few, long forward chunks against the floor's many backward ones
_INPUT = {}


def _model(fam, model):
    return FAST if model == "fast" else SLOW[fam[0]]


def _manager(fam, contigs, model=FAST):
    M = FAMILIES[fam]
    if fam == "D":
        return _twopop(M, contigs)
    if fam == "C":
        return _onepop(M, contigs, 2e-4, 6e-5)
    return _onepop(M, contigs, *model)


def _base(fam):
    return _base_B(FAMILIES[fam]) if fam[0] == "B" else _base_C() if fam == "C" else _base_D() if fam == "D" else _base_A()


def family_input(fam, engine_opt):
    """The contigs of a family with the features on their seams (contig 0 carries them), built once."""
    if fam in _INPUT:
        return _INPUT[fam]
    contigs = _base(fam)
    c = contigs[0]
    ncol = c.shape[1]
    if fam == "C":
        # cost units, not positions (a long row costs SS_HYB_COST): the run is INSERTED in front of an early seam's row; the cost
        # units it adds move that seam by a few rows, less than the run's length
        for back in (False, True):
            im = _manager(fam, [c] + contigs[1:])
            s = seam_rows(im.chunks(back), 0)
            assert len(s) >= 7, ("hybrid plan: fewer than eight chunks", len(s))
            # (row r is the first whose cumulative cost reaches the target; the three rows in front of it cost 3 .. 24 units)
            r = int(s[1 if back else 0])
            c = np.ascontiguousarray(np.vstack([c[:r - 4], _het_run(50, nb=N), c[r - 4:]]), dtype=np.int32)
            del im
        _INPUT[fam] = [c] + contigs[1:]
        return _INPUT[fam]
    im = _manager(fam, contigs)
    cut = bool(im.describe()["plan"]["long_rows_cut"])
    total = int(c[:, 0].sum())
    chf, chb = im.chunks(False), im.chunks(True)
    del im
    tf, tb = seam_targets(chf, 0, total), seam_targets(chb, 0, total)
    assert len(tf) >= 10 and len(tb) >= 10, (len(tf), len(tb))
    sp = engine_spans(c, cut)
    cum = np.concatenate([[0], np.cumsum(sp)])
    pf, pb = cum[seam_rows(chf, 0)], cum[seam_rows(chb, 0)]      # the seams in positions, as cut
    nb = 0 if ncol == 4 else 0
    het = _het_run(HET, ncol=ncol, nb=nb)
    k = len(tf)
    at = lambda q: max(1, min(k - 2, int(q * k)))                 # seam number at a fraction of the contig
    # (the windows below are disjoint and at least 300 positions from every seam they are not meant for)
    windows = []

    def put(c, start, rows):
        end = start + int(np.atleast_2d(rows)[:, 0].sum())
        assert all(end + 64 < a or b + 64 < start for a, b in windows), ("features collide", start, end, windows)
        windows.append((start, end))
        return _overwrite(c, start, rows)
    c = put(c, tf[at(0.08)] - HET // 2, het)                                     # a run of heterozygous sites across a seam
    c = put(c, tf[at(0.15)] - 32, _mono(64, ncol))                               # span 64, last row before a seam
    c = put(c, tf[at(0.21)], _mono(64, ncol))                                    # span 64, first row behind a seam
    if cut:
        c = put(c, tf[at(0.26)] - 64, _mono(150, ncol))                          # a seam between two pieces of one cut row
    # halo boundaries (positions counted back / ahead from the seam) inside a span-64 row: default lengths, the float-only
    # halo of the mid-size plan, the short halo of 300
    j = at(0.34); c = put(c, int(pf[j]) - HALO["DF"] - HALO["LF"] - 32, _mono(64, ncol))
    c = put(c, int(pf[j]) - HALO["DF"] - 32, _mono(64, ncol))
    j = at(0.42); c = put(c, int(pb[j]) + HALO["DB"] - 32, _mono(64, ncol))
    c = put(c, int(pb[j]) + HALO["DB"] + HALO["LB"] - 32, _mono(64, ncol))
    j = at(0.55); c = put(c, int(pf[j]) - HALO["LF"] - 32, _mono(64, ncol))
    j = at(0.60); c = put(c, int(pb[j]) + HALO["LB"] - 32, _mono(64, ncol))
    j = at(0.72); c = put(c, int(pf[j]) - 300 - 32, _mono(64, ncol))
    j = at(0.80); c = put(c, int(pb[j]) + 300 - 32, _mono(64, ncol))
    if fam[0] == "A":
        # the plan with few forward chunks: a run across one of ITS forward seams, a span-64 row in front of another
        for kk, v in SHARE.items():
            engine_opt(kk, v)
        im = _manager(fam, [c] + contigs[1:])
        t3 = seam_targets(im.chunks(False), 0, total)
        del im
        for kk in SHARE:
            engine_opt(kk, None)
        far = [t for t in t3 if t > 0.84 * total and min(abs(t - u) for u in tb) > 200]
        assert len(far) >= 2, (t3, "no forward seam of the unequal plan clear of the backward seams")
        c = put(c, far[0] - HET // 2, het)
        c = put(c, far[1] - 32, _mono(64, ncol))
    assert c[0, 0] == 1 and c[-1, 0] == 1 and int(c[:, 0].sum()) == total
    _INPUT[fam] = [c] + contigs[1:]
    return _INPUT[fam]


# ---------------------------------------------------------------------------------------------------------------------------------
# the features, as the getter shows them
# ---------------------------------------------------------------------------------------------------------------------------------
def seam_features(contig, cut, chf, chb, lens):
    """Which hand-placed features sit on the seams of contig 0 in THIS plan -> dict of counts.  lens = (LF, DF, LB, DB) of the plan's
    halo or None."""
    sp = engine_spans(contig, cut)
    L = len(sp)
    cum = np.concatenate([[0], np.cumsum(sp)])
    # engine row -> caller's row (0-based), to tell the pieces of one cut row
    owner = np.repeat(np.arange(len(contig)), [max(1, -(-int(s) // 64)) for s in contig[:, 0]]) if cut else np.arange(len(contig))
    hetrow = (contig[:, 0] == 1) & (contig[:, 1] == 1) & (contig[:, 2] == 0) if contig.shape[1] == 4 else (contig[:, 0] == 1) & (contig[:, 1] == 1)
    het = hetrow[owner]
    # rows i (1-based) with het[i - 6 .. i + 5] all set: a seam behind row i has six heterozygous rows on either side
    run = np.convolve(het.astype(int), np.ones(12, dtype=int), "full")
    inrun = lambda r: 6 <= r <= L - 6 and run[r + 5] == 12
    f = dict(het_fwd=0, het_bwd=0, s64_before=0, s64_behind=0, pieces=0, halo_float=0, halo_exact=0, clamp_first=0, clamp_last=0)
    sf, sb = seam_rows(chf, 0), seam_rows(chb, 0)
    f["het_fwd"] = sum(inrun(int(r)) for r in sf)
    f["het_bwd"] = sum(inrun(int(r)) for r in sb)
    for r in np.concatenate([sf, sb]).tolist():
        f["s64_before"] += int(sp[r - 1] == 64 and owner[r - 1] != owner[min(r, L - 1)] and (r < 2 or owner[r - 2] != owner[r - 1]))
        f["s64_behind"] += int(r < L and sp[r] == 64 and owner[r] != owner[r - 1] and (r + 1 >= L or owner[r + 1] != owner[r]))
        f["pieces"] += int(r < L and owner[r] == owner[r - 1])
    if lens is not None:
        LF, DF, LB, DB = lens
        for _, r0, r1, h0, h1 in chf[chf[:, 0] == 0][1:].tolist():
            assert 0 <= h0 <= h1 <= r0, (r0, h0, h1)
            e1, e0 = cum[r0] - DF, cum[r0] - DF - LF
            if e0 > 0 and sp[h0] == 64 and cum[h0] < e0 < cum[h0 + 1]:
                f["halo_float"] += 1
            if DF > 0 and e1 > 0 and sp[h1] == 64 and cum[h1] < e1 < cum[h1 + 1]:
                f["halo_exact"] += 1
        for _, r0, r1, h0, h1 in chb[chb[:, 0] == 0][:-1].tolist():
            assert L >= h0 >= h1 >= r1, (r1, h0, h1)
            e1, e0 = cum[r1] + DB, cum[r1] + DB + LB
            if e0 < cum[L] and sp[h0 - 1] == 64 and cum[h0 - 1] < e0 < cum[h0]:
                f["halo_float"] += 1
            if DB > 0 and e1 < cum[L] and sp[h1 - 1] == 64 and cum[h1 - 1] < e1 < cum[h1]:
                f["halo_exact"] += 1
        # clamping: a halo that would start in front of its contig's first row or behind its last one
        f["clamp_first"] = int(np.sum((chf[:, 3] == 0) & (chf[:, 1] > 0)))
        for cc, r0, r1, h0, h1 in chb.tolist():
            f["clamp_last"] += int(r1 < h0 == chb[chb[:, 0] == cc][:, 2].max())
    return f


def assert_halo_rows(case, contigs, cut, chf, chb, lens):
    """Every chunk's halo rows are the ones the documented lengths give, counted in positions from the chunk's OWN first (forward) or
    last (backward) row and clamped to its contig: forward h = the last row that ends at or in front of the boundary, backward the
    first row that ends at or behind it; the first forward and the last backward chunk of a contig have none."""
    LF, DF, LB, DB = lens if lens is not None else (0, 0, 0, 0)
    for c, ob in enumerate(contigs):
        cum = np.concatenate([[0], np.cumsum(engine_spans(ob, cut))])
        L = len(cum) - 1
        f, b = chf[chf[:, 0] == c], chb[chb[:, 0] == c]
        assert f[0, 1] == 0 and f[-1, 2] == L and np.array_equal(f[1:, 1], f[:-1, 2]), (case, c, "forward chunks do not tile the contig")
        assert b[0, 1] == 0 and b[-1, 2] == L and np.array_equal(b[1:, 1], b[:-1, 2]), (case, c, "backward chunks do not tile the contig")
        for j, (_, r0, r1, h0, h1) in enumerate(f.tolist()):
            e1, e0 = cum[r0] - DF, cum[r0] - DF - LF
            w1 = 0 if e1 <= 0 else int(np.searchsorted(cum, e1, "right")) - 1
            w0 = 0 if e0 <= 0 else int(np.searchsorted(cum, e0, "right")) - 1
            want = (r0, r0) if j == 0 or LF + DF == 0 else (min(w0, w1, r0), min(w1, r0))
            assert (h0, h1) == want, (case, "forward halo", c, j, (r0, r1, h0, h1), want)
        for j, (_, r0, r1, h0, h1) in enumerate(b.tolist()):
            e1, e0 = cum[r1] + DB, cum[r1] + DB + LB
            want = (r1, r1) if j == len(b) - 1 or LB + DB == 0 else (min(L, int(np.searchsorted(cum, e0, "left"))), min(L, int(np.searchsorted(cum, e1, "left"))))
            assert (h0, h1) == want, (case, "backward halo", c, j, (r0, r1, h0, h1), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# plans: id -> (family, model, switches, expected plan, halo lengths or None, features the seams of this plan must carry)
# ---------------------------------------------------------------------------------------------------------------------------------
H1 = {"SMCPP_SS_HALO": "1"}
MID = {"SMCPP_SS_HALO": "1", "SMCPP_HALO_DF": "0", "SMCPP_HALO_DB": "0", "SMCPP_SS_WPC": "2"}
SHORT = {"SMCPP_SS_HALO": "1", "SMCPP_HALO_LF": "300", "SMCPP_HALO_LB": "300", "SMCPP_HALO_DF": "0", "SMCPP_HALO_DB": "0"}
NOLIGHT = {"SMCPP_SS_LIGHT_F": "0", "SMCPP_SS_LIGHT_B": "0"}
L_DEF = (HALO["LF"], HALO["DF"], HALO["LB"], HALO["DB"])
L_MID = (HALO["LF"], 0, HALO["LB"], 0)
L_SHORT = (300, 0, 300, 0)
SEAM = ("het_fwd", "het_bwd", "s64_before", "s64_behind")


def _plans():
    p = {}
    for fam in ("A", "A32", "A13"):
        one = dict(states_per_lane=1, chain_family=5, float_scans_in_stored_passes=True)
        p[f"{fam}:auto"] = (fam, "fast", {}, dict(one, halo_pass=False, wavefronts_per_simd=1, light="some"), None, SEAM)
        p[f"{fam}:nolight"] = (fam, "fast", NOLIGHT, dict(one, halo_pass=False, wavefronts_per_simd=1, light="none"), None, SEAM)
        p[f"{fam}:halo"] = (fam, "fast", H1, dict(one, halo_pass=True, wavefronts_per_simd=1, light="none"), L_DEF,
                            SEAM + ("halo_float", "halo_exact", "clamp_first", "clamp_last"))
        p[f"{fam}:mid"] = (fam, "fast", MID, dict(one, halo_pass=True, wavefronts_per_simd=2, light="none"), L_MID,
                           SEAM + ("halo_float", "clamp_first", "clamp_last"))
        p[f"{fam}:wpc3"] = (fam, "fast", {"SMCPP_SS_WPC": "3"}, dict(one, halo_pass=False, wavefronts_per_simd=3, light="some"), None, SEAM)
        p[f"{fam}:short"] = (fam, "fast", SHORT, dict(one, halo_pass=True, wavefronts_per_simd=1, light="none"), L_SHORT,
                             SEAM + ("halo_float",))
        p[f"{fam}:share0.3"] = (fam, "fast", {"SMCPP_SS_FWD_SHARE": "0.3"},
                                dict(one, halo_pass=False, wavefronts_per_simd=1, light="some"), None, SEAM)
        p[f"{fam}:share0.03"] = (fam, "fast", SHARE, dict(one, halo_pass=False, wavefronts_per_simd=1, light="any", unequal=True), None, SEAM)
        f64 = dict(one, float_scans_in_stored_passes=False)
        p[f"{fam}:auto:fp64"] = (fam, "fast", {"SMCPP_SS_MIXED": "0"}, dict(f64, halo_pass=False, wavefronts_per_simd=1, light="some"), None, SEAM)
        p[f"{fam}:halo:fp64"] = (fam, "fast", dict(H1, SMCPP_SS_MIXED="0"), dict(f64, halo_pass=True, wavefronts_per_simd=1, light="none"),
                                 L_DEF, SEAM + ("halo_float", "halo_exact"))
    # the slow model (M = 64): every halo-entered row is wrong after the first pass
    one = dict(states_per_lane=1, chain_family=5, float_scans_in_stored_passes=True)
    p["A:auto:slow"] = ("A", "slow", {}, dict(one, halo_pass=False, wavefronts_per_simd=1, light="some"), None, SEAM)
    p["A:halo:slow"] = ("A", "slow", H1, dict(one, halo_pass=True, wavefronts_per_simd=1, light="none"), L_DEF, SEAM + ("halo_float", "halo_exact"))
    p["A:mid:slow"] = ("A", "slow", MID, dict(one, halo_pass=True, wavefronts_per_simd=2, light="none"), L_MID, SEAM + ("halo_float",))
    p["A:short:slow"] = ("A", "slow", SHORT, dict(one, halo_pass=True, wavefronts_per_simd=1, light="none"), L_SHORT, SEAM + ("halo_float",))
    for fam, npl in (("B100", 2), ("B256", 4)):
        for model in ("fast", "slow"):
            sfx = "" if model == "fast" else ":slow"
            b = dict(states_per_lane=npl, chain_family=5, float_scans_in_stored_passes=False, long_rows_cut=True)
            p[f"{fam}:halo{sfx}"] = (fam, model, {}, dict(b, halo_pass=True, wavefronts_per_simd=1, light="none"), L_DEF,
                                     SEAM + ("pieces", "halo_float", "halo_exact", "clamp_first", "clamp_last"))
            p[f"{fam}:nohalo{sfx}"] = (fam, model, {"SMCPP_SS_HALO": "0"}, dict(b, halo_pass=False, wavefronts_per_simd=1, light="some"), None,
                                       SEAM + ("pieces",))
            p[f"{fam}:wpc2{sfx}"] = (fam, model, {"SMCPP_SS_WPC": "2"}, dict(b, halo_pass=True, wavefronts_per_simd=2, light="none"), L_DEF,
                                     SEAM + ("pieces", "halo_float", "halo_exact"))
    hy = dict(states_per_lane=1, chain_family=6, float_scans_in_stored_passes=False, halo_pass=False, light="none")
    p["C:auto"] = ("C", "fast", {}, dict(hy, wavefronts_per_simd=1, min_chunks=8), None, ("het_fwd", "het_bwd"))
    p["C:wpc2"] = ("C", "fast", {"SMCPP_SS_WPC": "2"}, dict(hy, wavefronts_per_simd=2, min_chunks=8), None, ("het_fwd", "het_bwd"))
    tw = dict(states_per_lane=1, chain_family=5, float_scans_in_stored_passes=True, wavefronts_per_simd=1)
    p["D:auto"] = ("D", "fast", {}, dict(tw, halo_pass=False, light="some"), None, SEAM)
    p["D:halo"] = ("D", "fast", H1, dict(tw, halo_pass=True, light="none"), L_DEF, SEAM + ("halo_float", "halo_exact", "clamp_first", "clamp_last"))
    return p


PLANS = _plans()
_PASSES = {}        # plan id -> passes_to_certificate of its first E-step (the slow cases compare with their fast twins)
_SEQ = {}           # (family, model, float scans?) -> the sequential run's gammas
_TIMES = {"oracle": 0.0, "device": 0.0}


def assert_plan(case, plan, want, n_contigs):
    print(f"{case}: plan " + ", ".join(f"{k} {plan[k]}" for k in (
        "chain_family", "states_per_lane", "chunks_forward", "chunks_backward", "wavefronts_per_simd", "halo_pass", "light_passes_forward",
        "light_passes_backward", "float_scans_in_stored_passes", "long_rows_cut", "passes_to_certificate", "passes_launched")))
    assert plan["scan_chains"] and plan["save_gamma"], (case, plan)
    assert plan["chunks_forward"] > n_contigs and plan["chunks_backward"] > n_contigs, (case, plan)
    for k, v in want.items():
        if k == "light":
            lf, lb = plan["light_passes_forward"], plan["light_passes_backward"]
            assert v == "any" or (lf > 0 and lb > 0) == (v == "some") and (lf == 0 and lb == 0) == (v == "none"), (case, lf, lb, v)
        elif k == "unequal":
            assert plan["chunks_forward"] != plan["chunks_backward"], (case, plan)
        elif k == "min_chunks":
            assert min(plan["chunks_forward"], plan["chunks_backward"]) - (n_contigs - 1) >= v, (case, plan)
        else:
            assert plan[k] == v, (case, k, plan[k], v)


def setup_case(fam, model, switches, engine_opt):
    contigs = family_input(fam, engine_opt)
    for k, v in switches.items():
        engine_opt(k, v)
    im = _manager(fam, contigs, _model(fam, model))
    auto = [im.chunks(False).copy(), im.chunks(True).copy()]
    im.set_chunking(0, EPS_F, EPS_B)              # the test and the engine share one pair of tolerances ...
    assert np.array_equal(im.chunks(False), auto[0]) and np.array_equal(im.chunks(True), auto[1]), "set_chunking(0, ..) left the automatic plan"
    im.save_gamma = True
    return im, contigs


def sequential(fam, model, switches, contigs, key=None, prepare=None):
    """The same kernels on one chunk per contig and direction (nothing to iterate): -> (gammas, logliks)."""
    key = key or (fam, model, switches.get("SMCPP_SS_MIXED") == "0")
    if key not in _SEQ:
        im = _manager(fam, contigs, _model(fam, model))
        im.set_chunking(10**9, EPS_F, EPS_B)
        if prepare:
            prepare(im)
        im.save_gamma = True
        im.E_step()
        plan = im.describe()["plan"]
        assert plan["chunks_forward"] == len(contigs) == plan["chunks_backward"] and not plan["halo_pass"], plan
        assert len(im.chunks()) == len(contigs)
        _SEQ[key] = ([g.copy() for g in im.gammas], list(im.logliks()))
    return _SEQ[key]


def check_rows(case, im, contigs, seq, bound, cut):
    """Every column of every contig against the restatement and against the sequential run; one line with the worst of each and
    its distance from the nearest seam of either direction."""
    M = im.M
    keys = im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    pi, T = im.pi, im.transition
    lls, gams, xis, gss = im.logliks(), im.gammas, im.xisums, im.gamma_sums
    chf, chb = im.chunks(False), im.chunks(True)
    assert len(gams) == len(contigs)
    worst_o, worst_s = (0.0, -1, -1, -1), (0.0, -1, -1, -1)
    for c, ob in enumerate(contigs):
        t0 = time.time()
        o = oracle_estep(pi, T, keys, Etab, ob)
        _TIMES["oracle"] += time.time() - t0
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * max(1.0, abs(o["loglik"])), (case, c, lls[c], o["loglik"])
        assert gams[c].shape == (M, len(ob) + 1)
        check_gamma_columns(gams[c], o["gamma"], ob, arg_dev=im.gamma_argmax(c), label=f"{case} contig {c}")
        assert np.max(np.abs(xis[c] - o["xisum"]) / np.abs(o["xisum"])) <= STAT_TOL, (case, c, "xisum")
        assert sorted(gss[c].keys()) == sorted(o["gamma_sums"].keys())
        for k, v in o["gamma_sums"].items():
            assert np.max(np.abs(gss[c][k] - v)) <= STAT_TOL * max(np.abs(v).max(), 1e-300), (case, c, k)
        # distance in positions of every caller's row from the nearest seam
        spans = np.concatenate([[1.0], ob[:, 0].astype(float)])
        cumu = np.concatenate([[0], np.cumsum(ob[:, 0])])                  # cumu[l]: end of row l
        cume = np.concatenate([[0], np.cumsum(engine_spans(ob, cut))])
        seams = np.unique(np.concatenate([cume[seam_rows(chf, c)], cume[seam_rows(chb, c)]]))
        dist = np.abs(cumu[:, None] - seams[None, :]).min(axis=1) if len(seams) else np.full(len(cumu), -1)
        eo = np.abs(gams[c] - o["gamma"]).max(axis=0) / spans
        j = int(eo.argmax())
        if eo[j] > worst_o[0]:
            worst_o = (float(eo[j]), c, j, int(dist[j]))
        gs = seq[0][c]
        assert gs.shape == gams[c].shape
        es = (np.abs(gams[c] - gs) / np.maximum(gs, 1e-3 * spans)).max(axis=0)
        j = int(es.argmax())
        if es[j] > worst_s[0]:
            worst_s = (float(es[j]), c, j, int(dist[j]))
        if bound is not None:
            bad = np.nonzero(es > bound)[0]
            assert len(bad) == 0, f"{case} contig {c}: {len(bad)} columns differ from the sequential run by more than {bound:.2e} " \
                                  f"(relative, entries floored at 1e-3 of the span), e.g. columns {bad[:8]}, {es[bad[:8]]}, " \
                                  f"positions from a seam {dist[bad[:8]]}"
    print(f"{case}: seams forward {len(chf) - len(contigs)}, backward {len(chb) - len(contigs)}; worst column against the restatement "
          f"{worst_o[0]:.2e} of its span (contig {worst_o[1]}, column {worst_o[2]}, {worst_o[3]} positions from a seam); against the "
          f"sequential run {worst_s[0]:.2e} relative (contig {worst_s[1]}, column {worst_s[2]}, {worst_s[3]} positions from a seam), "
          f"bound {bound if bound is None else format(bound, '.2e')}")
    return worst_o, worst_s


def seq_bound(fam, model):
    b = 2.0 * (EPS_F + EPS_B)
    if model == "fast":
        return b
    return None if KAPPA_SLOW[fam[0]] is None else b / (1.0 - KAPPA_SLOW[fam[0]])


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
def _measure_forgetting(M, contig, model):
    """-> (positions until alpha_hat of the run without the first R0 rows agrees with the whole run's to 1e-6 per entry on 200 rows
    in a row (-1: never), kappa over FLOOR positions).  The restatement alone, on the host preparation's parameters."""
    from oracle import oracle
    from smcpp_amd import _engine, synth
    a, s = synth.model_pieces()
    keys = np.unique(contig[:, 1:], axis=0).astype(np.int32)
    pi, T, E = _engine.host_prep_onepop(N, synth.hidden_states(M), 0.5, a, s, model[0], model[1], 1.0, keys)
    o1 = oracle.estep(pi, T, keys, E, contig)
    o2 = oracle.estep(pi, T, keys, E, contig[R0:])
    a1, a2 = o1["alpha_hat"][R0 + 1:].astype(float), o2["alpha_hat"][1:].astype(float)
    d = np.max(np.abs(a1 - a2) / np.maximum(np.abs(a1), 1e-300), axis=1)
    pos = np.cumsum(contig[R0:, 0])
    ok = np.convolve((d <= 1e-6).astype(int), np.ones(200, dtype=int), "valid")
    i = np.nonzero(ok == 200)[0]
    flen = int(pos[i[0]]) if len(i) else -1
    j = np.searchsorted(pos, pos + FLOOR)
    use = (j < len(pos)) & (d > 1e-4)
    kappa = float(np.max(d[j[use]] / d[use])) if use.any() else 0.0
    return flen, kappa


@pytest.mark.parametrize("fam,M", [("A", 64), ("B", 100)])
def test_inputs_forget_as_claimed(fam, M):
    """No GPU: the fast inputs forget a wrong start within the forward halo the engine is tuned to, the slow ones do not within three
    times that, and the contraction over one chunk that the slow cases' bound divides by is what the restatement shows."""
    contig = (_base_A() if fam == "A" else _base_B(M))[0]
    if fam == "B":
        contig = contig[:len(contig) // 3]          # (M^3 per row: a third of the contig, 40 000 positions, shows the same lengths)
    total = int(contig[R0:, 0].sum())
    ff, kf = _measure_forgetting(M, contig, FAST)
    fs, ks = _measure_forgetting(M, contig, SLOW[fam])
    print(f"{fam} (M = {M}, {total} positions behind row {R0}): fast forgets in {ff} positions (kappa {kf:.3f}), slow in {fs} (kappa {ks:.3f})")
    assert 0 < ff <= HALO["LF"] + HALO["DF"] + FLOOR, ff
    assert kf <= KAPPA_FAST_MAX, kf
    assert fs < 0 or fs > FORGET_MIN_SLOW, fs
    assert fs < 0 or fs < total, fs
    assert KAPPA_SLOW[fam] is None or ks <= KAPPA_SLOW[fam], ks


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PLANS))
def test_seams(engine_opt, case):
    """One chunk plan: the plan and the features on its seams asserted, then every column of every contig against the restatement and
    against the sequential run of the same kernels.

    Measured on one MI355X (worst column of a case, all contigs).  Against the restatement, in units of the row's span (bar 2e-5):
    fast model 2.1e-7 - 1.4e-6, slow model 3.2e-7 - 1.9e-6.  Against the sequential run, relative with entries floored at 1e-3 of
    the span: A / A32 / A13 fast 5.6e-7 - 3.5e-6 (bound 6e-6), A slow 4.4e-6 - 5.6e-6 (bound 2.4e-5), B fast 5.9e-7 - 2.3e-6
    (bound 6e-6), B slow 2.9e-6 - 3.4e-6 (no bound: kappa >= 1), C 2.0e-6, D 2.1e-6 - 3.0e-6.  The worst columns lie anywhere
    between 1 and 500 positions from a seam: the distance to the sequential run is the float noise of alpha_hat, not a seam error.
    Passes to the certificate, fast -> slow: A light passes 6 -> 19, halo 2 -> 15, two wavefronts + float halo 2 -> 16, halo of
    300 positions 5 -> 18; B M = 100 halo 3 -> 16, no halo 8 -> 19; M = 256 halo 2 -> 10, no halo 7 -> 15."""
    fam, model, switches, want, lens, feats = PLANS[case]
    im, contigs = setup_case(fam, model, switches, engine_opt)
    t0 = time.time()
    im.E_step()
    _TIMES["device"] += time.time() - t0
    plan = im.describe()["plan"]
    assert_plan(case, plan, want, len(contigs))
    cut = bool(plan["long_rows_cut"])
    chf, chb = im.chunks(False), im.chunks(True)
    assert len(chf) == plan["chunks_forward"] and len(chb) == plan["chunks_backward"]
    if fam != "C":
        assert_halo_rows(case, contigs, cut, chf, chb, lens)
    f = seam_features(contigs[0], cut, chf, chb, lens)
    print(f"{case}: features on the seams of contig 0: {f}")
    for k in feats:
        assert f[k] >= 1, f"{case}: no '{k}' on a seam of this plan: {f}"
    if case.endswith("share0.03"):
        assert len(np.setdiff1d(seam_rows(chf, 0), seam_rows(chb, 0))) >= len(seam_rows(chf, 0)) // 2
    _PASSES[case] = plan["passes_to_certificate"]
    if model == "slow":
        twin = case[:-len(":slow")]
        if twin not in _PASSES:                    # (run on its own: the fast twin's E-step, for its pass count)
            fim, _ = setup_case(fam, "fast", switches, engine_opt)
            fim.E_step()
            _PASSES[twin] = fim.describe()["plan"]["passes_to_certificate"]
        print(f"{case}: {plan['passes_to_certificate']} passes to the certificate, the fast model {_PASSES[twin]}")
        assert plan["passes_to_certificate"] > _PASSES[twin], (case, plan["passes_to_certificate"], _PASSES[twin])
        if case in ("A:halo:slow", "A:short:slow"):
            assert plan["passes_launched"] > 6, (case, plan)       # the second round of run_chains_ss: the statistics redone
    seq = sequential(fam, model, switches, contigs)
    check_rows(case, im, contigs, seq, seq_bound(fam, model), cut)
    if fam in ("A", "B100") and model == "fast":
        # the run of heterozygous sites decodes the last state, and drives entries of the stored vector onto the floor
        keys = im.keys
        ep = im.emission_probs
        o = oracle_estep(im.pi, im.transition, keys, np.array([ep[tuple(k)] for k in keys.tolist()]), contigs[0])
        assert np.any(o["gamma"][:, 1:].argmax(axis=0) == im.M - 1)
        assert float(o["alpha_hat"][1:].min()) <= 1.0001e-10, float(o["alpha_hat"][1:].min())
    print(f"(so far: restatement {_TIMES['oracle']:.1f} s, E-steps {_TIMES['device']:.2f} s)")


@pytest.mark.gpu
@pytest.mark.parametrize("halo", [False, True])
def test_seams_warm_start(engine_opt, halo):
    """Warm start (the previous E-step's boundary vectors): an E-step, a 2 % parameter step, an E-step, a jump, an E-step; every
    row after each one.  With SMCPP_SS_HALO=1 the first E-step enters through the halo and the warm ones must not."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    contigs = family_input("A", engine_opt)
    if halo:
        engine_opt("SMCPP_SS_HALO", "1")
    a0, s = synth.model_pieces()
    rng = np.random.default_rng(7)
    steps = [a0, a0 * (1.0 + 0.02 * rng.standard_normal(len(a0))), a0[::-1] * 2.5]
    im = _manager("A", contigs)
    im.set_chunking(0, EPS_F, EPS_B)
    im.set_warm_start(True)
    im.save_gamma = True
    model = PiecewiseModel(a0, s, 1e4, "pop1")
    im.model = model
    for it, a in enumerate(steps):
        model[:] = a
        im.E_step()
        plan = im.describe()["plan"]
        case = f"A:warm{':halo' if halo else ''}:step{it}"
        assert_plan(case, plan, dict(states_per_lane=1, chain_family=5, warm_start=True, halo_pass=(halo and it == 0),
                                     wavefronts_per_simd=1), len(contigs))

        def prepare(m, a=a):
            m.model = PiecewiseModel(a, s, 1e4, "pop1")
        seq = sequential("A", "fast", {}, contigs, key=("A", "warm", it), prepare=prepare)
        check_rows(case, im, contigs, seq, seq_bound("A", "fast"), False)
