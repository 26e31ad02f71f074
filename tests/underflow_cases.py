"""Inputs with long rows (span > 1) of RARE keys, shared by tests/test_underflow_cases.py (CPU: the cases stay where they are meant
to be against the bound, the restatement is a good reference on them) and tests/test_gpu_underflow.py (the engine on them).

The scan chains (chains_ss.hpp) walk a row of span s in s steps WITHOUT rescaling, so a manager refuses them when some row has
s log(min_h E[key][h]) < -450 (engine_plans.hpp: ss_extract_generators on a host table; prep_dev.hpp: k_prep_csfs raises DevPrep
flag 2 on a device table, and estep() redoes the E-step on the dense kernels).  Everywhere else in the suite a long row carries the
monomorphic or the missing key, whose emission vector is O(1) in every state: nothing comes near that bound.  Here the long rows
carry segregating keys.  With synth.model_pieces(), synth.hidden_states(M), n = 8, theta = 2.5e-2, rho = 6.25e-3 the host
preparation gives, for M = 8 .. 300 alike (tests/test_underflow_cases.py recomputes and asserts the classes):

    key (a, b, nb)   log min_h E   log max_h E
    (0, 0, 8)           -0.6          -0.1
    (0, 1, 8)           -4.4          -3.9
    (1, 0, 0)           -8.3          -0.8
    (1, 1, 8)          -12.7          -3.2

  near   span x log min in [-445, -400]: inside the bound on the smallest entry.  (1,0,0) x 50 (-415), (1,1,8) x 34 (-433) and,
         while rows are not cut (M <= 64), (0,1,8) x 100 (-440).  Beyond 64 states the engine cuts rows at 64 positions: (0,1,8) x
         100 is then two pieces, 64 + 36, of a rare key (-282 at worst).  The scan chains were meant to take all three.  They cannot:
         the scan steps carry float intermediates, and span x log MAX_h E is -108 for the second row and -388 (-248 per piece) for
         the third - the row's evidence is below e^-87 whatever the data (measured: NaN; prep_dev.hpp: SS_SPAN_LOG_MAX = -80, the
         bound this finding added).  Class "near": the largest entry passes that bound; "near_small" / "cut_small": it does not.
  near64 the first two `near` rows alone (M <= 64): no row is longer than 64 positions, so the table stays on the device.
  near_run  (1,0,0) x 50 alone: the one `near` row the scans can take (its largest entry gives e^-42); beyond 64 states one
         monomorphic run has 100 positions, so that the manager cuts rows.  near_run60: the same on 60 rows (M = 300).
  edge_run / edge_redo  rows that pass BOTH table bounds and differ in what the scans then compute: the engine also guards on the
         evidence c of every scanned row (kernels.hpp: |log c| <= 80, else the E-step is redone on the dense kernels), because
         max_h(E)^span only bounds c from above and c lies 2 to 14 below it on these contigs.  edge_run: (0,1,8) x 19 (log c -75.8),
         (0,1,8) x 20 (-78.0), (1,1,8) x 17 - the scans must take them; edge_redo: (1,1,8) x 24 (-87, below FLT_MIN), (1,1,8) x 23 -
         the guard must send them to the redo.  log c from tests/llref.py, asserted on the CPU with a margin of 1.5 around 80.
         Beyond 64 states one monomorphic run has 100 positions (rows are cut).
  past   below -450, but the dominant states do not underflow: (1,0,0) x 64 (-531; its largest entry gives e^-51), (1,1,8) x 40 (-508).
  past_one  (1,0,0) x 64 alone, for the manager that crosses the bound: theta x 5 (CROSS) raises log min E of (1,0,0) from -8.3 to
         -6.7 and brings this row to -428 (largest entry: -4).  theta x 20, which looks better for this row (-339), sends the
         MONOMORPHIC runs past the bound instead (log E of (0,0,8) falls to -12.4 / -2.2: 59 positions give -733 / -129), and (1,1,8)
         x 40 stays refused at either scale (largest entry: -96): `past` itself does not cross.
  deep   every state underflows in `span` plain steps (M <= 64, where rows up to 512 positions are scanned): (0,1,8) x 400
         (-1760 at best, e^-1560 at the largest entry), (1,1,8) x 300.
  mixed  a contig without special rows, then one with the `past` rows (contig_base != 0), then a one-row contig: a `past` row.
  hybrid un-binned rows (theta = 2e-4, rho = 6e-5, M = 64), the longest monomorphic row above 512 so that the hybrid plan is taken;
         (1,0,0) x 5 000 - an eigen-power step, which the bound exempts - and (1,0,0) x 6, scanned and far from the bound.
  twopop test_gpu_gamma.twopop_contigs with ONE long row of a segregating two-population key, key and span chosen on the CPU from
         the host table (`twopop_case`) so that it passes the bound.

A one-population contig has about 120 rows: every third row is a monomorphic run of 2 .. 59 positions, the others span-1 sites of
mixed keys, the first and the last row have span 1.  Special rows REPLACE monomorphic runs chosen by hand, so two span-1 rows lie
between any two of them.
"""
import numpy as np

N = 8
ROWS = 120
TH_B, RH_B = 2.5e-2, 6.25e-3          # per 100 bp bin (test_gpu_gamma.TH_B, RH_B)
TH_U, RH_U = 2e-4, 6e-5               # per base pair (test_gpu_gamma.TH_U, RH_U)
BOUND = -450.0                        # the engine's (ss_extract_generators, k_prep_csfs)
MARGIN = 5.0                          # a last-bit difference between a device and a host table must not move a case across it
CROSS = 5.0                           # the theta scale of the manager that crosses the bound (past_one)
CUT = 64                              # beyond 64 states the engine cuts rows into pieces of at most 64 positions

MONO, MISSING = (0, 0, N), (-1, 0, 0)
K_100, K_118, K_018 = (1, 0, 0), (1, 1, N), (0, 1, N)
# kind -> [(key, span, class)]; classes: the docstring and tests/test_underflow_cases.py
SMALL = -85.0                         # span x log(max_h E) below this: the largest-entry bound (-80) refuses the row, with the margin
LARGE = -75.0                         # ... above this: it does not ("near" rows; edge rows only have to pass the bound itself)
EVIDENCE, EVIDENCE_MARGIN = 80.0, 1.5 # the engine's guard on |log c| of a scanned row; how far the edge rows keep from it
SPECIAL = {"near": [(K_100, 50, "near"), (K_118, 34, "near_small"), (K_018, 100, "near_small")],
           "near64": [(K_100, 50, "near"), (K_118, 34, "near_small")],
           "near_cut": [(K_100, 50, "near"), (K_118, 34, "near_small"), (K_018, 100, "cut_small")],
           "near_run": [(K_100, 50, "near")],
           "near_run_cut": [(K_100, 50, "near")],           # + a monomorphic run of 100 positions
           "near_run60": [(K_100, 50, "near")],             # 60 rows, for M = 300; + the monomorphic run of 100 positions
           "past": [(K_100, 64, "past"), (K_118, 40, "past")],
           "edge_run": [(K_018, 19, "edge_run"), (K_018, 20, "edge_run"), (K_118, 17, "edge_run")],
           "edge_redo": [(K_118, 24, "edge_redo"), (K_118, 23, "edge_redo")],
           "past_one": [(K_100, 64, "past")],               # the `past` row that theta x CROSS brings inside both bounds
           "deep": [(K_018, 400, "deep"), (K_118, 300, "deep")],
           "plain": []}
SLOTS = (13, 49, 85)                  # the monomorphic runs (row index % 3 == 1) the special rows replace


def plain_contig(seed, rows=ROWS, n=N, span_hi=60):
    """Every third row a monomorphic run of 2 .. span_hi - 1 positions, the others span-1 sites of mixed keys ((a, b, n), a = 0
    or 1, never the monomorphic key); first and last row span 1."""
    rng = np.random.default_rng(seed)
    c = np.zeros((rows, 4), dtype=np.int32)
    c[:, 0] = 1
    a = rng.integers(0, 2, rows)
    c[:, 1] = a
    c[:, 2] = np.where(a == 1, rng.integers(0, n + 1, rows), rng.integers(1, n + 1, rows))
    c[:, 3] = n
    run = np.arange(rows) % 3 == 1
    run[-1] = False
    c[run] = 0
    c[run, 0] = rng.integers(2, span_hi, int(run.sum()))
    c[run, 3] = n
    assert c[0, 0] == 1 and c[-1, 0] == 1
    return c


def with_special(c, special, slots=SLOTS):
    c = c.copy()
    for at, (key, span, _) in zip(slots, special):
        assert c[at, 0] > 1 and tuple(c[at, 1:]) == MONO and c[at - 1, 0] == 1 and c[at + 1, 0] == 1
        c[at] = (span, *key)
    return np.ascontiguousarray(c, dtype=np.int32)


def kind_for(name, M):
    """The SPECIAL list a case takes at M states."""
    if name == "near":
        return "near" if M <= CUT else "near_cut"
    if name in ("near_run", "edge_run", "edge_redo"):
        return name if M <= CUT else name + "_cut"
    if name == "deep":
        assert M <= CUT, "deep rows are scanned whole only up to 64 states"
    return name


_CASES = {}


def case(name, M):
    """-> dict(contigs, theta, rho, special): special = [(contig, row, key, span, class)].  Built once per (name, kind)."""
    if name == "hybrid":
        assert M == 64
    kind = name if name in ("mixed", "hybrid") else kind_for(name, M)
    if kind in _CASES:
        return _CASES[kind]
    if kind == "mixed":
        past = SPECIAL["past"]
        contigs = [plain_contig(301), with_special(plain_contig(302), past), np.array([[past[0][1], *past[0][0]]], dtype=np.int32)]
        special = [(1, at, *sp) for at, sp in zip(SLOTS, past)] + [(2, 0, *past[0])]
        r = dict(contigs=contigs, theta=TH_B, rho=RH_B, special=special)
    elif kind == "hybrid":
        c = plain_contig(401, span_hi=3000)
        c[7, 0], c[61, 0] = 100_000, 513                     # (monomorphic runs: the hybrid plan needs a row above 512)
        sp = [(K_100, 5000, "hybrid"), (K_100, 6, "scanned")]
        r = dict(contigs=[with_special(c, sp)], theta=TH_U, rho=RH_U, special=[(0, at, *s) for at, s in zip(SLOTS, sp)])
    elif kind in ("near_run_cut", "near_run60"):
        c = plain_contig(260, rows=60) if kind == "near_run60" else plain_contig(261)
        c[31, 0] = 100                                       # (a monomorphic run: rows are cut beyond 64 states)
        sp = SPECIAL[kind]
        r = dict(contigs=[with_special(c, sp)], theta=TH_B, rho=RH_B, special=[(0, at, *s) for at, s in zip(SLOTS, sp)])
    elif kind in ("edge_run", "edge_redo", "edge_run_cut", "edge_redo_cut"):
        c = plain_contig(270)
        if kind.endswith("_cut"):
            c[31, 0] = 100                                   # (a monomorphic run: rows are cut beyond 64 states)
        sp = SPECIAL[kind[:-4] if kind.endswith("_cut") else kind]
        r = dict(contigs=[with_special(c, sp)], theta=TH_B, rho=RH_B, special=[(0, at, *s) for at, s in zip(SLOTS, sp)])
    else:
        sp = SPECIAL[kind]
        r = dict(contigs=[with_special(plain_contig(200 + len(kind)), sp)], theta=TH_B, rho=RH_B,
                 special=[(0, at, *s) for at, s in zip(SLOTS, sp)])
    _CASES[kind] = r
    return r


def key_list(contigs):
    """The sorted distinct keys of the contigs (the order the managers keep)."""
    return np.unique(np.vstack([c[:, 1:] for c in contigs]), axis=0).astype(np.int32)


def host_table(M, contigs, theta, rho, n=N):
    """(pi, T, keys, E) of the host preparation of the synthetic model."""
    from smcpp_amd import _engine, synth
    a, s = synth.model_pieces()
    keys = key_list(contigs)
    pi, T, E = _engine.host_prep_onepop(n, synth.hidden_states(M), 0.5, a, s, theta, rho, 1.0, keys)
    return pi, T, keys, E


def special_rows(obs):
    """Indices of the rows of span > 1 whose key is neither monomorphic on the full sample nor missing."""
    obs = np.asarray(obs)
    k = obs[:, 1:]
    usual = np.all(k == np.array(MONO), axis=1) | (k[:, 0] == -1) if k.shape[1] == 3 else \
        (np.all(k[:, [0, 1, 3, 4]] == 0, axis=1) | (k[:, 0] == -1))
    return np.nonzero((obs[:, 0] > 1) & ~usual)[0]


def bound(prep_table, keys, obs, cut):
    """Per special row of `obs` (`special_rows`): (row, span_piece x log(min_h E), span_piece x log(max_h E)), span_piece =
    min(span, cut): `cut` is 64 where the engine cuts rows (M > 64), otherwise at least the span."""
    E = np.asarray(prep_table, dtype=np.float64)
    lut = {tuple(int(x) for x in k): i for i, k in enumerate(np.asarray(keys))}
    out = []
    for r in special_rows(obs):
        e = E[lut[tuple(int(x) for x in obs[r, 1:])]]
        piece = min(int(obs[r, 0]), int(cut))
        out.append((int(r), piece * float(np.log(e.min())), piece * float(np.log(e.max()))))
    return out


def bound_of_key(prep_table, keys, key, span):
    """(span x log min, span x log max) of one key."""
    E = np.asarray(prep_table, dtype=np.float64)
    e = E[[tuple(int(x) for x in k) for k in np.asarray(keys)].index(tuple(key))]
    return np.array([span * np.log(e.min())]), np.array([span * np.log(e.max())])


def cut_for(M):
    return CUT if M > CUT else 1 << 30


# ---------------------------------------------------------------------------------------------------------------------------------
# two populations (M = 24): test_gpu_gamma.twopop_contigs + one long row of a segregating key
# ---------------------------------------------------------------------------------------------------------------------------------
TWOPOP_M = 24
_TWOPOP = {}


def twopop_host_table(M, contigs):
    """The host preparation test_gpu_gamma._twopop's manager computes (n1 = 4, n2 = 3, a = (2, 0), split 0.3)."""
    from smcpp_amd import _engine, synth
    a, s = synth.model_pieces()
    m2 = (1.5 + 0.5 * np.cos(np.arange(8)), s[:8])
    keys = key_list(contigs)
    pi, T, E = _engine.host_prep_twopop(4, 3, 2, 0, synth.hidden_states(M), 0.5, (a, s), (a, s), m2, 0.3, synth.THETA, synth.RHO,
                                        1.0, keys)
    return pi, T, keys, E


def twopop_case(M=TWOPOP_M):
    """-> dict(contigs, special, key, span, value): the segregating key of the contigs whose smallest emission entry is smallest, on
    a row of the shortest span that puts span x log(min_h E) below BOUND - 4 MARGIN; the row replaces a span > 1 row in the
    middle of the first contig, between two span-1 rows."""
    if M in _TWOPOP:
        return _TWOPOP[M]
    from test_gpu_gamma import twopop_contigs
    contigs = [c.copy() for c in twopop_contigs(60_000)]
    _, _, keys, E = twopop_host_table(M, contigs)
    seg = [i for i, k in enumerate(keys.tolist()) if k[0] >= 0 and k[3] >= 0 and (k[0] + k[1] + k[3] + k[4]) > 0]
    i = min(seg, key=lambda j: E[j].min())
    lm = float(np.log(E[i].min()))
    span = int(np.ceil((BOUND - 4 * MARGIN) / lm))
    c = contigs[0]
    cand = [r for r in range(len(c) // 3, len(c) - 1) if c[r, 0] > 1 and c[r - 1, 0] == 1 and c[r + 1, 0] == 1]
    at = cand[0]
    c[at] = (span, *keys[i])
    r = dict(contigs=contigs, special=[(0, at, tuple(int(x) for x in keys[i]), span, "past")], key=tuple(int(x) for x in keys[i]),
             span=span, value=span * lm)
    _TWOPOP[M] = r
    return r
