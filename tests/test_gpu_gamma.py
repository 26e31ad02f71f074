"""Every per-row posterior route (`save_gamma`: what `smc++ posterior` prints) on every column, at the scale of the row's span.

Column l >= 1 of gamma is the sum of the posteriors of the row's s_l positions, normalised to s_l (hmm.cpp:113-150).  About ten kernels
produce it; which ones run depends on M, the spans, the structure of T and the SMCPP_* switches.  Each case below first asserts the
route it ran (`describe()["plan"]`), so that a change of routing cannot turn it into a copy of another case, and then checks every
column of every contig against the C restatement (oracle/) fed with the engine's own prepared parameters
(test_gpu_parity.check_gamma_columns: per column 2e-5 of the span, the sum to 1e-9, entries of 1e-3 of the span or more to 1e-4
relative, the decoded index).

  route (kernels)                                         how it is reached here
  span-1 rows (k_s1_scalars)                              every case: first and last row of every contig span 1; contigs of 1, 2 rows
  eigensystem, M <= 64 (k_gamma_rows_b<NT>, NT = 1..4)    binned rows, SMCPP_GAMMA_SCAN=0: 1, 15, 16, 17, 64, 65 rows per (contig, key)
  eigensystem, M > 64 (k_span_q + k_gamma_rows_eig)       un-binned rows, SMCPP_SPLIT_SPANS=0 + SMCPP_GAMMA_PIECES=0; unstructured T
  scan steps (k_gamma_rows_scan<NPL>, 1 2 3 4 8 16)       binned rows, spans <= 64 (2, 63 and 64 placed by hand)
  eigen-power pieces (k_piece_rowsums, k_piece_vectors,   un-binned rows, 64 < M <= 256, SMCPP_SPLIT_SPANS=0: spans 64, 65, 128, 129,
    k_gamma_rows_scan<NPL, true>, k_gamma_merge_pieces)     10^5; two contigs, two eigen keys
  rows cut into pieces (k_gamma_merge, merged_gamma)      un-binned rows of at most a few hundred positions at M = 100 / 300
  two populations (7-column rows)                         M = 48 eigensystem, M = 130 scan steps
  chunk boundaries                                        set_chunking(37), binned and un-binned

Each contig holds a run of consecutive heterozygous sites, so that the reference decodes the LAST state on some columns of every
padded width (a decode that never looks at state M - 1 fails).  The restatement runs once per (parameters, contig) and is shared by
the options that reuse a setup.  The whole module takes about 30 s on one MI355X, the restatement included.
"""
import numpy as np
import pytest

from test_gpu_parity import LL_TOL, check_gamma_columns, oracle_estep

pytestmark = pytest.mark.gpu

N = 8                     # haploid sample size of the one-population cases


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _het_run(k, ncol=4, nb=0):
    """k consecutive heterozygous sites (span 1): the reference's posterior sits in the deepest state there."""
    r = np.zeros((k, ncol), dtype=np.int32)
    r[:, 0] = 1
    r[:, 1] = 1
    if ncol == 4:
        r[:, 3] = nb
    return r


def _edged(body, ncol=4, nb=0):
    """First and last row of span 1 (k_s1_scalars writes the first and the last gamma row of the contig)."""
    first = np.zeros((1, ncol), dtype=np.int32); first[0, 0] = 1; first[0, 1] = 1
    last = np.zeros((1, ncol), dtype=np.int32); last[0, 0] = 1
    if ncol == 4:
        first[0, 3] = last[0, 3] = nb
    if body[0, 0] == 1 and body[-1, 0] == 1:
        return np.ascontiguousarray(body, dtype=np.int32)
    return np.ascontiguousarray(np.vstack([first, body, last]), dtype=np.int32)


def _tiny(long_span, ncol=4, nb=0):
    """A contig of one row and a contig of two rows (a long row, then a span-1 row)."""
    one = np.zeros((1, ncol), dtype=np.int32); one[0, 0] = 1; one[0, 1] = 1
    if ncol == 4:
        one[0, 3] = nb
    two = np.zeros((2, ncol), dtype=np.int32); two[:, 0] = (long_span, 1)
    if ncol == 4:
        two[:, 3] = nb
    return [one, two]


def binned_contigs(seed, length, n=N, spans=(2, 63, 64), cap=64):
    """Binned rows (spans <= 64): a synthetic contig with the given spans placed by hand, a run of 30 heterozygous bins, plus the
    one- and two-row contigs."""
    from smcpp_amd import synth
    c = synth.synth_contig(seed, length, n).copy()
    c[:, 0] = np.minimum(c[:, 0], cap)
    long_rows = np.nonzero(c[:, 0] > 1)[0]
    for j, s in enumerate(spans):
        c[long_rows[3 + 7 * j], 0] = s
    mid = len(c) // 2
    c = np.vstack([c[:mid], _het_run(30), c[mid:]])
    return [_edged(c)] + _tiny(max(spans))


def key_batch_contigs(counts=(1, 15, 16, 17, 64, 65), n=N, seed=5):
    """Contig j holds counts[j] span > 1 rows of the monomorphic key and (counts[j] % 5) + 1 of the missing key, between span-1
    sites: the batches of 16 rows per (contig, eigen key) of k_gamma_rows_b end ragged.  (A run of heterozygous sites in the
    longest one.)"""
    rng = np.random.default_rng(seed)
    out = []
    for j, r in enumerate(counts):
        kinds = np.array([0] * r + [1] * (r % 5 + 1))
        rng.shuffle(kinds)
        rows = []
        for k in kinds:
            s1 = np.zeros((int(rng.integers(1, 4)), 4), dtype=np.int32)
            s1[:, 0] = 1
            s1[:, 1] = rng.integers(0, 2, len(s1))
            s1[:, 3] = n
            s1[:, 2] = np.where(s1[:, 1] == 1, rng.integers(0, n + 1, len(s1)), rng.integers(1, n + 1, len(s1)))
            rows.append(s1)
            rows.append(np.array([[int(rng.integers(2, 65)), -1 if k else 0, 0, 0 if k else n]], dtype=np.int32))
        if j == len(counts) - 1:
            rows.append(_het_run(30, nb=0))
        out.append(_edged(np.vstack(rows), nb=n))
    return out


def unbinned_contigs(rows, n=N, seeds=(11, 12), spans=(64, 65, 128, 129, 100_000), cap=None):
    """Un-binned rows (`smc++ posterior`'s input): long monomorphic runs, span-1 sites, missing stretches; the given spans placed by
    hand in every contig, a run of 40 heterozygous sites; plus the one- and two-row contigs."""
    from smcpp_amd import synth
    out = []
    for i, sd in enumerate(seeds):
        c = synth.synth_posterior_contig(rows - 30 * i, n, seed=sd).copy()
        if cap is not None:
            c[:, 0] = np.minimum(c[:, 0], cap)
        mono = np.nonzero((c[:, 0] > 1) & (c[:, 1] == 0))[0]
        for j, s in enumerate(spans):
            c[mono[2 + 5 * j], 0] = s
        mid = len(c) // 3
        c = np.vstack([c[:mid], _het_run(40, nb=n), c[mid:]])
        out.append(_edged(c, nb=n))
    return out + _tiny(max(spans), nb=n)


def twopop_contigs(length, seed=3):
    from smcpp_amd import synth
    c = synth.synth_contig_twopop(seed, length, 4, 3).copy()
    c[:, 0] = np.minimum(c[:, 0], 64)
    mid = len(c) // 2
    c = np.vstack([c[:mid], _het_run(30, ncol=7), c[mid:]])
    return [_edged(c, ncol=7)] + _tiny(40, ncol=7)


# ---------------------------------------------------------------------------------------------------------------------------------
# managers
# ---------------------------------------------------------------------------------------------------------------------------------
def _onepop(M, contigs, theta, rho, n=N):
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel
    a, s = synth.model_pieces()
    im = _smcpp.PyOnePopInferenceManager(n, contigs, synth.hidden_states(M), ("pop1",), 0.5)
    im.model = PiecewiseModel(a, s, 1e4, "pop1")
    im.theta = theta; im.rho = rho; im.alpha = 1.0
    return im


def _unstructured(M, contigs, theta, rho, n=N):
    """set_raw with a reversible T of no structure (real spectrum: the restatement takes LAPACK's eig); pi and the emission table
    from the host preparation of the synthetic model."""
    from smcpp_amd import _engine, _smcpp, synth
    a, s = synth.model_pieces()
    hs = synth.hidden_states(M)
    keys = np.unique(np.vstack([c[:, 1:] for c in contigs]), axis=0).astype(np.int32)
    pi, _, E = _engine.host_prep_onepop(n, hs, 0.5, a, s, theta, rho, 1.0, keys)
    rng = np.random.default_rng(M)
    S = rng.random((M, M)); S = S + S.T + 4.0 * M * np.eye(M)
    T = S / S.sum(axis=1, keepdims=True)
    im = _smcpp.PyOnePopInferenceManager(n, contigs, hs, ("pop1",), 0.5)
    im.theta = theta; im.rho = rho
    im.set_raw(pi, T, keys, E)
    return im


def _twopop(M, contigs):
    from smcpp_amd import _smcpp, synth
    from smcpp_amd.model import PiecewiseModel, TwoPopulationModel
    a, s = synth.model_pieces()
    m1 = PiecewiseModel(a, s, 1e4, pid="pop1")
    m2 = PiecewiseModel(1.5 + 0.5 * np.cos(np.arange(8)), s[:8], 1e4, pid="pop2")
    im = _smcpp.PyTwoPopInferenceManager(4, 3, 2, 0, contigs, synth.hidden_states(M), ("pop1", "pop2"), 0.5)
    im.model = TwoPopulationModel(m1, m2, 0.3)
    im.theta = synth.THETA; im.rho = synth.RHO; im.alpha = 1.0
    return im


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: id -> (inputs, manager, switches, expected plan, oracle runs on the last state?)
# ---------------------------------------------------------------------------------------------------------------------------------
TH_B, RH_B = 2.5e-2, 6.25e-3          # per 100 bp bin (synth)
TH_U, RH_U = 2e-4, 6e-5               # per base pair (un-binned rows)
EIG = "eigensystem"
SCAN = "scan steps"
PIECES = "eigen-power pieces + scan steps"
NO_SCAN = {"SMCPP_GAMMA_SCAN": "0"}
UNCUT = {"SMCPP_SPLIT_SPANS": "0"}
UNCUT_EIG = {"SMCPP_SPLIT_SPANS": "0", "SMCPP_GAMMA_PIECES": "0"}


def _cases():
    c = {}
    # eigensystem, M <= 64: k_gamma_rows_b with NT = Mp / 16 = 1, 1, 2, 3, 4
    for M in (1, 13, 32, 48, 64):
        c[f"eig_b:M{M}"] = ("batches", M, NO_SCAN, 0, dict(per_row_gamma=EIG, states_per_lane=1, long_rows_cut=False, chain_family=5))
    c["eig_b:M48:side0"] = ("batches", 48, dict(NO_SCAN, SMCPP_GAMMA_SIDE="0"), 0,
                            dict(per_row_gamma=EIG, states_per_lane=1, long_rows_cut=False, chain_family=5))
    c["eig_b:M32:binned:chunk37"] = ("binned", 32, NO_SCAN, 37,
                                     dict(per_row_gamma=EIG, states_per_lane=1, long_rows_cut=False, chain_family=5))
    # eigensystem, M > 64: k_span_q + k_gamma_rows_eig (un-binned rows: the streamed-operand chains, family 3; the unstructured T
    # keeps the family the manager was built with and falls back to the dense kernels per E-step)
    for M in (65, 130, 256):
        c[f"eig_big:M{M}"] = ("unbinned", M, UNCUT_EIG, 0,
                              dict(per_row_gamma=EIG, states_per_lane=(M + 63) // 64, long_rows_cut=False, chain_family=3))
    c["eig_big:M96:unstructured"] = ("unstructured", 96, {}, 0,
                                     dict(per_row_gamma=EIG, states_per_lane=2, long_rows_cut=False, chain_family=5))
    # scan steps: k_gamma_rows_scan<NPL>
    for M, npl in ((64, 1), (100, 2), (150, 3), (256, 4), (300, 8), (520, 16)):
        c[f"scan:M{M}"] = ("binned", M, {}, 0, dict(per_row_gamma=SCAN, states_per_lane=npl, long_rows_cut=False, chain_family=5))
    c["scan:M100:chunk37"] = ("binned", 100, {}, 37, dict(per_row_gamma=SCAN, states_per_lane=2, long_rows_cut=False, chain_family=5))
    # eigen-power pieces: NPL = 2, 3, 4
    for M in (65, 150, 256):
        c[f"pieces:M{M}"] = ("unbinned", M, UNCUT, 0,
                             dict(per_row_gamma=PIECES, states_per_lane=(M + 63) // 64, long_rows_cut=False, chain_family=3))
    c["pieces:M65:chunk37"] = ("unbinned", 65, UNCUT, 37, dict(per_row_gamma=PIECES, states_per_lane=2, long_rows_cut=False, chain_family=3))
    # rows cut into pieces of 64 positions (merged_gamma / k_gamma_merge)
    for M, npl in ((100, 2), (300, 8)):
        c[f"cut:M{M}"] = ("short_unbinned", M, {}, 0, dict(per_row_gamma=SCAN, states_per_lane=npl, long_rows_cut=True, chain_family=5))
    # two populations
    c["twopop:M48"] = ("twopop", 48, NO_SCAN, 0, dict(per_row_gamma=EIG, states_per_lane=1, long_rows_cut=False, chain_family=5))
    c["twopop:M130"] = ("twopop", 130, {}, 0, dict(per_row_gamma=SCAN, states_per_lane=3, long_rows_cut=False, chain_family=5))
    return c


CASES = _cases()
# the routes whose reference decodes the last state on some column: one per padded width of each kernel family
LAST_STATE = {"eig_b:M1", "eig_b:M13", "eig_b:M32", "eig_b:M48", "eig_b:M64", "eig_big:M65", "eig_big:M130", "eig_big:M256",
              "scan:M64", "scan:M100", "scan:M150", "scan:M256", "scan:M300", "scan:M520", "pieces:M65", "pieces:M150", "pieces:M256",
              "cut:M100", "cut:M300", "twopop:M48", "twopop:M130"}

_INPUTS = {}


def case_inputs(kind, M):
    """-> (contigs, theta, rho); built once per (kind, size class)."""
    key = (kind, M if kind in ("binned", "unbinned", "short_unbinned") else None)
    if key in _INPUTS:
        return _INPUTS[key]
    if kind == "batches":
        r = (key_batch_contigs(), TH_B, RH_B)
    elif kind == "binned":
        # (the restatement takes 2 M^3 flop per span > 1 row on one core: fewer rows as M grows)
        length = 600_000 if M <= 64 else 200_000 if M <= 256 else 60_000 if M <= 300 else 20_000
        r = (binned_contigs(40 + M, length), TH_B, RH_B)
    elif kind == "unbinned":
        r = (unbinned_contigs(160 if M <= 150 else 110), TH_U, RH_U)
    elif kind == "unstructured":
        r = (binned_contigs(77, 200_000), TH_B, RH_B)
    elif kind == "short_unbinned":
        r = (unbinned_contigs(120 if M <= 256 else 70, spans=(65, 129, 193, 257), cap=300), TH_U, RH_U)
    elif kind == "twopop":
        r = (twopop_contigs(150_000 if M <= 64 else 60_000), None, None)
    else:
        raise AssertionError(kind)
    _INPUTS[key] = r
    return r


def run_case(case, engine_opt):
    kind, M, switches, chunk, want = CASES[case]
    contigs, theta, rho = case_inputs(kind, M)
    for k, v in switches.items():
        engine_opt(k, v)
    if kind == "twopop":
        im = _twopop(M, contigs)
    elif kind == "unstructured":
        im = _unstructured(M, contigs, theta, rho)
    else:
        im = _onepop(M, contigs, theta, rho)
    if chunk:
        im.set_chunking(chunk)
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    got = {k: plan[k] for k in ("per_row_gamma", "states_per_lane", "long_rows_cut", "chain_family")}
    print(f"{case}: plan {got}")
    for k, v in want.items():
        assert plan[k] == v, (case, k, plan[k], v, plan)
    # the statistics plan: the per-row form, and whether it runs beside the statistics (all but the eigen-power pieces, which read
    # the statistics' own products, unless SMCPP_GAMMA_SIDE=0)
    st = im.describe()["statistics"]
    form = {SCAN: SCAN, PIECES: PIECES, EIG: "eigensystem batches" if M <= 64 else "eigensystem rows"}[want["per_row_gamma"]]
    beside = want["per_row_gamma"] != PIECES and switches.get("SMCPP_GAMMA_SIDE") != "0"
    assert (st["per_row_gamma"], st["per_row_gamma_beside"], st["per_row_gamma_stream"]) == \
        (form, beside, "high priority" if beside else "main"), (case, st)
    return im, contigs


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_gamma_route(engine_opt, case):
    """One route of the per-row posterior against the C restatement on every column of every contig.

    Measured on one MI355X (worst over the contigs of a case): per column, the error in units of the row's span is 5e-8 - 1.2e-6
    (bar 2e-5); a column's sum is its span to 1.5e-15 (bar 1e-9); the entries of 1e-3 of the span or more agree to 0.9e-6 - 7.9e-6
    relative (bar 1e-4; worst: rows cut into pieces at M = 100), the float alpha of the reference's algorithm."""
    im, contigs = run_case(case, engine_opt)
    M = im.M
    keys = im.keys
    ep = im.emission_probs
    Etab = np.array([ep[tuple(k)] for k in keys.tolist()])
    pi, T = im.pi, im.transition
    lls, gams = im.logliks(), im.gammas
    assert len(gams) == len(contigs)
    last = False
    for c, ob in enumerate(contigs):
        o = oracle_estep(pi, T, keys, Etab, ob)
        assert abs(lls[c] - o["loglik"]) <= LL_TOL * max(1.0, abs(o["loglik"])), (c, lls[c], o["loglik"])
        # (rows cut into pieces: the caller's row count, the pieces added up)
        assert gams[c].shape == (M, len(ob) + 1)
        check_gamma_columns(gams[c], o["gamma"], ob, arg_dev=im.gamma_argmax(c), label=f"{case} contig {c}")
        last |= bool(np.any(o["gamma"][:, 1:].argmax(axis=0) == M - 1))
    if case in LAST_STATE:
        assert last, f"{case}: the reference never decodes the last state: the input does not test it"


def test_save_npz_product(tmp_path):
    """`smc++ posterior`'s output file (posterior.save_npz): keys, shapes, dtypes, normalised columns, the sites column."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    from smcpp_amd.posterior import posterior, save_npz
    a, s = synth.model_pieces()
    model = PiecewiseModel(a, s, 1e4, "pop1")
    raw = [synth.synth_posterior_contig(200, N, seed=21), synth.synth_posterior_contig(90, N, seed=22)]
    M = 16
    hs, gammas, sites, paths = posterior(model, raw, M, N, TH_U, RH_U)
    names = ["chr1.smc.gz", "chr2.smc.gz"]
    path = tmp_path / "post.npz"
    save_npz(str(path), hs, gammas, sites, names)
    z = np.load(str(path))
    assert sorted(z.files) == sorted(["hidden_states"] + names + [nm + "_sites" for nm in names])
    assert z["hidden_states"].shape == (M + 1,) and z["hidden_states"].dtype == np.float64
    assert z["hidden_states"][0] == 0 and np.isinf(z["hidden_states"][-1]) and np.all(np.diff(z["hidden_states"]) > 0)
    for nm, r, g, p in zip(names, raw, gammas, paths):
        gz, sz = z[nm], z[nm + "_sites"]
        L = len(r) + 1                                       # the missing row posterior() puts in front
        assert gz.shape == (M, L + 1) and gz.dtype == np.float64
        np.testing.assert_allclose(gz.sum(axis=0), 1.0, rtol=1e-12)
        assert np.all(gz >= 0)
        assert np.array_equal(gz, g)
        assert sz.shape == (L,) and np.issubdtype(sz.dtype, np.integer)
        assert sz[0] == 1 and np.array_equal(sz[1:], r[:, 0])
        assert np.array_equal(np.asarray(p), gz.argmax(axis=0))
