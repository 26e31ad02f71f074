"""Every compiled form of the scan chains' position step (smcpp_amd/csrc/chains_ss.hpp) against the dense float64 product.

The step is a pure function: generators of T, a vector x and an emission vector e in, out_f = A_f x and out_b = A_b x out, with
A_f = diag(e) T^T and A_b = T diag(e).  `smcpp_debug_ss_apply_form` runs the production device functions on caller vectors, one
wavefront per vector:

  form 0  ss_fwd_step<NPL> / ss_bwd_step<NPL>, fp64 scans                                  M = 1 .. 64 and the edges of 2 .. 16 states per lane
  form 1  float scans of the stored passes as the engine picks them (two-row form, M <= 32) M = 1 .. 64
  form 2  float scans of the stored passes, full-width form (SMCPP_SS_H32=0)                M = 1 .. 64
  form 3  the all-float step of the light passes and the float halo, ss_*_step_f<NPL>       as form 0
  form 4  the all-float step, two-row form                                                  M = 1 .. 32
  form 5  power jumps (k_ss_jump_tables + ss_jump_load + ss_jump_run), P = 4, 8, 16,        M = 1 .. 64
          one jump (A^P x) and three (A^3P x)

Two transition matrices per state count - the model's own (host preparation of the synthetic model, n = 4) and the generator-built
matrix of tests/test_gpu_ss.py, whose part above the diagonal decays to the mixing constant c0 = 1e-5 / (M + 1) within a few states -
and per call ALL M unit vectors (the output is the operator column by column: every (source lane, register) -> (destination lane,
register) pair) plus the dense set of tests/test_gpu_ss.py (ones, first state, last state, rng ** 8 + 1e-12).  e = 0.2 + 0.8 rng per
vector; the rows of one unit vector and of one dense vector are all ones, so that an error in e cannot hide one in the scan.  (Form 5
takes ONE emission vector per call: the jump key's.)

Bounds.  u = 2^-53 (form 0), U = 2^-24 (float forms); g_j = T[M-1][j] is the constant of column j below the diagonal, d_j = T[j][j].
The factors count operations; none is measured.  Where a bound below differs from "entrywise relative", the operation that accounts
for it is named: the step does not form T[i][j] for j > i as the sum c0 + Phi'(i, j) but as  g_j S + (c0 - g_j) incl_j + Z_j, in which
g_j cancels, and its backward half forms the c0 term from a FLOAT prefix sum of e o x.

  form 0, dense vectors  the bars of tests/test_gpu_ss.py: 1e-11 of the vector's largest entry, 1e-7 per entry.
  form 0, unit vectors   1e-12 relative per entry (at most 6 + NPL fp64 factors), plus
                           forward, j > i:  2^-52 g_j e_j - two roundings at the size of g_j (c0 - g_j when the generators are packed,
                             (c0 - g_j) incl + Z in the step) ahead of the cancellation;
                           backward, r < i: U c0 e_i - inclW is a float prefix sum (lf / lif in ss_bwd_step), one rounding of e_i x_i.
  forms 1 / 2, dense     the bar of tests/test_gpu_ss.py: 2e-8 of the largest entry.
  forms 1 / 2, unit      off the diagonal (8 + 6) U relative: float products of at most 6 + 2 factors.  The diagonal entry is the fp64
                         term (d_i - g_i) x_i plus the float scans' own entry of lane i - the inclusive suffix sum hands
                         (g_i - c0) x_i + c0 x_i (forward) / g_i w_i + c0 w_i (backward) back in float: 1e-12 relative plus
                         3 U (g_i + c0) e_i forward, 4 U (g_i + c0) e_i backward.
                         Form 1 against form 2 at M <= 32: no bit differs on the live states.
  forms 3 / 4            every operation in float, depth <= NPL + 8: factor F = NPL + 16.
                         forward, unit vectors: F U times the sum of the MAGNITUDES of the terms of the entry,
                           e_j (T[i][j] + 2 max(g_j - c0, 0)) for j >= i, e_j T[i][j] below - (c0 - g_j) is negative, so an entry above
                           the diagonal is not a sum of non-negative terms; it is one only below the diagonal.
                         backward (forms Gtot - inclG, a difference) and dense vectors: F U times the largest entry of the reference
                           vector.  Form 4 against form 3 at M <= 32: no bit differs.
  form 5                 16 U per jump, entrywise relative, unit and dense vectors (table entry rounded to float, 64 float products in
                         four accumulators, the diagonal in float); the hook itself returns 3 if a padded state holds anything but 0.0.

Before a bar is trusted the same check is run on the CPU on a plain dense product in the form's number formats (forms 1 / 2: the
off-diagonal part in float32, the diagonal in float64; forms 3 / 4: float32 throughout; form 5: the float64 power rounded to
float32 and applied in float32): it must pass, i.e. no bar is below what the format delivers on these inputs.

Measured on one MI355X (worst over both matrices; "of its bound" = |out - ref| / bound, unit vectors / dense vectors):
  form 0   forward, by states per lane 1, 2, 3, 4, 8, 16: 0.67, 0.54, 0.71, 0.59, 0.57, 0.73 of its bound on unit vectors (worst relative
           error 2.2e-12 .. 3.7e-12: the cancellation of g_j - a plain 1e-12 relative does not hold), <= 0.003 on dense vectors;
           backward: 0.95, 0.94, 0.97, 0.93, 0.98, 0.96 / 0.48, 0.29, 0.35, 0.49, 0.31, 0.23 (worst relative error 4.9e-8 .. 5.7e-8 on
           entries that are c0 to within 1e-3: the float prefix sum - a plain 1e-12 relative does not hold there either).
  form 1   forward 0.55 / 0.15, backward 0.69 / 0.20; worst relative error off the diagonal 3.3e-7 (bar 8.3e-7).
  form 2   the same figures: it equals form 1 in every bit at M <= 32 and IS form 1 above.
  form 3   forward 0.27, 0.22, 0.26, 0.25, 0.27, 0.27 / 0.15, 0.11, 0.11, 0.11, 0.09, 0.07; backward 0.13, 0.11, 0.11, 0.10, 0.10, 0.07 /
           0.16, 0.11, 0.13, 0.11, 0.09, 0.05.  Worst RELATIVE error of a forward entry 1.9e-3 .. 2.9e-3 (an entry ~ c0 behind a g_j of 1e-3
           of the row: F U relative, 1.0e-6 .. 1.9e-6, does not hold above the diagonal), of a backward entry on unit vectors 2.4e-7 .. 6.3e-7.
  form 4   forward 0.22 / 0.15, backward 0.11 / 0.15; equals form 3 in every bit.
  form 5   one jump (P = 4, 8, 16): 0.06 / 0.30 .. 0.42 (a unit vector reads one table entry: one rounding); three jumps: 0.16 .. 0.20 /
           0.12 .. 0.17.
  SMCPP_SS_H32 unset against 0 at M = 16, 17, 31, 32: log-likelihood, xi sums, gamma sums, gamma_0 and every per-row posterior equal in
  every bit (0 < 1.9e-9 .. 7.3e-7, the distance of either from the restatement); against the restatement (M = 33 included) loglik 1.9e-9 .. 4.0e-9, xi sums
  2.6e-7 .. 6.2e-7, gamma sums 3.1e-7 .. 7.3e-7, worst column of its span 5.5e-7 .. 1.0e-6.
The whole file runs in about 7 s, the restatement's E-steps included; no test takes 2 s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
N_DENSE = 8                                  # random dense vectors behind the three special ones
SMALL = list(range(1, 65))
GROUPS = {                                   # states per lane -> state counts (every switch of NPL from both sides, every 16-lane row edge at NPL = 1)
    1: SMALL, 2: [65, 127, 128], 3: [129, 191, 192], 4: [193, 255, 256], 8: [257, 300, 511, 512], 16: [513, 767, 768, 1023, 1024]}
BIG = [65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 511, 512, 513, 767, 768, 1023, 1024]
POWERS = (4, 8, 16)
_T = {}                                      # M -> {"model": T, "generators": T}, built once and shared by every form
LAUNCHED = set()                             # (form, M, power, kind of T) of every hook call that returned


def npl_of(M):
    return 16 if M > 512 else 8 if M > 256 else (M + 63) // 64


def generator_T(M):
    """The matrix of tests/test_gpu_ss.py::test_one_position_other_state_counts (same draws, same formula, vectorised)."""
    rng = np.random.default_rng(M)
    c0 = 1e-5 / (M + 1)
    g = 1e-4 * rng.random(M)
    u = 1e-3 * rng.random(M)
    r = np.cumsum(0.05 + 0.1 * rng.random(M))
    i, j = np.indices((M, M))
    T = np.where(j < i, g[None, :] + c0, c0 + u[:, None] * np.exp(-(r[None, :] - r[:, None])))
    T[i == j] = 0.0
    T[np.arange(M), np.arange(M)] = 1.0 - T.sum(axis=1)
    return T


def matrices(M):
    if M not in _T:
        from smcpp_amd import _engine, synth
        a, s = synth.model_pieces()
        _, Tm, _ = _engine.host_prep_onepop(4, synth.hidden_states(M), 0.5, a, s, synth.THETA, synth.RHO, 1.0,
                                            np.array([[0, 0, 0]], dtype=np.int32))
        _T[M] = {"model": np.ascontiguousarray(Tm), "generators": generator_T(M)}
    return _T[M]


def vectors(M, one_e=False):
    """-> x [M + 3 + N_DENSE][M] (rows 0 .. M-1 the unit vectors), e of the same shape."""
    rng = np.random.default_rng(4000 + M)
    x = np.zeros((M + 3 + N_DENSE, M))
    x[:M] = np.eye(M)
    x[M] = 1.0
    x[M + 1, 0] = 1.0
    x[M + 2, M - 1] = 1.0
    x[M + 3:] = rng.random((N_DENSE, M)) ** 8 + 1e-12
    e = 0.2 + 0.8 * rng.random(x.shape)
    if one_e:
        e[:] = e[0]
    else:
        e[M // 2] = 1.0
        e[M + 3] = 1.0
    return x, e


def apply_form(T, x, e, form, power=0, kind=""):
    from smcpp_amd import _engine
    L = _engine.lib()
    T = np.ascontiguousarray(T, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    of = np.full_like(x, np.nan)
    ob = np.full_like(x, np.nan)
    rc = L.smcpp_debug_ss_apply_form(T.shape[0], _engine.dptr(T), x.shape[0], _engine.dptr(x), _engine.dptr(e), _engine.dptr(of),
                                     _engine.dptr(ob), form, power)
    if rc == 1:
        raise RuntimeError(L.smcpp_last_error().decode())
    if rc == 0:
        LAUNCHED.add((form, T.shape[0], power, kind))
    return rc, of, ob


def reference(T, x, e, power=0):
    if not power:
        return e * (x @ T), (e * x) @ T.T
    Af = e[0][:, None] * T.T
    Ab = T * e[0][None, :]
    return x @ np.linalg.matrix_power(Af, power).T, x @ np.linalg.matrix_power(Ab, power).T


def dot32(x, A):
    """x @ A.T in float32 with PAIRWISE summation (depth log2 M, as the scans'): float32 products, float32 adds, no wider accumulator.
    (A sequential float32 sum of M terms carries up to M roundings, and below the diagonal a column of T is constant, so they all pull
    the same way: 20 U at M = 30 on the all-ones vector.  The bars count the roundings of a sum of depth NPL + 8.)"""
    x = np.asarray(x, dtype=np.float32)
    A = np.asarray(A, dtype=np.float32)
    n = 1 << max(0, (A.shape[1] - 1).bit_length())
    out = np.empty((x.shape[0], A.shape[0]), dtype=np.float32)
    for v0 in range(0, x.shape[0], 16):
        t = np.zeros((min(16, x.shape[0] - v0), A.shape[0], n), dtype=np.float32)
        t[:, :, :A.shape[1]] = x[v0:v0 + 16, None, :] * A[None, :, :]
        while t.shape[2] > 1:
            t = t[:, :, 0::2] + t[:, :, 1::2]
        out[v0:v0 + 16] = t[:, :, 0]
    return out


def plain_float32(form, T, x, e, power=0):
    """The same products by plain dense arithmetic in the number formats of the form (see the module docstring).  The unit vectors
    need no sum: their product is the rounded column itself."""
    f32 = np.float32
    M = T.shape[0]

    def mv(v, A):              # v @ A.T, rows 0 .. M-1 of v being the unit vectors scaled by v[i, i]
        A32 = A.astype(f32)
        return np.vstack([(np.diag(v)[:M].astype(f32)[:, None] * A32.T).astype(f32), dot32(v[M:], A32)])
    if form in (1, 2):
        d = np.diag(T).copy()
        off = T - np.diag(d)
        w = e * x
        return e * (d * x + mv(x, off.T).astype(np.float64)), d * w + mv(w, off).astype(np.float64)
    if form in (3, 4):
        e32 = e.astype(f32)
        return (e32 * mv(x, T.T)).astype(np.float64), mv((e32 * x.astype(f32)), T).astype(np.float64)
    P = next(q for q in POWERS if power in (q, 3 * q))
    outs = []
    for A in (e[0][:, None] * T.T, T * e[0][None, :]):
        AP = np.linalg.matrix_power(A, P)
        d32 = np.diag(AP).astype(f32)
        off = (AP - np.diag(np.diag(AP))).astype(f32)
        y = x.astype(f32)
        for _ in range(power // P):
            y = (dot32(y, off) + d32 * y).astype(f32)
        outs.append(y.astype(np.float64))
    return outs


def bounds(form, T, x, e, ref_f, ref_b, power=0):
    """-> the absolute bound of every output entry, forward and backward (module docstring); rows 0 .. M-1 are the unit vectors."""
    M = T.shape[0]
    npl = npl_of(M)
    c0 = 1e-5 / (M + 1)
    g = T[M - 1].copy()
    g[M - 1] = 0.0
    ii = np.arange(M)
    above = ii[None, :] > ii[:, None]            # [i (the unit vector)][j (the output entry)]: j > i
    ediag = e[ii, ii]                            # e_i of unit vector i
    mx_f = np.abs(ref_f).max(axis=1, keepdims=True)
    mx_b = np.abs(ref_b).max(axis=1, keepdims=True)
    if form == 0:
        bf = np.minimum(1e-11 * mx_f, 1e-7 * np.abs(ref_f)) * np.ones_like(ref_f)
        bb = np.minimum(1e-11 * mx_b, 1e-7 * np.abs(ref_b)) * np.ones_like(ref_b)
        bf[:M] = 1e-12 * ref_f[:M] + np.where(above, 2.0 ** -52 * g[None, :] * e[:M], 0.0)
        bb[:M] = 1e-12 * ref_b[:M] + np.where(above.T, U32 * c0 * ediag[:, None], 0.0)
    elif form in (1, 2):
        bf = 2e-8 * mx_f * np.ones_like(ref_f)
        bb = 2e-8 * mx_b * np.ones_like(ref_b)
        bf[:M] = 14 * U32 * ref_f[:M]
        bb[:M] = 14 * U32 * ref_b[:M]
        bf[ii, ii] = 1e-12 * ref_f[ii, ii] + 3 * U32 * (g + c0) * ediag
        bb[ii, ii] = 1e-12 * ref_b[ii, ii] + 4 * U32 * (g + c0) * ediag
    elif form in (3, 4):
        F = (npl + 16) * U32
        bf = F * mx_f * np.ones_like(ref_f)
        bb = F * mx_b * np.ones_like(ref_b)
        mag = T + np.where(ii[None, :] >= ii[:, None], 2.0 * np.maximum(g - c0, 0.0)[None, :], 0.0)
        bf[:M] = F * e[:M] * mag
    else:
        nj = power // next(q for q in POWERS if power in (q, 3 * q))
        bf = 16 * U32 * nj * ref_f
        bb = 16 * U32 * nj * ref_b
    return bf, bb


def worst_ratio(out, ref, bound, M):
    """-> (unit vectors, dense vectors): the largest |out - ref| / bound."""
    assert np.all(np.isfinite(out))
    assert np.all(ref > 0.0) and np.all(bound > 0.0)
    r = np.abs(out - ref) / bound
    return float(r[:M].max()), float(r[M:].max())


def worst_relative(out, ref, M):
    r = np.abs(out - ref) / ref
    return float(r[:M].max()), float(r[M:].max())


def check_one(form, M, kind, power=0):
    """One hook call: (form, M, kind of T[, power]) -> dict of worst ratios; asserts the form's bounds and the format check."""
    T = matrices(M)[kind]
    x, e = vectors(M, one_e=form == 5)
    ref_f, ref_b = reference(T, x, e, power)
    bf, bb = bounds(form, T, x, e, ref_f, ref_b, power)
    if form != 0:
        pf, pb = plain_float32(form, T, x, e, power)
        for name, o, r, b in (("forward", pf, ref_f, bf), ("backward", pb, ref_b, bb)):
            wu, wd = worst_ratio(o, r, b, M)
            assert wu <= 1.0 and wd <= 1.0, f"form {form}, M = {M}, {kind} T, {name}: the bar is below what a plain product in the form's " \
                                            f"formats gives ({wu:.2f} / {wd:.2f} of it)"
    rc, of, ob = apply_form(T, x, e, form, power, kind)
    assert rc == 0, (form, M, kind, power, rc)
    res = {}
    for name, o, r, b in (("forward", of, ref_f, bf), ("backward", ob, ref_b, bb)):
        wu, wd = worst_ratio(o, r, b, M)
        ru, rd = worst_relative(o, r, M)
        res[name] = (wu, wd, ru, rd)
        if wu > 1.0 or wd > 1.0:
            d = np.abs(o - r) / b
            v, j = np.unravel_index(int(d.argmax()), d.shape)
            raise AssertionError(f"form {form}, power {power}, M = {M}, {kind} T, {name}: vector {v} ({'unit' if v < M else 'dense'}), entry {j}: "
                                 f"{o[v, j]!r} against {r[v, j]!r}, {d[v, j]:.3g} of its bound")
    return res, of, ob


def run_group(form, Ms, power=0):
    """Every M of the group on both matrices; prints the worst of each measure; -> number of hook calls that launched."""
    n0 = len(LAUNCHED)
    worst = {}
    for M in Ms:
        for kind in ("model", "generators"):
            res, _, _ = check_one(form, M, kind, power)
            for name, (wu, wd, ru, rd) in res.items():
                w = worst.setdefault(name, [0.0, 0.0, 0.0, 0.0, 0, 0])
                if wu > w[0]:
                    w[0], w[4] = wu, M
                if wd > w[1]:
                    w[1], w[5] = wd, M
                w[2] = max(w[2], ru)
                w[3] = max(w[3], rd)
    for name, w in worst.items():
        print(f"form {form}{f', power {power}' if power else ''}, M = {Ms[0]} .. {Ms[-1]} ({npl_of(Ms[0])} per lane), {name}: worst of its bound "
              f"{w[0]:.3f} (unit vectors, M = {w[4]}) / {w[1]:.3f} (dense, M = {w[5]}); worst relative error {w[2]:.2e} / {w[3]:.2e}")
    return len(LAUNCHED) - n0


def test_cases_cover_the_table():
    assert sorted(M for Ms in GROUPS.values() for M in Ms) == SMALL + BIG
    assert all(npl_of(M) == npl for npl, Ms in GROUPS.items() for M in Ms)


def test_model_matrices_have_the_structure():
    """The hook extracts the generators from the dense T and returns 2 where it finds no structure: it must find it in the model's own T
    at every state count of this file (a 2 here would have to be matched by a manager that leaves chain family 5)."""
    for M in SMALL + BIG:
        T = matrices(M)["model"]
        rc, _, _ = apply_form(T, np.ones((1, M)), np.ones((1, M)), 0, kind="probe")
        assert rc == 0, (M, rc)


@pytest.mark.parametrize("npl", sorted(GROUPS))
@pytest.mark.parametrize("form", [0, 3])
def test_every_state_count_fp64_and_light_step(form, npl):
    assert run_group(form, GROUPS[npl]) == 2 * len(GROUPS[npl])


@pytest.mark.parametrize("form", [1, 2])
def test_float_scans_of_the_stored_passes(form):
    assert run_group(form, SMALL) == 2 * 64


def test_two_row_light_step():
    assert run_group(4, SMALL[:32]) == 2 * 32


@pytest.mark.parametrize("pair", [(1, 2), (4, 3)])
def test_two_row_form_equals_full_width_form_bit_for_bit(pair):
    """M <= 32: the two-row form only skips a level that moves zeros and takes the total from another lane."""
    n = 0
    for M in SMALL[:32]:
        for kind in ("model", "generators"):
            T = matrices(M)[kind]
            x, e = vectors(M)
            rc2, f2, b2 = apply_form(T, x, e, pair[0], kind=kind)
            rcw, fw, bw = apply_form(T, x, e, pair[1], kind=kind)
            assert rc2 == 0 == rcw
            assert np.array_equal(f2, fw), (pair, M, kind, "forward", np.argwhere(f2 != fw)[:4].tolist())
            assert np.array_equal(b2, bw), (pair, M, kind, "backward", np.argwhere(b2 != bw)[:4].tolist())
            n += 1
    assert n == 64


@pytest.mark.parametrize("jumps", [1, 3])
@pytest.mark.parametrize("P", POWERS)
def test_power_jumps(P, jumps):
    assert run_group(5, SMALL, power=P * jumps) == 2 * 64


@pytest.mark.parametrize("args", [(1, 65, 0), (2, 65, 0), (4, 33, 0), (5, 65, 8), (5, 64, 0), (5, 64, 5), (5, 64, 32), (0, 64, 8), (3, 1025, 0),
                                  (6, 16, 0), (-1, 16, 0), (0, 0, 0)])
def test_forms_the_engine_never_compiles_are_refused(args):
    """(form, M, power): refused with a message before anything is launched (the outputs stay untouched)."""
    from smcpp_amd import _engine
    form, M, power = args
    L = _engine.lib()
    n = max(M, 1)
    T, x, of, ob = generator_T(n), np.ones((1, n)), np.full((1, n), -7.0), np.full((1, n), -7.0)
    rc = L.smcpp_debug_ss_apply_form(M, _engine.dptr(T), 1, _engine.dptr(x), _engine.dptr(x), _engine.dptr(of), _engine.dptr(ob), form, power)
    assert rc == 1 and len(L.smcpp_last_error().decode()) > 10, (args, rc)
    assert np.all(of == -7.0) and np.all(ob == -7.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# SMCPP_SS_H32 end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _estep(M, h32, save_gamma, engine_opt):
    from test_gpu_gamma import RH_B, TH_B, _onepop
    from test_gpu_ss_jumps import CHUNK, _contig
    contig, _ = _contig(False)
    engine_opt("SMCPP_SS_H32", h32)
    im = _onepop(M, [contig], TH_B, RH_B)
    im.set_chunking(CHUNK)
    im.save_gamma = save_gamma
    im.E_step()
    assert im.chain_mode() == 5
    keys = im.keys
    ep = im.emission_probs
    out = dict(ll=im.loglik(), xis=im.xisums[0].copy(), gs={k: v.copy() for k, v in im.gamma_sums[0].items()}, g0=im.gammas[0][:, 0].copy(),
               gam=im.gammas[0].copy() if save_gamma else None, plan=im.describe()["plan"], pi=np.array(im.pi), T=np.array(im.transition),
               keys=np.array(keys), E=np.array([ep[tuple(k)] for k in keys.tolist()]), contig=contig)
    engine_opt("SMCPP_SS_H32", None)
    return out


@pytest.mark.parametrize("M", [16, 17, 31, 32, 33])
def test_two_row_switch_end_to_end(engine_opt, M):
    """SMCPP_SS_H32 unset and 0, with and without save_gamma, on the contig of tests/test_gpu_ss_jumps.py (4096 rows, 16 chunks of 256:
    light passes, the stored pass and a re-run): each against the C restatement at the bars of tests/test_gpu_parity.py, the plan's
    "two_row_scans" as expected (M = 33: false either way), and on against off below off against the restatement."""
    from test_gpu_parity import LL_TOL, STAT_TOL, check_gamma_columns, oracle_estep
    from test_gpu_ss_jumps import CHUNK, ROWS, _diff
    runs = {}
    for h32 in (None, "0"):
        for sg in (False, True):
            r = runs[(h32, sg)] = _estep(M, h32, sg, engine_opt)
            plan = r["plan"]
            assert plan["two_row_scans"] is (h32 is None and M <= 32), (M, h32, plan)
            assert plan["states_per_lane"] == 1 and plan["chunks_forward"] == ROWS // CHUNK == plan["chunks_backward"], plan
            # light passes, the stored pass and at least one re-run pass behind it
            lf, lb = plan["light_passes_forward"], plan["light_passes_backward"]
            assert lf > 0 and lb > 0 and plan["passes_launched"] >= max(lf, lb) + 2, plan
            o = oracle_estep(r["pi"], r["T"], r["keys"], r["E"], r["contig"], save_gamma=True)
            ref = dict(ll=o["loglik"], xis=o["xisum"], gs=o["gamma_sums"], g0=o["gamma"][:, 0])
            assert sorted(r["gs"]) == sorted(ref["gs"])
            r["d_ref"] = d = _diff(r, ref)
            print(f"M = {M}, SMCPP_SS_H32 {'unset' if h32 is None else h32}, save_gamma {sg}: two_row_scans {plan['two_row_scans']}; against the "
                  f"restatement: loglik {d[0]:.2e}, xi sums {d[1]:.2e}, gamma sums {d[2]:.2e}, gamma_0 {d[3]:.2e}")
            assert d[0] <= LL_TOL and d[1] <= STAT_TOL and d[2] <= STAT_TOL and d[3] <= STAT_TOL
            if sg:
                check_gamma_columns(r["gam"], o["gamma"], r["contig"], label=f"M = {M}, SMCPP_SS_H32 {h32}")
    for sg in (False, True):
        on, off = runs[(None, sg)], runs[("0", sg)]
        d_on = _diff(on, off)
        print(f"M = {M}, save_gamma {sg}: on against off: loglik {d_on[0]:.2e}, xi sums {d_on[1]:.2e}, gamma sums {d_on[2]:.2e}, gamma_0 {d_on[3]:.2e}")
        for name, a, b in zip(("loglik", "xi sums", "gamma sums", "gamma_0"), d_on, off["d_ref"]):
            assert a < b, (M, sg, name, a, b)
        if sg:
            dg = float(np.max(np.abs(on["gam"] - off["gam"])))
            print(f"M = {M}: per-row posteriors, on against off: largest difference {dg:.2e}")
