"""The posterior path sampler - `posterior_sample_rows`, `posterior_sample_positions` (smcpp_amd/csrc/posterior_paths_dev.hpp) and
`posterior.posterior_products(paths=K)`.

Managers come from `test_gpu_gamma.run_case` (scan steps at 1, 2, 8 and 16 states per lane, a forced chunking, rows cut into pieces,
two populations at three states per lane) and from the un-binned case at M = 64 of tests/test_gpu_posterior_transitions.py (rows of
64 / 65 / 128 / 129 / 10^5 positions: the block seams and the checkpointed walk; contigs of one and of two rows).

The truth is tests/pathref.py.  A sampled path cannot be compared with the oracle's own path state by state (a CDF off by 1e-8 moves
a draw whose u lies that close to an edge, and every draw behind it follows), so EVERY draw of every path is held to the oracle's
float64 CDF conditioned on the path's own next state: the distance by which its u lies outside [C_{x-1}, C_x) / C_{M-1} is at most
GAMMA_TOL = 2e-5, the project's bar for the per-row posterior, which is built from the same stored float vectors.  No draw is exempt.
The per-row product is the per-position product reduced by `pathref.rows_from_positions`, integer for integer; windows and
selections are slices; repetition, call order, a split of the paths into calls, SMCPP_PATH_BATCH, a repeated E-step and poisoned
allocations give the same bits.  State frequencies of 4096 paths are held to Bernstein's inequality at t = 30 around the float64
marginals (failure probability 2e-13 per cell for an exact sampler) plus GAMMA_TOL; the oracle's sampler is held to the same bound.

Measured on one MI355X (worst distance over all draws of all paths of all contigs of a case / draws with a distance above 0 / draws):

  case                 worst distance   draws off   draws
  scan:M64             0                0           49 512
  scan:M100            0                0           17 592
  scan:M300            0                0           6 440
  scan:M520            0                0           3 360
  scan:M100:chunk37    0                0           17 592
  cut:M100             0                0           162 584
  twopop:M130          0                0           5 400
  unbinned:M64         0                0           1 345 588

No u of these 1.6e6 draws lay between the device's CDF and the oracle's: with the 1e-8 .. 1e-6 by which the per-row posteriors built
from the same vectors miss theirs, about one draw in 1e7 .. 1e5 is expected to (two edges per draw).  State frequencies of 4096 paths
at 739 positions: worst deviation 0.49 of the bound, the oracle's sampler 0.49 as well; mean up / down totals of 1024 paths 0.19 /
0.22 standard errors from the expected counts; the states at the row ends 0.43 of the bound.

The launch shape.  The kernel is persistent: wavefront gw owns one slice of scratch (the parked vectors of a block of 64 positions,
the fp64 checkpoints of a long row) and takes batches gw, gw + nwaves, ..; the host gives it the fewest of the batches, 4096 slots
(1024 from 8 states per lane) and the wavefronts whose scratch fits 1 GiB.  The cases below assert from `describe()` (`path_batch`,
`path_batches`, `path_waves`, the plan) that they reach the branch they are named for, and hold every bit-equality between a call
in which wavefronts take a second batch and calls of at most 64 paths, in which none does:

  case                                      launch (batches x paths on wavefronts)   worst distance   draws off   draws held
  long rows M = 65 / 150 / 256 (4 paths;    4 x 1 on 4; rows of 16 blocks at         0                0           157 588 each
    SMCPP_SPLIT_SPANS=0)                      2 / 3 / 4 states per lane
  scan:M300, 1030 paths, batch 1            1030 x 1 on 1024 (8 states per lane)     0                0           19 320
    the same without the switch             515 x 2 on 515                           (the same bits)
  freq:M64, 4100 paths, batch 1             4100 x 1 on 4096                         0                0           17 736
  scratch cap: M = 256, a row of 10^5       340 x 1 on 328 (3 264 512 bytes of       0                0           1 400 028
    positions, 340 paths, default switches    scratch per wavefront)
  scan:M64 / cut:M100, 130 paths, batch 64  3 x (64, 64, 2) on 3                     0                0           49 512 / 162 584
  cut:M100 / long rows M = 65, 8 paths,     2 x (7, 1) on 2: windows and selections  (slices of the full results of batch 1)
    batch 7

(draws held: those of the paths handed to the oracle - paths 0 .. 7 and the last 16, which include every path of a second batch;
paths 326 .. 339; paths 60 .. 67 across the seam of two full batches.)  Wall time on one MI355X: every case below 1.5 s but the
scratch cap: its call for the positions of the 340 paths takes 0.16 s (two walks of 10^5 positions behind each other on 12
wavefronts, 136 MB copied to the host), the call for the per-row product 0.15 s, the six calls of 64 paths about as much each;
the test takes 4.5 s, most of it the oracle's 10^5 positions at 256 states.
"""
import time

import numpy as np
import pytest

import pathref
import test_gpu_gamma as tg
import test_gpu_posterior_transitions as tpt
import transref
from test_gpu_parity import GAMMA_TOL
from test_gpu_posterior_products import _selections

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
CASES = ["scan:M64", "scan:M100", "scan:M300", "scan:M520", "scan:M100:chunk37", "cut:M100", "twopop:M130", "unbinned:M64"]
NAMES = ("state", "up", "down")


def manager(case, engine_opt):
    return tpt.manager(case, engine_opt) if case.startswith("unbinned") else tg.run_case(case, engine_opt)


def n_paths(case):
    return 4 if case.startswith("unbinned") else 8


def hmm(im):
    return im.pi, im.transition, im.keys, transref.emission_table(im)


def rows(im, c, *a, **kw):
    r = im.posterior_sample_rows(c, *a, **kw)
    assert sorted(r) == ["down", "state", "up"]
    assert all(r[k].dtype == np.int32 for k in NAMES)
    return np.stack([r[k] for k in NAMES])


def products(im, c, K=8, seed=SEED):
    return {"rows": rows(im, c, K, seed), "pos": im.posterior_sample_positions(c, K, seed)}


def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.int32 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def position_windows(spans):
    """Windows of positions over 0 .. N: inside one block of a row, across a block seam (the row with the most positions, if it
    has more than 64), across a row seam, [0, 1), [N, N + 1)."""
    spans = np.asarray(spans, dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(spans)])
    N = int(P[-1])
    l = int(np.argmax(spans))
    r0 = int(P[l])                                                       # the row's positions are r0 + 1 .. r0 + span
    want = [(r0 + 2, r0 + 10), (r0 + 60, r0 + 70), (int(P[len(P) // 2]) - 1, int(P[len(P) // 2]) + 3), (0, 1), (N, N + 1),
            (r0 + 64, r0 + 66), (max(N - 70, 0), N + 1)]
    out = []
    for a, b in want:
        a, b = max(a, 0), min(b, N + 1)
        if a < b and (a, b) not in out:
            out.append((a, b))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# every draw, the per-row product, selections and windows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_draw_against_the_oracle(engine_opt, case):
    """All positions of 8 (un-binned: 4) paths of every contig: every state in 0 .. M - 1, every draw within GAMMA_TOL of the oracle's
    CDF conditioned on the path's own next state."""
    im, contigs = manager(case, engine_opt)
    assert any(len(ob) == 1 for ob in contigs) and any(len(ob) == 2 for ob in contigs)
    K, M = n_paths(case), im.M
    model = hmm(im)
    worst, off, draws = 0.0, 0, 0
    for c, ob in enumerate(contigs):
        N = int(ob[:, 0].sum())
        pos = im.posterior_sample_positions(c, K, SEED)
        assert pos.shape == (K, N + 1) and pos.dtype == np.int32
        assert pos.min() >= 0 and pos.max() < M, (case, c, pos.min(), pos.max())
        m = pathref.draw_margins(*model, ob, SEED, c, 0, pos)
        assert np.all(np.isfinite(m))
        print(f"{case} contig {c}: {N + 1} positions, worst distance {m.max():.2e}, {int((m > 0).sum())} of {m.size} draws off, "
              f"{int((np.diff(pos, axis=1) != 0).sum())} changes in {K} paths")
        worst, off, draws = max(worst, float(m.max())), off + int((m > 0).sum()), draws + m.size
        bad = np.argwhere(m > GAMMA_TOL)
        assert len(bad) == 0, f"{case} contig {c}: {len(bad)} draws further than {GAMMA_TOL} from the oracle's CDF, e.g. (path, " \
                              f"position) {bad[:8].tolist()}: {m[tuple(bad[:8].T)]}"
    print(f"{case}: WORST distance {worst:.2e}, {off} draws off of {draws}")


@pytest.mark.parametrize("case", CASES)
def test_rows_product_selections_and_windows(engine_opt, case):
    """posterior_sample_rows = rows_from_positions of the device's own positions; column 0 is (x_0, 0, 0); selections and position
    windows are slices of the full results."""
    im, contigs = manager(case, engine_opt)
    K = n_paths(case)
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        spans, L = ob[:, 0], len(ob)
        N = int(spans.sum())
        pos = im.posterior_sample_positions(c, K, SEED)
        v = rows(im, c, K, SEED)
        assert v.shape == (3, K, L + 1), (label, v.shape)
        want = np.stack(pathref.rows_from_positions(pos, spans))
        assert np.array_equal(v, want), (label, np.argwhere(v != want)[:8].tolist())
        assert np.array_equal(v[0, :, 0], pos[:, 0]) and np.all(v[1:, :, 0] == 0), label
        assert np.all(v[1] + v[2] <= np.concatenate([[0], spans])[None, :]), label
        for start, stop, step in _selections(L):
            got = rows(im, c, K, SEED, 0, start, stop, step)
            assert np.array_equal(got, v[:, :, slice(start, stop, step)]), (label, start, stop, step)
        for p0, p1 in position_windows(spans):
            got = im.posterior_sample_positions(c, K, SEED, 0, p0, p1)
            assert got.shape == (K, p1 - p0) and np.array_equal(got, pos[:, p0:p1]), (label, p0, p1, N)


# ---------------------------------------------------------------------------------------------------------------------------------
# the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scan:M64", "cut:M100"])
def test_same_bits(engine_opt, case):
    """Repetition, call order against the other posterior products, [0, 8) against [0, 3) + [3, 8), SMCPP_PATH_BATCH = 1 / 7 /
    default, a second E-step with the same parameters, poisoned allocations: the same bits.  Another seed: other paths."""
    engine_opt("SMCPP_PATH_BATCH", None)
    engine_opt("SMCPP_DEBUG_POISON", None)
    im, contigs = manager(case, engine_opt)
    nc = len(contigs)
    first = [products(im, c) for c in range(nc)]
    assert im.describe()["path_batch"] == 1
    for c in range(nc):
        same_bits(products(im, c), first[c])
    for c in reversed(range(nc)):
        im.posterior_transitions(c)
        pos = im.posterior_sample_positions(c, 8, SEED)                      # (positions before rows, contigs descending)
        im.posterior_windows(c, 100)
        im.posterior_summary(nc - 1 - c)
        assert np.array_equal(pos, first[c]["pos"])
        assert np.array_equal(rows(im, c, 8, SEED), first[c]["rows"])
    for c in range(nc):
        a, b = products(im, c, 3), {"rows": rows(im, c, 5, SEED, 3), "pos": im.posterior_sample_positions(c, 5, SEED, 3)}
        assert np.array_equal(np.concatenate([a["rows"], b["rows"]], axis=1), first[c]["rows"])
        assert np.array_equal(np.concatenate([a["pos"], b["pos"]], axis=0), first[c]["pos"])
        assert np.array_equal(im.posterior_sample_positions(c, 1, SEED, 7), first[c]["pos"][7:])
    for batch in ("1", "7", "64", None):
        engine_opt("SMCPP_PATH_BATCH", batch)
        for c in range(nc):
            same_bits(products(im, c), first[c])
        assert im.describe()["path_batch"] == (int(batch) if batch else 1)
    other = products(im, 0, seed=SEED + 1)
    assert not np.array_equal(other["pos"], first[0]["pos"]) and not np.array_equal(other["rows"], first[0]["rows"])
    assert not np.array_equal(im.posterior_sample_positions(0, 8, SEED ^ (1 << 40)), first[0]["pos"])     # (the seed's high word)
    im.E_step()
    for c in (1, 0) + tuple(range(2, nc)):
        same_bits(products(im, c), first[c])
    del im
    engine_opt("SMCPP_DEBUG_POISON", "255")
    engine_opt("SMCPP_PATH_BATCH", "7")
    im, contigs = manager(case, engine_opt)
    poisoned = [products(im, c) for c in range(nc)]
    del im
    engine_opt("SMCPP_DEBUG_POISON", None)
    for a, b in zip(first, poisoned):
        same_bits(b, a)


def test_identical_contigs_get_different_paths(engine_opt):
    """Two contigs with the same rows in one manager: the same posterior, other paths - the counter carries the contig."""
    ob = tg.binned_contigs(9, 100_000)[0]
    im = tg._onepop(64, [ob, ob.copy()], tg.TH_B, tg.RH_B)
    im.save_gamma = True
    im.E_step()
    g = im.gammas
    assert np.array_equal(g[0], g[1])
    a, b = products(im, 0), products(im, 1)
    assert not np.array_equal(a["pos"], b["pos"]) and not np.array_equal(a["rows"], b["rows"])
    model = hmm(im)
    for c, pr in enumerate((a, b)):
        assert pathref.draw_margins(*model, ob, SEED, c, 0, pr["pos"]).max() <= GAMMA_TOL
    assert pathref.draw_margins(*model, ob, SEED, 0, 0, b["pos"]).max() > GAMMA_TOL      # (contig 1's paths are not contig 0's)


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch shape: multi-block rows beyond one state per lane, a wavefront's second batch, full batches, windows under batching
# ---------------------------------------------------------------------------------------------------------------------------------
_LONG = {}


def launch(im, label):
    """(paths per batch, batches, wavefronts) of the last path call, printed."""
    d = im.describe()
    got = d["path_batch"], d["path_batches"], d["path_waves"]
    print(f"{label}: launch {got[1]} batches of {got[0]} paths on {got[2]} wavefronts")
    return got


def long_rows_manager(M, engine_opt):
    """Un-cut un-binned rows of 64 / 65 / 128 / 129 / 1000 positions (16 blocks, 15 checkpoints, a ragged last block) at
    2 .. 4 states per lane (SMCPP_SPLIT_SPANS=0); contigs of 160, 132, 1 and 2 rows."""
    if "c" not in _LONG:
        _LONG["c"] = tg.unbinned_contigs(120, spans=(64, 65, 128, 129, 1000), cap=1000)
    contigs = _LONG["c"]
    assert [len(ob) for ob in contigs] == [160, 132, 1, 2]
    assert [int(ob[:, 0].sum()) for ob in contigs] == [21_666, 16_725, 1, 1001]
    assert all(int(ob[:, 0].max()) == 1000 for ob in (contigs[0], contigs[1], contigs[3]))
    engine_opt("SMCPP_SPLIT_SPANS", "0")
    im = tg._onepop(M, contigs, tg.TH_U, tg.RH_U)
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    print(f"long rows, M = {M}: plan { {k: plan[k] for k in ('per_row_gamma', 'states_per_lane', 'long_rows_cut', 'chain_family')} }")
    assert plan["states_per_lane"] == (M + 63) // 64 and not plan["long_rows_cut"], plan
    return im, contigs


def in_calls(im, c, K, size=64):
    """Paths 0 .. K - 1 of both products fetched in calls of at most `size` paths, none of which gives a wavefront a second batch."""
    pos, rws = [], []
    for k0 in range(0, K, size):
        n = min(size, K - k0)
        pos.append(im.posterior_sample_positions(c, n, SEED, k0))
        d = im.describe()
        assert d["path_batches"] <= d["path_waves"], d
        rws.append(rows(im, c, n, SEED, k0))
        d = im.describe()
        assert d["path_batches"] <= d["path_waves"], d
    return {"rows": np.concatenate(rws, axis=1), "pos": np.concatenate(pos, axis=0)}


def check_margins(model, ob, c, k0, pos, label):
    """Every draw of the given paths (path k0 + i in line i) within GAMMA_TOL of the oracle's CDF; -> (worst, off, draws)."""
    m = pathref.draw_margins(*model, ob, SEED, c, k0, pos)
    assert np.all(np.isfinite(m))
    print(f"{label}: paths {k0} .. {k0 + len(pos) - 1}, worst distance {m.max():.2e}, {int((m > 0).sum())} of {m.size} draws off")
    bad = np.argwhere(m > GAMMA_TOL)
    assert len(bad) == 0, f"{label}: {len(bad)} draws further than {GAMMA_TOL} from the oracle's CDF, e.g. (path - {k0}, position) " \
                          f"{bad[:8].tolist()}: {m[tuple(bad[:8].T)]}"
    return float(m.max()), int((m > 0).sum()), m.size


@pytest.mark.parametrize("M", [65, 150, 256])
def test_multi_block_rows_beyond_one_state_per_lane(engine_opt, M):
    """Rows of up to 16 blocks at 2, 3 and 4 states per lane (the checkpoints ckpt[(b - 1) MS + lane NPL + k], the ragged last
    block): every draw of 4 paths of every contig against the oracle, the per-row product, the position windows."""
    im, contigs = long_rows_manager(M, engine_opt)
    model = hmm(im)
    K = 4
    worst, off, draws = 0.0, 0, 0
    for c, ob in enumerate(contigs):
        label = f"long rows M = {M} contig {c}"
        spans = ob[:, 0]
        N = int(spans.sum())
        pos = im.posterior_sample_positions(c, K, SEED)
        assert launch(im, label) == (1, K, K)
        assert pos.shape == (K, N + 1) and pos.dtype == np.int32
        assert pos.min() >= 0 and pos.max() < M, (label, pos.min(), pos.max())
        w = check_margins(model, ob, c, 0, pos, label)
        worst, off, draws = max(worst, w[0]), off + w[1], draws + w[2]
        v = rows(im, c, K, SEED)
        want = np.stack(pathref.rows_from_positions(pos, spans))
        assert v.shape == (3, K, len(ob) + 1) and np.array_equal(v, want), (label, np.argwhere(v != want)[:8].tolist())
        for p0, p1 in position_windows(spans):
            got = im.posterior_sample_positions(c, K, SEED, 0, p0, p1)
            assert got.shape == (K, p1 - p0) and np.array_equal(got, pos[:, p0:p1]), (label, p0, p1, N)
    print(f"long rows M = {M}: WORST distance {worst:.2e}, {off} draws off of {draws}")


@pytest.mark.parametrize("case", ["scan:M300", "freq:M64"])
def test_second_batch_by_slots(engine_opt, freq, case):
    """More batches of one path than wavefront slots (1030 on 1024 at 8 states per lane, 4100 on 4096 at one): the wavefronts that
    take a second batch start it from a fresh state on scratch the first has used.  Both products have the bits of the same
    paths fetched in calls of 64 (which never stride); every draw of paths 0 .. 7 and of the last 16 - every path of a second
    batch among them - against the oracle.  M = 300 without the switch: batches of 2 paths, the same bits."""
    if case == "freq:M64":
        im, contigs, K, slots, npl = freq["im"], [freq["ob"]], 4100, 4096, 1
    else:
        (im, contigs), K, slots, npl = tg.run_case(case, engine_opt), 1030, 1024, 8
        assert [int(ob[:, 0].sum()) for ob in contigs] == [736, 1, 65]
    assert im.describe()["plan"]["states_per_lane"] == npl
    model = hmm(im)
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        engine_opt("SMCPP_PATH_BATCH", "1")
        pos = im.posterior_sample_positions(c, K, SEED)
        shape = launch(im, label + " positions")
        assert shape == (1, K, slots) and shape[1] > shape[2], shape
        v = rows(im, c, K, SEED)
        shape = launch(im, label + " rows")
        assert shape == (1, K, slots) and shape[1] > shape[2], shape
        same_bits({"rows": v, "pos": pos}, in_calls(im, c, K))
        assert pos.min() >= 0 and pos.max() < im.M
        check_margins(model, ob, c, 0, pos[:8], label)
        check_margins(model, ob, c, K - 16, pos[K - 16:], label)
        assert np.array_equal(v, np.stack(pathref.rows_from_positions(pos, ob[:, 0]))), label
        if npl == 8:
            # the host's own choice above one path per wavefront
            engine_opt("SMCPP_PATH_BATCH", None)
            two = {"pos": im.posterior_sample_positions(c, K, SEED)}
            assert launch(im, label + " default batching") == (2, K // 2, K // 2)
            two["rows"] = rows(im, c, K, SEED)
            assert launch(im, label + " default batching") == (2, K // 2, K // 2)
            same_bits(two, {"rows": v, "pos": pos})


def test_second_batch_by_the_scratch_cap(engine_opt):
    """Default switches, M = 256, an un-cut row of 10^5 positions: 64 256 4 + 1562 256 8 = 3 264 512 bytes of scratch per wavefront,
    328 wavefronts in 1 GiB, 340 paths of a batch each - 12 wavefronts walk the row a second time over the checkpoints and parked
    vectors of their first path.  The bits of calls of 64 paths; every draw of paths 326 .. 339 against the oracle."""
    engine_opt("SMCPP_PATH_BATCH", None)
    engine_opt("SMCPP_SPLIT_SPANS", None)
    contigs, theta, rho = tg.case_inputs("unbinned", 256)
    im = tg._onepop(256, contigs, theta, rho)
    im.save_gamma = True
    im.E_step()
    plan = im.describe()["plan"]
    assert plan["states_per_lane"] == 4 and not plan["long_rows_cut"], plan
    c, K = 3, 340
    ob = contigs[c]
    assert ob[:, 0].tolist() == [100_000, 1]
    waves = (1 << 30) // (64 * 256 * 4 + 1562 * 256 * 8)
    assert waves == 328
    t0 = time.perf_counter()
    pos = im.posterior_sample_positions(c, K, SEED)
    t1 = time.perf_counter()
    shape = launch(im, f"scratch cap, positions ({t1 - t0:.3f} s)")
    assert shape == (1, K, waves) and shape[1] > shape[2], shape
    assert pos.shape == (K, 100_002) and pos.min() >= 0 and pos.max() < 256
    t0 = time.perf_counter()
    v = rows(im, c, K, SEED)
    t1 = time.perf_counter()
    shape = launch(im, f"scratch cap, rows ({t1 - t0:.3f} s)")
    assert shape == (1, K, waves) and shape[1] > shape[2], shape
    same_bits({"rows": v, "pos": pos}, in_calls(im, c, K))
    assert np.array_equal(v, np.stack(pathref.rows_from_positions(pos, ob[:, 0])))
    check_margins(hmm(im), ob, c, 326, pos[326:], "scratch cap")


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100"])
def test_full_and_ragged_batches(engine_opt, case):
    """130 paths in batches of 64, 64 and 2: every lane of a wavefront carries a path.  The bits of one path per wavefront; every
    draw of paths 60 .. 67 against the oracle."""
    im, contigs = manager(case, engine_opt)
    model = hmm(im)
    K = 130
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        engine_opt("SMCPP_PATH_BATCH", "64")
        full = {"pos": im.posterior_sample_positions(c, K, SEED)}
        assert launch(im, label + " positions") == (64, 3, 3)
        full["rows"] = rows(im, c, K, SEED)
        assert launch(im, label + " rows") == (64, 3, 3)
        engine_opt("SMCPP_PATH_BATCH", "1")
        one = {"pos": im.posterior_sample_positions(c, K, SEED)}
        assert launch(im, label + " one path per wavefront") == (1, K, K)
        one["rows"] = rows(im, c, K, SEED)
        assert launch(im, label + " one path per wavefront") == (1, K, K)
        same_bits(full, one)
        assert full["pos"].min() >= 0 and full["pos"].max() < im.M
        check_margins(model, ob, c, 60, full["pos"][60:68], label)
        assert np.array_equal(full["rows"], np.stack(pathref.rows_from_positions(full["pos"], ob[:, 0]))), label


@pytest.mark.parametrize("case", ["cut:M100", "long:M65"])
def test_windows_and_selections_under_batching(engine_opt, case):
    """8 paths in batches of 7 and 1: the early exits of a window of positions (the rows and blocks below it, the skipped column
    0) and the column selections are slices of the full results of one path per wavefront."""
    engine_opt("SMCPP_PATH_BATCH", None)
    im, contigs = long_rows_manager(65, engine_opt) if case == "long:M65" else manager(case, engine_opt)
    K = 8
    for c, ob in enumerate(contigs):
        label = f"{case} contig {c}"
        spans, L = ob[:, 0], len(ob)
        N = int(spans.sum())
        engine_opt("SMCPP_PATH_BATCH", None)
        pos = im.posterior_sample_positions(c, K, SEED)
        assert launch(im, label + " full") == (1, K, K)
        v = rows(im, c, K, SEED)
        engine_opt("SMCPP_PATH_BATCH", "7")
        for start, stop, step in _selections(L):
            got = rows(im, c, K, SEED, 0, start, stop, step)
            assert np.array_equal(got, v[:, :, slice(start, stop, step)]), (label, start, stop, step)
        assert launch(im, label + " selections") == (7, 2, 2)
        for p0, p1 in position_windows(spans):
            got = im.posterior_sample_positions(c, K, SEED, 0, p0, p1)
            assert got.shape == (K, p1 - p0) and np.array_equal(got, pos[:, p0:p1]), (label, p0, p1, N)
        assert launch(im, label + " windows") == (7, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# frequencies and counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def freq():
    """An own binned input of about 1000 positions at M = 64 after a save_gamma E-step, with the float64 marginals."""
    ob = tg.binned_contigs(13, 60_000)[0]
    N = int(ob[:, 0].sum())
    assert 700 <= N <= 1500, N
    im = tg._onepop(64, [ob], tg.TH_B, tg.RH_B)
    im.save_gamma = True
    im.E_step()
    return {"im": im, "ob": ob, "N": N, "g": pathref.marginals(*hmm(im), ob)}


def test_state_frequencies(freq):
    """4096 paths: at every position and state |frequency - marginal| <= sqrt(60 g (1 - g) / K) + 10 / K + GAMMA_TOL; the oracle's
    sampler is held to the same bound on the same input."""
    im, ob, g, K = freq["im"], freq["ob"], freq["g"], 4096
    pos = im.posterior_sample_positions(0, K, SEED)
    assert pos.shape == (K, freq["N"] + 1) and pos.min() >= 0 and pos.max() < im.M
    bound = pathref.frequency_bound(g, K, GAMMA_TOL)
    for name, p in (("device", pos), ("oracle", pathref.sample(*hmm(im), ob, SEED, 0, K))):
        ratio = np.abs(pathref.state_frequencies(p, im.M) - g) / bound
        print(f"{name}: worst frequency deviation {ratio.max():.2f} of the bound over {ratio.size} cells")
        assert ratio.max() <= 1.0, (name, np.argwhere(ratio > 1.0)[:8].tolist())


def test_counts_against_expectations(freq):
    """1024 paths: the mean contig totals of up and of down lie within six of the sample's own standard errors of the expected counts
    (posterior_transitions); the state at a row's end is distributed as that position's marginal."""
    im, ob, g, K = freq["im"], freq["ob"], freq["g"], 1024
    r = im.posterior_sample_rows(0, K, SEED)
    tr = im.posterior_transitions(0)
    for k in ("up", "down"):
        tot = r[k].sum(axis=1).astype(np.float64)
        se = tot.std(ddof=1) / np.sqrt(K)
        want = tr[k].sum()
        print(f"{k}: mean {tot.mean():.3f}, expected {want:.3f}, {abs(tot.mean() - want) / se:.2f} standard errors of {se:.3f}")
        assert se > 0.0
        assert abs(tot.mean() - want) <= 6.0 * se, (k, tot.mean(), want, se)
    P = np.concatenate([[0], np.cumsum(ob[:, 0])])
    f = pathref.state_frequencies(r["state"], im.M)
    ratio = np.abs(f - g[P]) / pathref.frequency_bound(g[P], K, GAMMA_TOL)
    print(f"state at the row ends: worst frequency deviation {ratio.max():.2f} of the bound")
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------------
CALLS = (lambda im, **kw: im.posterior_sample_rows(0, **kw), lambda im, **kw: im.posterior_sample_positions(0, **kw))


@pytest.mark.parametrize("case", ["scan:M64", "cut:M100"])
def test_errors(engine_opt, case):
    """Every refusal raises RuntimeError with a message that names the cause, before anything is launched; the manager still works."""
    fresh, _ = tpt.manager(case, engine_opt, estep=False)
    fresh.save_gamma = True
    for call in CALLS:
        with pytest.raises(RuntimeError, match="E-step"):
            call(fresh)
    im, contigs = manager(case, engine_opt)
    L, nc = len(contigs[0]), len(contigs)
    N = int(contigs[0][:, 0].sum())
    good = products(im, 0, 2)

    def raises(call, match):
        with pytest.raises(RuntimeError, match=match) as e:
            call()
        assert str(e.value).strip()
        same_bits(products(im, 0, 2), good)

    for c in (-1, nc, nc + 5):
        raises(lambda: im.posterior_sample_rows(c), "contig")
        raises(lambda: im.posterior_sample_positions(c), "contig")
    for kw in (dict(start=-1), dict(stop=L + 2), dict(start=3, stop=3), dict(start=4, stop=2), dict(step=0), dict(step=-1),
               dict(start=L + 1)):
        raises(lambda: im.posterior_sample_rows(0, **kw), "start|stop|step|selection")
    for kw, match in ((dict(pos0=-1), "pos0"), (dict(pos1=N + 2), "pos1"), (dict(pos0=5, pos1=5), "empty window"),
                      (dict(pos0=9, pos1=4), "empty window"), (dict(pos0=N + 1), "empty window")):
        raises(lambda: im.posterior_sample_positions(0, **kw), match)
    for call in CALLS:
        raises(lambda: call(im, n_paths=0), "n_paths")
        raises(lambda: call(im, n_paths=-3), "n_paths")
        raises(lambda: call(im, first_path=-1), "first_path")
        raises(lambda: call(im, first_path=2 ** 31 - 1, n_paths=2), "2\\^31")
        raises(lambda: call(im, first_path=2 ** 31), "2\\^31")
        raises(lambda: call(im, n_paths=2 ** 31 - 1), "fewer paths or a narrower window")
    same_bits({"pos": im.posterior_sample_positions(0, 1, SEED, 2 ** 31 - 1, 0, 3)}, {"pos": im.posterior_sample_positions(0, 1, SEED, 2 ** 31 - 1)[:, :3]})
    # the parameters set again without an E-step
    im.theta = im.theta * 1.0
    for call in CALLS:
        with pytest.raises(RuntimeError, match="E-step"):
            call(im)
    im.E_step()
    same_bits(products(im, 0, 2), good)
    # the last E-step ran without save_gamma
    im.save_gamma = False
    im.E_step()
    for call in CALLS:
        with pytest.raises(RuntimeError, match="save_gamma"):
            call(im)
    assert np.all(np.isfinite(im.logliks()))
    im.save_gamma = True
    im.E_step()
    same_bits(products(im, 0, 2), good)


def test_unstructured_transition_matrix_is_refused(engine_opt):
    im, contigs = tg.run_case("eig_big:M96:unstructured", engine_opt)
    gam = im.gammas[0]
    for call in CALLS + (lambda im: im.posterior_sample_rows(1, 3, 5, 0, 0, 1, 1),):
        with pytest.raises(RuntimeError, match="semiseparable structure"):
            call(im)
    assert np.array_equal(im.posterior_columns(0, normalize=False), gam)


# ---------------------------------------------------------------------------------------------------------------------------------
# the Cython manager, posterior_products
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cython_manager_gives_the_same_bits(engine_opt):
    from smcpp_amd import _build, synth
    _build.build_cython()
    from smcpp_amd import _smcpp_cy as cy
    from smcpp_amd.model import AdPiecewiseModel
    im, contigs = tg.run_case("scan:M64", engine_opt)
    a, s = synth.model_pieces()
    im2 = cy.PyOnePopInferenceManager(tg.N, contigs, synth.hidden_states(im.M), ("pop1",), 0.5)
    im2.model = AdPiecewiseModel(a, s, 1e4, "pop1", differentiable=[])
    im2.theta = tg.TH_B; im2.rho = tg.RH_B; im2.alpha = 1.0
    im2.save_gamma = True
    im2.E_step()
    for c in range(len(contigs)):
        same_bits(products(im2, c, 3), products(im, c, 3))
        assert np.array_equal(rows(im2, c, 2, SEED, 1, 1, None, 7), rows(im, c, 2, SEED, 1, 1, None, 7))
        assert np.array_equal(im2.posterior_sample_positions(c, 2, SEED, 1, 0, 1), im.posterior_sample_positions(c, 2, SEED, 1, 0, 1))
    with pytest.raises(RuntimeError, match="n_paths"):
        im2.posterior_sample_rows(0, n_paths=0)
    with pytest.raises(RuntimeError, match="pos1"):
        im2.posterior_sample_positions(0, pos1=10 ** 9)


def test_posterior_products_with_paths(tmp_path):
    """posterior_products(paths=3, seed=s): the arrays of the manager's own call; paths=0: today's key set; the file round-trips."""
    from smcpp_amd import synth
    from smcpp_amd.model import PiecewiseModel
    from smcpp_amd.posterior import posterior_products, save_products_npz
    a, s = synth.model_pieces()
    model = PiecewiseModel(a, s, 1e4, "pop1")
    raw = [synth.synth_posterior_contig(200, tg.N, seed=21), synth.synth_posterior_contig(90, tg.N, seed=22)]
    args = (model, raw, 16, tg.N, tg.TH_U, tg.RH_U)
    today = ["mean_tmrca", "path", "qstate", "sites"]
    new = ["path_state", "path_up", "path_down"]
    hs, prods, im = posterior_products(*args, paths=3, seed=SEED, return_manager=True)
    for c, pr in enumerate(prods):
        assert sorted(pr) == sorted(today + new)
        own = im.posterior_sample_rows(c, 3, SEED)
        ncol = len(pr["sites"]) + 1
        for k in NAMES:
            assert pr["path_" + k].shape == (3, ncol) and pr["path_" + k].dtype == np.int32
            assert np.array_equal(pr["path_" + k], own[k]), (c, k)
        assert np.array_equal(np.stack([pr["path_" + k] for k in NAMES]),
                              np.stack(pathref.rows_from_positions(im.posterior_sample_positions(c, 3, SEED), pr["sites"])))
    hs2, plain = posterior_products(*args)
    assert all(sorted(pr) == today for pr in plain)
    _, zero = posterior_products(*args, paths=0, seed=5)
    assert all(sorted(pr) == today for pr in zero)
    for pr, pl in zip(prods, plain):
        for k in today:
            assert pr[k].dtype == pl[k].dtype and np.array_equal(pr[k], pl[k]), k
    _, both = posterior_products(*args, window=1000, transitions=True, paths=1)
    assert all(sorted(pr) == sorted(today + new + ["windows", "transitions", "transition_windows"]) for pr in both)
    _, one = posterior_products(*args, paths=1, seed=SEED)
    assert all(np.array_equal(o["path_" + k], p["path_" + k][:1]) for o, p in zip(one, prods) for k in NAMES)
    names = ["chr1.smc.gz", "chr2.smc.gz"]
    path = tmp_path / "products.npz"
    save_products_npz(str(path), hs, prods, names)
    z = np.load(str(path))
    keys = today + new
    assert sorted(z.files) == sorted(["hidden_states"] + [f"{nm}_{k}" for nm in names for k in keys])
    for nm, pr in zip(names, prods):
        for k in keys:
            assert z[f"{nm}_{k}"].dtype == pr[k].dtype and np.array_equal(z[f"{nm}_{k}"], pr[k]), (nm, k)
    path2 = tmp_path / "plain.npz"
    save_products_npz(str(path2), hs2, plain, names)
    assert sorted(np.load(str(path2)).files) == sorted(["hidden_states"] + [f"{nm}_{k}" for nm in names for k in today])
