"""The device data shaping (smcpp_amd/csrc/shaping.hpp: Thin -> Bin -> Compress behind `smcpp_dev_shape`) at its block and scan edges.

tests/test_gpu_shaping.py holds the kernels to the reference's goldens and to the host loops on one random contig; this module holds
them, BIT FOR BIT (same shape, int32, `np.array_equal`), to the vectorised position-based oracle tests/shaperef.py (pinned to the host
loops and to golden G23 by tests/test_shaperef.py) where index code goes wrong:

  a  the scan's tiles: L on both sides of 256 and 2048            g  every thinning phase, thinning == P and > P
  b  the second level of the scan: nb = 1024 / 1025 / 2049        h  columns: ncol 4 / 7 / 10, every na, sum a == 2, missing a
  c  one source row that holds whole emit blocks                  i  more than 2^31 positions
  d  zero-count items that fill whole blocks and tiles            j  the per-thread work area: big -> small -> big, ncol changes,
  e  nout / nbins exactly at 1, 255, 256, 257, 512, 513              fresh and poisoned allocations
  f  bins of > 256 and > 2048 rows, w > P, w = 1, P % w           k  refused calls leave the previous result fetchable

Every test first asserts, from quantities computed on the host (shaperef's `info`, `scan_plan`, `emit_blocks`), that its input reaches
the branch it is named for; inputs are seeded.  Mutated kernels are not run on the GPU (a wrong prefix walks out of a buffer): the
reach assertions are what shows that a wrong index would be seen.

Wall time of every test on one MI355X, oracle included (the whole module: 6 s beside tests/test_gpu_shaping.py):
  a  0.23 s the first size (it opens the device), 0.01 s every other      f  0.06 s            j  0.38 s (39 device calls, 3 threads)
  b  thin 0.31 / 0.32 s, bin 0.16 / 0.25 s, compress 0.08 / 0.15 s,       g  0.06 s            k  0.01 s
     pipeline 0.29 / 0.45 s at 2^21 / 2^21 + 1 rows; 2^22 + 1 rows        h  0.01 s each
     0.21 s; equal rows 0.04 s                                            i  < 0.005 s
  c  0.16 / 0.17 s        d  0.01 s        e  < 0.005 s each
Oracle calls alone, timed on one core of a slower CPU than that host's: 2^21 rows - thin 0.9 - 1.0 s (3.1 10^6 rows out),
bin 0.8 - 1.1 s, bin of the thinned rows 0.9 - 1.3 s, compress 0.15 - 0.3 s; 2^22 + 1 rows - compress 0.3 s; the 10^6-position row -
thin 0.13 s, bin at w = 1 0.11 s; everything else below 0.05 s.
"""
import threading

import numpy as np
import pytest

import shaperef as R

pytestmark = pytest.mark.gpu

THIN, BIN, COMPRESS, PIPELINE = 0, 1, 2, 3
NA = {4: [2], 7: [1, 1], 10: [1, 1, 0]}
SMALL = tuple(range(6))                      # spans 0 .. 5


def _device(mode, rows, p0=0, p1=0, na=None):
    from smcpp_amd import data as D
    return D._shape_on_device(mode, rows, p0, p1, na=na)


def _oracle(mode, rows, p0=0, p1=0, na=None):
    if mode == THIN:
        return R.thin(rows, p0, p1)
    if mode == BIN:
        return R.bin_(rows, p0, na)
    if mode == COMPRESS:
        return R.compress(rows)
    return R.pipeline(rows, p0, p1, na)


def _check(mode, rows, p0=0, p1=0, na=None, want=None, what=None):
    if want is None:
        want = _oracle(mode, rows, p0, p1, na)
    got = _device(mode, rows, p0, p1, na)
    what = what if what is not None else (mode, rows.shape, p0, p1, na)
    assert got.dtype == np.int32 and want.dtype == np.int32, what
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, f"{int(np.sum(np.any(got != want, axis=1)))} of {len(want)} rows differ, "
                                             f"first at {int(np.flatnonzero(np.any(got != want, axis=1))[0])}")
    return got


def _with_positions(rows):
    if rows[:, 0].sum() == 0:
        rows[0, 0] = 3
    return rows


def _aligned_zero_group(counts, group):
    """True if some aligned group of `group` consecutive items (a 256-block, a 2048-tile of the scan) produces no output at all."""
    c = np.asarray(counts)
    c = c[:len(c) // group * group].reshape(-1, group)
    return bool(np.any(c.sum(axis=1) == 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the scan's tiles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097))
def test_a_scan_tiles(L):
    nb, per = R.scan_plan(L)
    assert nb == {1: 1, 2: 1, 255: 1, 256: 1, 257: 1, 2047: 1, 2048: 1, 2049: 2, 4097: 3}[L] and per == 1
    for ncol in (4, 7):
        rng = np.random.default_rng(100 * L + ncol)
        rows = _with_positions(R.random_rows(rng, L, ncol, spans=SMALL))
        _check(THIN, rows, 3, 1)
        _check(BIN, rows, 4, 0, NA[ncol])
        _check(PIPELINE, rows, 3, 4, NA[ncol])
        runs = R.random_rows(rng, L, ncol, spans=SMALL, max_run=9)
        want = R.compress(runs)
        assert L < 255 or L / 9 <= len(want) < L
        _check(COMPRESS, runs, want=want)
        distinct = runs.copy()
        distinct[:, 2] = np.arange(L)
        want = R.compress(distinct)
        assert len(want) == L                               # nout = L: every emit thread of every block has a run of its own
        _check(COMPRESS, distinct, want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the second level of the scan
# ---------------------------------------------------------------------------------------------------------------------------------
_BIG = {}


def _big_rows(L, runs=False):
    """ncol = 4 at 2^21 rows, 7 at 2^21 + 1 (34 / 59 MB), 4 at 2^22 + 1 (67 MB); built once per size."""
    key = (L, runs)
    if key not in _BIG:
        ncol = 7 if L == 2097153 else 4
        rows = R.random_rows(np.random.default_rng(L % 1000 + runs), L, ncol, spans=SMALL, max_run=9 if runs else 1)
        rows.setflags(write=False)
        _BIG[key] = rows
    return _BIG[key]


def _big_thinned(L):
    """The oracle's thinning (5, offset 0) of `_big_rows(L)`: the thin test and the pipeline test of a size share it."""
    key = (L, "thinned")
    if key not in _BIG:
        _BIG[key] = R.thin(_big_rows(L), 5, 0)
        _BIG[key].setflags(write=False)
    return _BIG[key]


def _assert_second_level(n, nb, per):
    assert R.scan_plan(n) == (nb, per)
    idle = 1024 - -(-nb // per)                              # threads of k_scan_of_partials whose range [lo, hi) is empty
    assert idle == {1: 0, 2: 511, 3: 341}[per]


@pytest.mark.parametrize("mode", (THIN, BIN, COMPRESS, PIPELINE))
@pytest.mark.parametrize("L,nb,per", ((2097152, 1024, 1), (2097153, 1025, 2)))
def test_b_second_level_of_the_scan(L, nb, per, mode):
    _assert_second_level(L, nb, per)
    rows = _big_rows(L, runs=mode == COMPRESS)
    na = NA[rows.shape[1]]
    if mode == THIN:
        want = _big_thinned(L)
        assert R.scan_plan(len(want))[1] == 2               # (more than 2^21 outputs as well)
        _check(THIN, rows, 5, 0, want=want)
    elif mode == BIN:
        _check(BIN, rows, 2, 0, na)
    elif mode == COMPRESS:
        want = R.compress(rows)
        assert 1 < len(want) < L
        _check(COMPRESS, rows, want=want)
    else:
        t = _big_thinned(L)
        b = R.bin_(t, 2, na)
        assert R.scan_plan(len(t))[1] == 2 and R.scan_plan(len(b))[1] == 2      # every step of the pipeline scans past 2^21 items
        _check(PIPELINE, rows, 5, 2, na, want=R.compress(b))


def test_b_compress_with_three_block_sums_per_thread():
    L = 4194305
    _assert_second_level(L, 2049, 3)
    rows = _big_rows(L, runs=True)
    want = R.compress(rows)
    assert R.scan_plan(len(want))[0] > 256
    _check(COMPRESS, rows, want=want)


def test_b_compress_of_equal_rows_into_one():
    L = 2097153
    _assert_second_level(L, 1025, 2)
    rows = np.tile(np.array([[2, 1, 0, 3, 0, 2, 2]], dtype=np.int32), (L, 1))
    want = R.compress(rows)
    assert want.shape == (1, 7) and int(want[0, 0]) == 2 * L
    _check(COMPRESS, rows, want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. one source row, many outputs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surrounded", (False, True))
def test_c_one_row_holds_whole_emit_blocks(surrounded):
    big = np.array([[1_000_000, 1, 2, 3, 0, 1, 3]], dtype=np.int32)
    if surrounded:
        rng = np.random.default_rng(31)
        rows = np.concatenate((R.random_rows(rng, 300, 7, spans=(0, 1, 2, 3)), big, R.random_rows(rng, 300, 7, spans=(0, 1, 2, 3))))
    else:
        rows = big
    for offset in (0, 1, 2):
        want, info = R.thin(rows, 3, offset, info=True)
        assert info["counts"].max() > 600_000 and R.full_single_holder_blocks(info["counts"]) > 2000
        _check(THIN, rows, 3, offset, want=want)
    for w in (1, 7):
        want, info = R.bin_(rows, w, NA[7], info=True)
        fr, full = info["first_row"], info["nbins"] // 256
        assert int(np.sum(fr[0:full * 256:256] == fr[255:full * 256:256])) > 500      # blocks whose 256 bins all start in one row
        if surrounded:
            assert int(np.sum(fr[0:full * 256:256] != fr[255:full * 256:256])) >= 1   # ... and blocks that cross into and out of it
        _check(BIN, rows, w, 0, NA[7], want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. zero-count items
# ---------------------------------------------------------------------------------------------------------------------------------
def _zero_layout(ncol, zero_spans, first):
    """Runs of `first`, 300 and 2100 rows that produce nothing - at the start, in the middle, back to back, at the end - between
    random rows.  The rows of a run are equal and carry the LARGEST sample size of the input: a bin that looked at them would pick
    them.  zero_spans: their span is 0 (nothing for thin, no overlap for bin); otherwise it is positive (no head for compress)."""
    rng = np.random.default_rng(41 + ncol)
    parts = []
    for kind, n in (("z", first), ("n", 50), ("z", 300), ("n", 700), ("z", 300), ("z", 2100), ("n", 3000), ("z", 2100), ("n", 10),
                    ("z", 300)):
        if kind == "n":
            parts.append(R.random_rows(rng, n, ncol, spans=(0, 1, 2, 3, 4)))
        else:
            z = np.zeros((n, ncol), dtype=np.int32)
            z[:, 1::3], z[:, 2::3], z[:, 3::3] = 1, len(parts) % 3, 5
            z[:, 0] = 0 if zero_spans else rng.integers(1, 4, n)
            parts.append(z)
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.parametrize("ncol", (4, 7))
def test_d_zero_count_items(ncol):
    rows = _zero_layout(ncol, True, 2100)
    want, info = R.thin(rows, 3, 0, info=True)
    c = info["counts"]
    assert c[0] == 0 and c[-1] == 0 and R.zero_runs(c) >= 2400 and _aligned_zero_group(c, 256) and _aligned_zero_group(c, 2048)
    _check(THIN, rows, 3, 0, want=want)
    _check(THIN, rows, 400, 5, want=None)
    want, info = R.bin_(rows, 3, NA[ncol], info=True)
    ss = rows[:, 3::3].sum(axis=1)
    assert np.all(rows[info["chosen"], 0] > 0) and ss[rows[:, 0] > 0].max() < ss.max()      # (the largest sample size sits in rows without positions only)
    _check(BIN, rows, 3, 0, NA[ncol], want=want)
    _check(BIN, rows, 1, 0, NA[ncol])
    _check(PIPELINE, rows, 3, 3, NA[ncol])
    _check(COMPRESS, rows)
    runs = _zero_layout(ncol, False, 4200)
    want, info = R.compress(runs, info=True)
    c = info["counts"]
    assert c[-1] == 0 and R.zero_runs(c) >= 4199 and _aligned_zero_group(c, 256) and _aligned_zero_group(c, 2048)
    _check(COMPRESS, runs, want=want)


def test_d_thin_of_rows_without_positions():
    rows = R.random_rows(np.random.default_rng(43), 500, 7, spans=(0,))
    want = R.thin(rows, 3, 0)
    assert want.shape == (0, 7)
    _check(THIN, rows, 3, 0, want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. output counts at the emit block
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 255, 256, 257, 512, 513))
def test_e_output_counts_at_the_emit_block(N):
    rng = np.random.default_rng(500 + N)
    # thin: one row of span N at thinning 2 is N pieces (thinned, kept, thinned, kept, ...)
    one = np.array([[N, 1, 1, 2, 0, 2, 3]], dtype=np.int32)
    want = R.thin(one, 2, 0)
    assert len(want) == N
    _check(THIN, one, 2, 0, want=want)
    # thin: random rows at thinning 3, cut where they have produced at most N outputs, topped up with span-1 rows (one output each)
    rows = R.random_rows(rng, N, 7, spans=(0, 1, 2, 3, 7))
    _, info = R.thin(rows, 3, 1, info=True)
    keep = int(np.searchsorted(np.cumsum(info["counts"]), N, side="right"))
    rows = rows[:keep]
    have = len(R.thin(rows, 3, 1)) if keep else 0
    rows = np.ascontiguousarray(np.concatenate((rows, R.random_rows(rng, N - have, 7, spans=(1,)))))
    want = R.thin(rows, 3, 1)
    assert len(want) == N
    _check(THIN, rows, 3, 1, want=want)
    # compress: N runs of 1 - 9 rows
    obs = R.random_rows(rng, N, 7, spans=(1,))
    obs[:, 2] = np.arange(N)
    runs = np.repeat(obs, rng.integers(1, 10, N), axis=0)
    runs[:, 0] = rng.integers(0, 6, len(runs))
    want = R.compress(runs)
    assert len(want) == N
    _check(COMPRESS, runs, want=want)
    # bin: N bins of 3 positions, the last one full (P % w == 0) and holding one position only
    for target in (3 * N, 3 * (N - 1) + 1):
        rows = R.random_rows(rng, N // 2, 7, spans=SMALL)
        P0 = int(rows[:, 0].sum())
        assert P0 < target
        last = R.random_rows(rng, 1, 7, spans=(target - P0,))
        rows = np.ascontiguousarray(np.concatenate((rows, last)))
        want, info = R.bin_(rows, 3, NA[7], info=True)
        assert len(want) == N and info["P"] == target
        _check(BIN, rows, 3, 0, NA[7], want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. bins
# ---------------------------------------------------------------------------------------------------------------------------------
def test_f_bins():
    rng = np.random.default_rng(61)
    ones = R.random_rows(rng, 5000, 7, spans=(1,))
    want, info = R.bin_(ones, 100_000, NA[7], info=True)      # w > P: one bin, 5000 rows in it
    assert len(want) == 1 and info["rows_per_bin"].tolist() == [5000]
    _check(BIN, ones, 100_000, 0, NA[7], want=want)
    want, info = R.bin_(ones, 300, NA[7], info=True)          # > 256 rows per bin, P % w != 0
    assert info["rows_per_bin"].min() > 256 - 100 and info["rows_per_bin"].max() == 300 and info["P"] % 300 != 0
    _check(BIN, ones, 300, 0, NA[7], want=want)
    many = R.random_rows(rng, 250_000, 4, spans=(1,))
    want, info = R.bin_(many, 100_000, NA[4], info=True)      # > 2048 rows in every bin
    assert info["rows_per_bin"].tolist() == [100_000, 100_000, 50_000]
    _check(BIN, many, 100_000, 0, NA[4], want=want)
    rows = R.random_rows(rng, 3000, 7, spans=SMALL)
    pad = -int(rows[:, 0].sum()) % 6
    rows[-1, 0] += pad if (int(rows[:, 0].sum()) + pad) % 7 else pad + 6          # P a multiple of 2 and 3, not of 7
    start, end = R.positions(rows)
    P = int(end[-1])
    for w in (1, 2, 3, 7, P, P + 1, P - 1):
        want, info = R.bin_(rows, w, NA[7], info=True)
        assert info["nbins"] == -(-P // w)
        _check(BIN, rows, w, 0, NA[7], want=want)
    assert P % 7 != 0 and P % 2 == 0 and P % 3 == 0
    # a row that ends exactly on a bin boundary, followed by a row of span 0 (it belongs to neither bin)
    on_edge = (end[:-1] % 3 == 0) & (rows[:-1, 0] > 0) & (rows[1:, 0] == 0)
    assert int(on_edge.sum()) > 20
    hand = np.array([[3, 0, 0, 1], [0, 1, 0, 3], [2, 1, 0, 0], [1, 0, 1, 1], [0, 1, 0, 3], [0, 1, 0, 3], [4, 0, 0, 0], [2, 1, 0, 0]], dtype=np.int32)
    _check(BIN, hand, 3, 0, NA[4])


# ---------------------------------------------------------------------------------------------------------------------------------
# g. the thinning phase
# ---------------------------------------------------------------------------------------------------------------------------------
def _phase_rows(rows, thinning, offset):
    """`rows` followed by rows placed on the thinning phase: one that ends exactly on a kept position (its span is the distance to the
    first kept position), one that starts just behind it and ends on the next, one that ends one position short of a kept one, one
    that is a kept position and nothing else, one that holds three of them."""
    P0 = int(rows[:, 0].sum())
    d = thinning - (offset + P0) % thinning
    tail = rows[:5].copy()
    tail[:, 0] = (d, thinning, thinning - 1, 1, 3 * thinning + 1)
    return np.ascontiguousarray(np.concatenate((rows, tail)))


def test_g_thinning_phase():
    base = R.random_rows(np.random.default_rng(71), 3000, 7)
    for thinning in (1, 2, 3, 400):
        for offset in (0, thinning - 1, thinning, thinning + 5):
            rows = _phase_rows(base, thinning, offset) if offset < thinning else base
            start, end = R.positions(rows)
            span = rows[:, 0].astype(np.int64)
            want, info = R.thin(rows, thinning, offset, info=True)
            assert bool(info["kept"].any()) == (offset < thinning)
            if offset < thinning and thinning > 1:
                to_first = thinning - (offset + start) % thinning          # positions up to and including the first kept one
                assert np.any((span > 0) & ((offset + end) % thinning == 0))              # rows that end on a kept position
                assert np.any((span > 0) & ((offset + start) % thinning == 0))            # rows that start just behind one
                assert np.any(span == to_first) and np.any((span > 0) & (span == to_first - 1))
                assert np.any((span == 1) & (to_first == 1)) and np.any(span > 2 * thinning + to_first)
            _check(THIN, rows, thinning, offset, want=want)
    rows = base
    P = int(rows[:, 0].sum())
    for thinning, n_kept in ((P, 1), (P + 1, 0), (P - 1, 1)):
        want, info = R.thin(rows, thinning, 0, info=True)
        assert int(info["kept"].sum()) == n_kept
        _check(THIN, rows, thinning, 0, want=want)
    want, info = R.thin(rows, P, P - 1, info=True)           # offset = thinning - 1: the first position is kept, and no other
    assert info["kept"].tolist() == [True] + [False] * (len(want) - 1)
    _check(THIN, rows, P, P - 1, want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# h. columns
# ---------------------------------------------------------------------------------------------------------------------------------
def test_h_ten_columns_once_per_mode():
    rng = np.random.default_rng(81)
    rows = R.random_rows(rng, 5000, 10, spans=(0, 1, 1, 2, 3, 7, 50))
    _check(THIN, rows, 7, 3)
    _check(BIN, rows, 10, 0, NA[10])
    _check(COMPRESS, R.random_rows(rng, 5000, 10, spans=SMALL, max_run=9))
    _check(PIPELINE, rows, 7, 10, NA[10])


def test_h_distinguished_lineages_and_the_second_clause_of_the_bin_rule():
    rng = np.random.default_rng(82)
    main = R.random_rows(rng, 20_000, 4, spans=(1, 1, 1, 2, 3), p_nb0=0.8)
    want, info = R.bin_(main, 10, [2], info=True)
    decided = float(np.mean(info["chosen"] != info["first_max"]))
    assert decided >= 0.05, decided                          # the `max_ss == 2 and seg == 1` clause picked another row than the first maximum
    _check(BIN, main, 10, 0, [2], want=want)
    for ncol, nas in ((7, ([2, 0], [1, 1], [0, 2])), (10, ([1, 1, 0],))):
        rows = R.random_rows(rng, 6000, ncol, spans=(0, 1, 1, 2, 3, 7), p_nb0=0.7)
        for na in nas:
            want, info = R.bin_(rows, 5, na, info=True)
            assert np.any(info["chosen"] != info["first_max"]) and np.any(info["chosen"] != info["first_row"])
            _check(BIN, rows, 5, 0, na, want=want)


def test_h_recoded_and_missing_rows_at_kept_and_thinned_positions():
    rng = np.random.default_rng(83)
    for ncol, forms in ((4, ((2,), (-1,))), (7, ((1, 1), (2, 0), (0, 2), (-1, -1), (-1, 1)))):
        rows = R.random_rows(rng, 4000, ncol, spans=(0, 1, 1, 2, 3, 7))
        want, info = R.thin(rows, 3, 1, info=True)
        a = rows[info["src"], 1::3]
        for form in forms:
            m = np.all(a == np.array(form)[None, :], axis=1)
            assert np.any(m & info["kept"]) and np.any(m & ~info["kept"]), form
            if sum(form) == 2:
                assert not want[m, 1:].any()                # (written as all zeros in both kinds of piece)
        _check(THIN, rows, 3, 1, want=want)
        _check(PIPELINE, rows, 3, 2, NA[ncol])


# ---------------------------------------------------------------------------------------------------------------------------------
# i. more than 2^31 positions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_i_more_than_two_to_the_31_positions():
    rng = np.random.default_rng(91)
    parts = []
    for k in range(3):
        parts.append(R.random_rows(rng, 7, 7, spans=(0, 1, 2, 3, 7, 50)))
        parts.append(np.array([[2_000_000_000, k % 2, 1, 2, 1 - k % 2, 0, 3]], dtype=np.int32))
    parts.append(R.random_rows(rng, 7, 7, spans=(0, 1, 2, 3, 7, 50)))
    rows = np.ascontiguousarray(np.concatenate(parts))
    start, end = R.positions(rows)
    P = int(end[-1])
    assert P > 6_000_000_000 and int(np.sum(end > 2 ** 31)) >= 16 and int(np.sum(start > 2 ** 32)) >= 7
    for offset in (0, 999_999):
        want, info = R.thin(rows, 1_000_000, offset, info=True)
        assert int(info["kept"].sum()) == (P + offset) // 1_000_000 and int(want[:, 0].astype(np.int64).sum()) == P
        _check(THIN, rows, 1_000_000, offset, want=want)
    want, info = R.bin_(rows, 1_000_000, NA[7], info=True)
    assert len(want) == -(-P // 1_000_000) > 6000
    _check(BIN, rows, 1_000_000, 0, NA[7], want=want)
    rows[:, 2] = np.arange(len(rows)) % 2                   # neighbours differ: no run adds two spans, none reaches 2^31
    want = R.compress(rows)
    assert len(want) == len(rows) and np.array_equal(want[:, 0], rows[:, 0]) and int(want[:, 0].astype(np.int64).sum()) == P > 2 ** 31
    _check(COMPRESS, rows, want=want)


# ---------------------------------------------------------------------------------------------------------------------------------
# j. the work area
# ---------------------------------------------------------------------------------------------------------------------------------
def _work_area_calls():
    rng = np.random.default_rng(101)
    big4 = R.random_rows(rng, 300_000, 4, spans=SMALL)
    big7 = R.random_rows(rng, 200_000, 7, spans=SMALL)
    small4 = R.random_rows(rng, 100, 4, spans=SMALL)
    small7 = R.random_rows(rng, 37, 7, spans=SMALL)
    runs4 = R.random_rows(rng, 250_000, 4, spans=SMALL, max_run=9)
    calls = [(THIN, big4, 3, 0, None), (BIN, small4, 4, 0, NA[4]), (PIPELINE, big4, 5, 3, NA[4]), (COMPRESS, small7, 0, 0, None),
             (THIN, big7, 2, 1, None), (PIPELINE, small7, 3, 2, NA[7]), (BIN, big7, 3, 0, NA[7]), (COMPRESS, runs4, 0, 0, None),
             (THIN, small4, 400, 0, None), (PIPELINE, big7, 7, 5, NA[7]), (BIN, big4, 1, 0, NA[4]), (THIN, small7, 1, 0, None),
             (COMPRESS, big4, 0, 0, None)]
    sizes = [c[1].size for c in calls]
    ncols = [c[1].shape[1] for c in calls]
    assert any(sizes[i] > 100 * sizes[i + 1] and sizes[i + 2] > 100 * sizes[i + 1] for i in range(len(calls) - 2))     # big -> small -> big
    assert any(ncols[i:i + 3] in ([4, 7, 4], [7, 4, 7]) for i in range(len(calls) - 2)) and len(calls) >= 12
    return calls


def _run_calls(calls):
    return [_device(*c) for c in calls]


def _in_fresh_thread(fn, *args):
    box = {}

    def body():
        try:
            box["out"] = fn(*args)
        except BaseException as e:                           # noqa: BLE001 - handed to the calling thread
            box["err"] = e
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def test_j_work_area_reuse_fresh_threads_and_poison(engine_opt):
    calls = _work_area_calls()
    want = [_oracle(*c) for c in calls]
    engine_opt("SMCPP_DEBUG_POISON", None)
    runs = {"reused area": _run_calls(calls), "fresh thread": _in_fresh_thread(_run_calls, calls)}
    engine_opt("SMCPP_DEBUG_POISON", "255")                 # every allocation of the next thread is fresh: all of them are filled with -1
    runs["fresh thread, poisoned"] = _in_fresh_thread(_run_calls, calls)
    engine_opt("SMCPP_DEBUG_POISON", None)
    for name, got in runs.items():
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (name, k, calls[k][0], calls[k][1].shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# k. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_k_refused_calls_leave_the_previous_result_fetchable():
    from smcpp_amd import _engine as E
    rng = np.random.default_rng(111)
    good_rows = R.random_rows(rng, 500, 4, spans=SMALL)
    good = _check(THIN, good_rows, 3, 0)
    r7 = R.random_rows(rng, 900, 7, spans=SMALL)
    refused = {"unknown mode": (4, r7, 1, 1, NA[7]), "mode -1": (-1, r7, 1, 1, NA[7]),
               "thinning 0": (THIN, r7, 0, 0, None), "thinning -3": (THIN, r7, -3, 0, None), "pipeline thinning 0": (PIPELINE, r7, 0, 5, NA[7]),
               "w 0 (bin)": (BIN, r7, 0, 0, NA[7]), "w -1 (bin)": (BIN, r7, -1, 0, NA[7]), "w 0 (pipeline)": (PIPELINE, r7, 3, 0, NA[7]),
               "w -2 (pipeline)": (PIPELINE, r7, 3, -2, NA[7]), "na None (bin)": (BIN, r7, 3, 0, None),
               "na None (pipeline)": (PIPELINE, r7, 3, 3, None),
               "ncol 5": (THIN, np.ones((10, 5), np.int32), 3, 0, None), "ncol 3": (COMPRESS, np.ones((10, 3), np.int32), 0, 0, None),
               "L 0": (THIN, np.zeros((0, 7), np.int32), 3, 0, None)}
    for name, call in refused.items():
        with pytest.raises(RuntimeError) as err:
            _device(*call)
        assert str(err.value).strip(), name
        # the C ABI allows a fetch after an error: the host buffer is sized for the larger of the two column counts
        buf = np.full(len(good) * 7, -77, dtype=np.int32)
        E.check(E.lib().smcpp_dev_shape_fetch(E.iptr(buf)))
        assert np.array_equal(buf[:good.size].reshape(good.shape), good), name
        assert np.all(buf[good.size:] == -77), name
    _check(PIPELINE, r7, 3, 4, NA[7])
