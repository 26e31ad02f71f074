"""tests/shaperef.py (the vectorised, position-based oracle of the device data shaping) against the host implementation
`smcpp_amd.data.thin_data` / `bin_observations` - the reference's loops with their carried counters, pinned by golden G23 - and
against G23 itself, bit for bit.  CPU only."""
import os
import zlib

import numpy as np
import pytest

import shaperef as R
from conftest import GOLDEN

THIN_PAIRS = ((1, 0), (2, 0), (2, 1), (7, 0), (7, 3), (7, 6), (5, 9), (100000, 0))
WIDTHS = (1, 2, 3, 10, 64, 100000)
NA = {4: ([2],), 7: ([2, 0], [1, 1], [0, 2]), 10: ([1, 1, 0], [2, 0, 0], [0, 1, 1])}
N_INPUTS = 96


def _same(got, want, what):
    assert got.dtype == np.int32 and want.dtype == np.int32, what
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), what


def _input(i):
    rng = np.random.default_rng(1000 + i)
    ncol = (4, 7, 10)[i % 3]
    L = int(rng.integers(1, 401)) if i >= 9 else 1 + i // 3          # (1, 2 and 3 rows at every ncol, then 1 - 400)
    return R.random_rows(rng, L, ncol)


def test_the_oracle_equals_the_host_loops_on_random_small_inputs():
    from smcpp_amd import data as D
    seen_thin, seen_w, seen_ncol, n_second_clause, n_sa2_kept, n_sa2_thinned = set(), set(), set(), 0, 0, 0
    for i in range(N_INPUTS):
        rows = _input(i)
        ncol = rows.shape[1]
        seen_ncol.add(ncol)
        for thinning, offset in (THIN_PAIRS[i % 8], THIN_PAIRS[(i // 8 + 3 + i) % 8]):
            got, info = R.thin(rows, thinning, offset, info=True)
            _same(got, D.thin_data(rows, thinning, offset), ("thin", i, thinning, offset))
            seen_thin.add((thinning, offset))
            sa2 = rows[info["src"], 1::3].sum(axis=1) == 2
            n_sa2_kept += int(np.sum(sa2 & info["kept"]))
            n_sa2_thinned += int(np.sum(sa2 & ~info["kept"]))
            assert int(got[:, 0].astype(np.int64).sum()) == info["P"] and np.array_equal(info["counts"] == 0, rows[:, 0] == 0)
        if rows[:, 0].sum() == 0:
            continue                                       # (no position: the host bin loop has no answer)
        for k, w in enumerate((WIDTHS[i % 6], WIDTHS[(i // 6 + 1 + i) % 6])):
            na = NA[ncol][(i // 3 + k) % len(NA[ncol])]
            got, info = R.bin_(rows, w, na, info=True)
            _same(got, D.bin_observations(rows, w, na), ("bin", i, w, na))
            seen_w.add(w)
            n_second_clause += int(np.sum(info["chosen"] != info["first_max"]))
    assert seen_thin == set(THIN_PAIRS) and seen_w == set(WIDTHS) and seen_ncol == {4, 7, 10}
    assert n_second_clause > 20 and n_sa2_kept > 100 and n_sa2_thinned > 100, (n_second_clause, n_sa2_kept, n_sa2_thinned)


def test_the_oracle_equals_the_host_pipeline():
    from smcpp_amd import data as D
    for i in (7, 20, 45):
        rows = _input(i)
        if rows[:, 0].sum() == 0:
            rows[0, 0] = 5
        na = NA[rows.shape[1]][0]
        for thinning, w in ((7, 3), (2, 10), (100000, 64)):
            want = D.compress_repeated_obs(D.bin_observations(D.thin_data(rows, thinning), w, na))
            _same(R.pipeline(rows, thinning, w, na), want, (i, thinning, w))


def _expect(z, key, got):
    if key in z.files:
        _same(got, z[key], key)
        return
    assert tuple(z[key + "__shape"]) == got.shape, (key, got.shape, tuple(z[key + "__shape"]))
    assert np.array_equal(got[:500], z[key + "__head"]), key
    assert np.array_equal(got[-500:], z[key + "__tail"]), key
    assert zlib.crc32(got.tobytes()) == int(z[key + "__crc"]), key


def test_the_oracle_equals_the_reference_cython_golden():
    z = np.load(os.path.join(GOLDEN, "G23_estimation_tools.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    n = 0
    for inp in ("ex", "chr11", "twopop", "small", "zspan"):
        raw = np.ascontiguousarray(z[inp + "_in"], dtype=np.int32)
        a = [int(x) for x in z[inp + "_a"]]
        for key in names:
            if not key.startswith(inp + "_") or key.endswith(("_in", "_a")):
                continue
            op = key[len(inp) + 1:].split("_")
            if op[0] == "thin" and len(op) == 3:
                got = R.thin(raw, int(op[1]), int(op[2]))
            elif op[0] == "bin":
                got = R.bin_(raw, int(op[1]), a)
            elif op[0] == "thin400":
                got = R.bin_(R.thin(raw, 400, 0), 1000 if inp == "chr11" else 100, a)
            else:
                continue                                   # (realign / windowed_mutation_counts are not device steps)
            _expect(z, key, got)
            n += 1
    assert n >= 30


def test_the_coverage_counters():
    assert R.scan_plan(1) == (1, 1) and R.scan_plan(2048) == (1, 1) and R.scan_plan(2049) == (2, 1)
    assert R.scan_plan(2097152) == (1024, 1) and R.scan_plan(2097153) == (1025, 2) and R.scan_plan(4194305) == (2049, 3)
    counts = np.array([3, 0, 0, 600, 1, 0])
    f, l = R.emit_blocks(counts)
    assert f.tolist() == [0, 3, 3] and l.tolist() == [3, 3, 4]
    assert R.full_single_holder_blocks(counts) == 1 and R.zero_runs(counts) == 2 and R.zero_runs([1, 2]) == 0
    with pytest.raises(AssertionError):
        R.bin_(np.zeros((3, 4), np.int32), 2, [2])
