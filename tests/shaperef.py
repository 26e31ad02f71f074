"""A vectorised NumPy statement of the pre-HMM data shaping (thin / bin / compress), the oracle of tests/test_gpu_shaping_edges.py.

Defined from POSITIONS, not from the carried counters of the reference's loops (`smcpp_amd.data.thin_data` / `bin_observations`, which
tests/test_shaperef.py pins it to bit for bit) and not from the per-row geometry of smcpp_amd/csrc/shaping.hpp (`ThinGeom`):

  thin      with offset < thinning the 1-based position p is KEPT iff (offset + p) % thinning == 0.  The contig (0, P] is cut at every
            row end and on both sides of every kept position; a piece that is a kept position is a span-1 row with the full
            observation of the row it lies in, every other piece keeps (a, 0, 0) per population; rows with sum a == 2 are written as
            all zeros in both kinds of piece.  offset >= thinning: no position is kept.  Rows of span 0 own no position: nothing.
  bin       bin k = positions [k w, (k + 1) w); its rows = the rows with a positive overlap, in order.  Over the (bin, row) pairs -
            which are sorted by bin when listed row by row - the reference's running rule (`_estimation_tools.pyx:113-143`: a new
            strict maximum of the sample size takes over; while the maximum is 2 a row with exactly one derived distinguished allele
            takes over) is a segmented running maximum plus "the last pair of the bin at which something took over".
  compress  `smcpp_amd.data.compress_repeated_obs` is vectorised already and is the oracle.

The same functions return what the device tests assert about their own inputs (`info=True`): the source row of every output, which
outputs are kept positions, the rows per bin, where the second clause of the rule decided; `scan_plan` and `emit_blocks` restate the
launch geometry of the device scan (2048 items per block, one 1024-thread block over the block sums) and of the emit kernels (256
outputs per block).
"""
import numpy as np

from smcpp_amd import data as D

SCAN_TILE = 2048          # items per block of the device scan (shaping.hpp: SCAN_BLOCK * SCAN_ITEMS)
EMIT_BLOCK = 256          # outputs per block of the emit kernels


def _rows(data):
    data = np.ascontiguousarray(data, dtype=np.int32)
    assert data.ndim == 2 and data.shape[1] >= 4 and (data.shape[1] - 1) % 3 == 0, data.shape
    return data


def positions(data):
    """(start, end) of every row, int64: the row covers the 1-based positions start + 1 .. end."""
    end = np.cumsum(_rows(data)[:, 0], dtype=np.int64)
    return end - data[:, 0], end


def thin(data, thinning, offset=0, info=False):
    data = _rows(data)
    ncol = data.shape[1]
    thinning, offset = int(thinning), int(offset)
    assert thinning > 0 and offset >= 0
    start, end = positions(data)
    P = int(end[-1]) if len(end) else 0
    kept_pos = np.arange(thinning - offset, P + 1, thinning, dtype=np.int64) if offset < thinning else np.zeros(0, np.int64)
    cuts = np.unique(np.concatenate((np.zeros(1, np.int64), end, kept_pos, kept_pos - 1)))
    hi = cuts[1:]
    src = np.searchsorted(end, hi, side="left")                 # the row that holds position hi (rows of span 0 hold none)
    kept = (offset + hi) % thinning == 0 if offset < thinning else np.zeros(len(hi), bool)
    out = np.zeros((len(hi), ncol), dtype=np.int32)
    out[:, 0] = hi - cuts[:-1]
    if len(hi):
        assert np.all(out[kept, 0] == 1) and np.all(start[src] < hi) and np.all(hi <= end[src])
        rows = data[src]
        out[:, 1::3] = rows[:, 1::3]
        out[kept, 2::3] = rows[kept, 2::3]
        out[kept, 3::3] = rows[kept, 3::3]
        out[rows[:, 1::3].sum(axis=1) == 2, 1:] = 0
    if not info:
        return out
    return out, {"src": src, "kept": kept, "counts": np.bincount(src, minlength=len(data)), "P": P}


def bin_(data, w, na, info=False):
    data = _rows(data)
    w = int(w)
    na = np.asarray(na, dtype=np.int64)
    assert w > 0 and len(na) == (data.shape[1] - 1) // 3
    start, end = positions(data)
    P = int(end[-1])
    assert P > 0, "the reference has no answer for a contig without positions"
    nbins = -(-P // w)
    nz = np.flatnonzero(end > start)
    first, last = start[nz] // w, (end[nz] - 1) // w
    cnt = last - first + 1
    off = np.cumsum(cnt) - cnt
    row = np.repeat(nz, cnt)                                     # the (bin, row) pairs, row by row: sorted by bin, rows in order
    b = np.repeat(first - off, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    assert np.all(b[1:] >= b[:-1]) and b[0] == 0 and b[-1] == nbins - 1
    a_nz = data[nz, 1::3].astype(np.int64)
    ss = (data[nz, 3::3].astype(np.int64).sum(axis=1) + ((a_nz >= 0) * na[None, :]).sum(axis=1))
    seg = np.maximum(a_nz, 0).sum(axis=1)
    assert ss.min() > -2
    inv = np.repeat(np.arange(len(nz)), cnt)
    ss, seg = ss[inv], seg[inv]
    K = int(ss.max()) + 3
    run = np.maximum.accumulate(b * K + (ss + 2)) - b * K - 2    # running maximum of the sample size inside the bin, this pair included
    new_bin = np.concatenate(([True], b[1:] != b[:-1]))
    prev = np.where(new_bin, -2, np.concatenate(([0], run[:-1])))
    higher = ss > prev
    take = higher | ((run == 2) & (seg == 1))
    last_of_bin = np.concatenate((b[1:] != b[:-1], [True]))

    def last_marked(mark):
        idx = np.flatnonzero(mark)
        idx = idx[np.concatenate((b[idx][1:] != b[idx][:-1], [True]))]
        assert np.array_equal(b[idx], np.arange(nbins))
        return row[idx]
    chosen = last_marked(take)
    out = data[chosen].copy()
    out[:, 0] = 1
    if not info:
        return out
    return out, {"chosen": chosen, "first_max": last_marked(higher), "rows_per_bin": np.bincount(b, minlength=nbins), "P": P,
                 "nbins": nbins, "first_row": row[new_bin], "last_row": row[last_of_bin]}


def compress(data, info=False):
    data = _rows(data)
    out = D.compress_repeated_obs(data)
    if not info:
        return out
    head = np.ones(len(data), bool)
    head[1:] = np.any(data[1:, 1:] != data[:-1, 1:], axis=1)
    return out, {"heads": np.flatnonzero(head), "counts": head.astype(np.int64)}


def pipeline(data, thinning, w, na):
    return compress(bin_(thin(data, thinning, 0), w, na))


def scan_plan(n):
    """(nb, per) of the device scan over n items: nb blocks of 2048 items, each of the 1024 threads of the second kernel sums `per`
    block sums."""
    nb = max(1, -(-int(n) // SCAN_TILE))
    return nb, -(-nb // 1024)


def emit_blocks(counts):
    """For the outputs that `counts[i]` per item produce: (first, last) holder of every emit block of 256 outputs."""
    counts = np.asarray(counts, dtype=np.int64)
    cum = np.cumsum(counts)
    nout = int(cum[-1]) if len(cum) else 0
    o_first = np.arange(0, nout, EMIT_BLOCK, dtype=np.int64)
    o_last = np.minimum(o_first + EMIT_BLOCK - 1, nout - 1)
    return np.searchsorted(cum, o_first, side="right"), np.searchsorted(cum, o_last, side="right")


def full_single_holder_blocks(counts):
    """Number of emit blocks whose 256 threads all find the same holder."""
    f, l = emit_blocks(counts)
    nout = int(np.sum(counts))
    full = np.arange(len(f)) < nout // EMIT_BLOCK
    return int(np.sum((f == l) & full))


def zero_runs(counts):
    """Length of the longest run of items that produce no output."""
    z = np.concatenate(([0], (np.asarray(counts) == 0).astype(np.int64), [0]))
    d = np.flatnonzero(np.diff(z))
    return int((d[1::2] - d[0::2]).max()) if len(d) else 0


def random_rows(rng, L, ncol, spans=(0, 1, 1, 1, 2, 3, 7, 50, 400), p_nb0=0.25, max_run=1):
    """Seeded rows: spans drawn from `spans`, a in -1..2, b in 0..2, nb in 0..3 (nb = 0 with probability at least p_nb0: the bins in
    which only the distinguished pair is observed are the ones the second clause of the bin rule decides); `max_run` > 1 repeats
    observations in runs of 1..max_run rows (compress)."""
    npop = (ncol - 1) // 3
    n = L
    obs = np.zeros((n, ncol), dtype=np.int32)
    obs[:, 1::3] = rng.integers(-1, 3, (n, npop))
    obs[:, 2::3] = rng.integers(0, 3, (n, npop))
    obs[:, 3::3] = rng.integers(0, 4, (n, npop)) * (rng.random((n, npop)) >= p_nb0)
    if max_run > 1:
        obs = np.repeat(obs, rng.integers(1, max_run + 1, n), axis=0)[:L]
    obs[:, 0] = np.asarray(spans, dtype=np.int32)[rng.integers(0, len(spans), L)]
    return np.ascontiguousarray(obs)
