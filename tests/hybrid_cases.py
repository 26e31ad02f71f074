"""Inputs and cases of the hybrid rows' eigen-power step (chain family 6), shared by tests/test_hybrid_forms.py (the plan, from the
host hook) and tests/test_gpu_hybrid_forms.py (every form on the device against the C restatement).

A row longer than SMCPP_HYB_TH is one step P d^s P^-1 inside k_chain_ss; the step exists in several forms, chosen from the padded
state count Mp = 16 ceil(M / 16) and the number of eigen keys Ke (keys that occur in rows of span > 1).  Four tables per key take
4 Mp (Mp + 1) 8 bytes: ALL_TABLES while Ke of them fit 120 KB, DIRECTION_SPLIT while half of that fits 136 KB, else as many keys'
pairs as fit 136 KB stay in LDS and the least frequent - COLD - keys' table rows come from L2:

    Mp   per key   Ke = 1        Ke = 2        Ke = 3                 Ke = 4
    16    8.5 KB   all tables    all tables    all tables             all tables
    32   33   KB   all tables    all tables    all tables (99 KB)     direction split (66 KB)
    48   73.5 KB   all tables    dir. split    dir. split (110 KB)    cold: 136 / 36.75 = 3 in LDS, 1 from L2
    64  130   KB   dir. split    dir. split    cold: 136 / 65 = 2, 1  cold: 2 in LDS, 2 from L2

Ke = 5 leaves the hybrid plan.  FORMS below is that table, written out; nothing here calls back into the rule.
"""
import numpy as np

ALL, SPLIT, COLD = "all tables", "direction split", "direction split, cold keys"
# (Mp, Ke) -> (form, tables_in_lds)
FORMS = {(16, 1): (ALL, 1), (16, 2): (ALL, 2), (16, 3): (ALL, 3), (16, 4): (ALL, 4),
         (32, 1): (ALL, 1), (32, 2): (ALL, 2), (32, 3): (ALL, 3), (32, 4): (SPLIT, 4),
         (48, 1): (ALL, 1), (48, 2): (SPLIT, 2), (48, 3): (SPLIT, 3), (48, 4): (COLD, 3),
         (64, 1): (SPLIT, 1), (64, 2): (SPLIT, 2), (64, 3): (COLD, 2), (64, 4): (COLD, 2)}

TH = (6, 40)                 # the thresholds whose two sides every input holds rows of (SMCPP_HYB_TH: 6 is the default)
LONGEST = 100_000
CHUNK_ROWS = 200             # set_chunking: a dozen chunks on the long contig, three or four on the short one
THETA_BP, RHO_BP = 4.02e-4, 1e-4          # per base pair, as test_config_c1_reference_example_end_to_end has them
W4 = (0.55, 0.25, 0.13, 0.07)             # how often a long row takes the first, second, ... eigen key
W5 = (0.40, 0.25, 0.15, 0.12, 0.08)


def eigen_key_list(n, count):
    """Realistic keys of long rows: monomorphic, missing, monomorphic on a reduced sample (n - 2, n - 4; n - 6: the fifth key)."""
    return [(0, 0, n), (-1, 0, 0), (0, 0, n - 2), (0, 0, n - 4), (0, 0, n - 6)][:count]


def key_list(n, eigen_keys, n_keys):
    """The eigen keys, then segregating-site keys (a, b, nb) of the full sample and, where more are asked for, of smaller ones."""
    keys = list(eigen_keys)
    for nb in range(n, 1, -1):
        for a in (0, 1):
            for b in range(1 - a, nb + 1):
                if len(keys) < n_keys and (a, b, nb) not in keys:
                    keys.append((a, b, nb))
    assert len(keys) == n_keys, (len(keys), n_keys)
    return keys


def unbinned(seed, M, n, eigen_keys, weights, n_keys=20, th=TH):
    """Three ragged contigs of un-binned rows (span, a, b, nb): about 2 500 rows, about 700 rows, 1 row.  45 % of the rows have span 1,
    keys from the whole list; the others 1 + geometric(3e-3) positions (at most 10^5) and one of `eigen_keys`, drawn with `weights`,
    so no other key ever has span > 1.  By hand: for every eigen key and every threshold of `th` a row of span th and one of th + 1,
    and one row of 10^5 - near the head of the long contig (the 10^5 rows), near its tail (the threshold rows) and inside the short
    one (all of them); the one-row contig is a 10^5 row of the rarest eigen key."""
    rng = np.random.default_rng([seed, M, n, len(eigen_keys)])
    keys = np.array(key_list(n, eigen_keys, n_keys), dtype=np.int32)
    ke = len(eigen_keys)
    w = np.asarray(weights, dtype=float)
    assert len(w) == ke and abs(w.sum() - 1.0) < 1e-12
    contigs = []
    for L in (2500 + int(rng.integers(0, 37)), 700 + int(rng.integers(0, 23))):
        kid = rng.integers(0, len(keys), L)
        span = np.where(rng.random(L) < 0.45, 1, np.minimum(LONGEST, 1 + rng.geometric(3e-3, L)))
        kid[span > 1] = rng.choice(ke, size=int((span > 1).sum()), p=w)
        hand = [(e, s) for e in range(ke) for t in th for s in (t, t + 1)]
        head = [(e, LONGEST) for e in range(ke)]
        at_tail = L - 3 - 2 * np.arange(len(hand))                 # every other row, so that span-1 rows stay between them
        at_head = 3 + 2 * np.arange(len(head)) if L > 1000 else L // 2 + 2 * np.arange(len(head))
        for pos, (e, s) in list(zip(at_tail, hand)) + list(zip(at_head, head)):
            kid[pos], span[pos] = e, s
        contigs.append(np.ascontiguousarray(np.concatenate([span[:, None], keys[kid]], axis=1), dtype=np.int32))
    rare = int(np.argmin(w))
    contigs.append(np.array([[LONGEST, *keys[rare]]], dtype=np.int32))
    return contigs


def eigen_index(eigen_keys):
    """The engine's index of every eigen key: its rank among the eigen keys in the key list's (lexicographic) order."""
    order = sorted(eigen_keys)
    return [order.index(k) for k in eigen_keys]


def rotate(w, r):
    return tuple(w[(i - r) % len(w)] for i in range(len(w)))


# case number -> (M, Ke, n, n_keys, weightings).  Every weighting is one input; position i of a weighting belongs to eigen_key_list[i].
# 5: each eigen key the hot one once; 10 and 13: each eigen key the cold one once; 14: two disjoint cold pairs; 12: more keys than
# emission slots beside the tables (n = 10, 64 keys)
CASES = {1: (2, 1, 8, 20, [(1.0,)]),
         2: (7, 2, 8, 20, [(0.7, 0.3)]),
         3: (16, 4, 8, 20, [W4]),
         4: (17, 1, 8, 20, [(1.0,)]),
         5: (32, 3, 8, 20, [rotate((0.6, 0.27, 0.13), r) for r in range(3)]),
         6: (29, 4, 8, 20, [W4]),
         7: (33, 1, 8, 20, [(1.0,)]),
         8: (48, 2, 8, 20, [(0.7, 0.3)]),
         9: (40, 3, 8, 20, [(0.6, 0.27, 0.13)]),
         10: (48, 4, 8, 20, [rotate(W4, r) for r in range(4)]),
         11: (49, 1, 8, 20, [(1.0,)]),
         12: (64, 2, 10, 64, [(0.7, 0.3)]),
         13: (57, 3, 8, 20, [rotate((0.6, 0.27, 0.13), r) for r in range(3)]),
         14: (64, 4, 8, 20, [W4, rotate(W4, 2)]),
         15: (64, 5, 8, 20, [W5])}
INPUTS = [(c, r) for c, v in CASES.items() for r in range(len(v[4]))]
SEEDS = {}                   # (case, weighting) -> seed, where the default (100 case + weighting) did not meet the conditions on the input


def case_input(case, r=0):
    """-> dict: M, Mp, n, Ke, eigen keys, weights, contigs, the expected form / tables_in_lds / cold and hot eigen-key indices."""
    M, ke, n, n_keys, ws = CASES[case]
    ek = eigen_key_list(n, ke)
    w = ws[r]
    Mp = 16 * ((M + 15) // 16)
    contigs = unbinned(SEEDS.get((case, r), 100 * case + r), M, n, ek, w, n_keys)
    idx = eigen_index(ek)
    by_weight = sorted(range(ke), key=lambda i: -w[i])
    form, in_lds = FORMS.get((Mp, ke), (None, 0))
    cold = sorted(idx[i] for i in by_weight[in_lds:]) if form else []
    return dict(case=case, rotation=r, M=M, Mp=Mp, n=n, Ke=ke, eigen_keys=ek, weights=w, contigs=contigs, keys=key_list(n, ek, n_keys),
                form=form, tables_in_lds=in_lds, cold=cold, hot=idx[by_weight[0]] if form and Mp == 32 else -1,
                rarest=ek[by_weight[-1]], most=ek[by_weight[0]])


def long_rows(contig, key, th):
    """Indices of the rows of `key` whose span exceeds `th`."""
    return np.nonzero((contig[:, 0] > th) & np.all(contig[:, 1:] == np.asarray(key, dtype=contig.dtype), axis=1))[0]


def with_key_swapped(contigs, rarest, most, th=TH[0]):
    """The sensitivity input: the rarest eigen key's long rows carry the most frequent eigen key's key instead."""
    out = []
    for c in contigs:
        c = c.copy()
        c[long_rows(c, rarest, th), 1:] = most
        out.append(c)
    return out
