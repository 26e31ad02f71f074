"""Recipes, contigs built by count and forms of the statistics phase, shared by tests/test_gpu_stats_edges.py (every form on the device
against the C restatement), tests/test_stats_plan.py (the plan and the layout, from the host hook) and tools/record_stats_plans.py
(the recorded table tests/stats_plans.json).  tests/test_gpu_stats_edges.py's docstring says which edge every count places.
"""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------------------
# contigs built by count
# ---------------------------------------------------------------------------------------------------------------------------------
# observation triples (a, b, nb) valid for n = 8 undistinguished haplotypes; span > 1 rows carry "mono" and "miss" only
KEYS1 = dict(p0=(0, 1, 8), p1=(0, 3, 8), p2=(1, 0, 8), p3=(1, 2, 8), p4=(0, 7, 8), p5=(1, 0, 0), mono=(0, 0, 0), miss=(-1, 0, 0))
# ... and for the two-population manager of test_gpu_gamma._twopop (n1 = 4, n2 = 3, a = (2, 0))
KEYS2 = dict(p0=(0, 1, 4, 0, 0, 3), p1=(1, 0, 4, 0, 1, 3), p2=(0, 2, 4, 0, 2, 3), p3=(1, 1, 4, 0, 0, 3), p4=(0, 3, 4, 0, 1, 3),
             p5=(1, 0, 0, 0, 0, 0), mono=(0, 0, 0, 0, 0, 0), miss=(-1, 0, 0, 0, 0, 0))

ONES = dict([((s, "mono"), 1) for s in range(2, 41)] + [((s, "miss"), 1) for s in range(2, 21)])      # 58 groups of one row
# (label, span-1 rows per key, rows per (span, key) group)
EDGE = [
    ("n1=0", {}, {(2, "mono"): 5, (3, "miss"): 3}),
    ("n1=1", dict(p0=1), {(31, "mono"): 1}),
    ("n1=2", dict(p1=1, p2=1), {(2, "miss"): 4}),
    ("n1=3", dict(p0=3), {}),
    ("n1=4", dict(p1=4), {(63, "mono"): 3}),
    ("n1=5", dict(p2=5), {(64, "miss"): 1, (64, "mono"): 1}),
    ("n1=15", dict(p0=4, p1=4, p2=4, p3=3), {(2, "mono"): 15}),
    ("n1=16", dict(p4=8, p2=8), {(3, "mono"): 16, (3, "miss"): 17}),
    ("n1=17", dict(p5=17), {(2, "miss"): 17}),
    ("n1=63", dict(p0=15, p1=16, p2=17, p3=5, p4=4, p5=3, mono=3), {(31, "mono"): 31, (31, "miss"): 32}),
    ("n1=64", dict(p0=16, p1=16, p2=16, p3=16), {(2, "mono"): 33}),
    ("n1=65", dict(p0=17, p1=17, p2=17, p3=14), ONES),
    ("n1=127", dict(p0=25, p1=25, p2=25, p3=25, mono=27), {(2, "mono"): 127}),
    ("n1=128", dict(p1=64, p2=64), {(3, "miss"): 128}),
    ("n1=129", dict(p0=43, p1=43, p2=43), {(2, "miss"): 129, (63, "mono"): 5}),
    ("n1=143", dict(p0=36, p1=36, p2=36, p3=35), {(64, "mono"): 15, (64, "miss"): 16}),
    ("n1=144", dict(p4=72, p5=72), {(63, "miss"): 17}),
    ("n1=145", dict(p5=145), {}),
    ("n1=511", dict(p2=255, mono=256), {(3, "mono"): 129}),
    ("n1=512", dict(p2=255, p5=257), {(2, "mono"): 128, (31, "miss"): 4}),
    ("n1=513", dict(p4=256, p5=257), {(5, "mono"): 16, (7, "miss"): 31}),
]
_BY_LABEL = {r[0]: r for r in EDGE}
ONE = [_BY_LABEL["n1=63"]]
TWO = [_BY_LABEL["n1=513"], _BY_LABEL["n1=0"]]
NO_GT1 = [(lb + ", span 1 only", s1, {}) for lb, s1, _ in (_BY_LABEL["n1=3"], _BY_LABEL["n1=145"], _BY_LABEL["n1=63"], _BY_LABEL["n1=129"])]
TWOPOP = [
    ("n1=0", {}, {(2, "mono"): 5, (3, "miss"): 3}),
    ("n1=3", dict(p0=3), {}),
    ("n1=17", dict(p1=17), {(31, "mono"): 1, (2, "miss"): 17}),
    ("n1=65", dict(p0=17, p1=17, p2=17, p3=14), {(64, "mono"): 16, (63, "miss"): 15}),
    ("n1=129", dict(p2=43, p4=43, p5=43), {(2, "mono"): 33}),
    ("n1=257", dict(p3=257), {(3, "mono"): 129}),
]
KINDS = dict(edge=(EDGE, KEYS1), one=(ONE, KEYS1), two=(TWO, KEYS1), no_gt1=(NO_GT1, KEYS1), twopop=(TWOPOP, KEYS2),
             unstructured=(EDGE, KEYS1))

# the counts the edges above need (span-1 rows per contig / per (contig, key) / rows per (contig, span, key) group, spans)
WANT_N1 = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 143, 144, 145, 511, 512, 513}
WANT_N1_KEY = {0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257}
WANT_GROUP = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129}
WANT_SPANS = {2, 3, 31, 63, 64}
MAX_POSITIONS, MAX_ROWS = 20_000, 60_000


def _rotation(counts):
    """counts: {name: n} -> the names, one of each in turn until every count is used up (a deterministic interleaving)."""
    left = dict(counts)
    out = []
    while any(left.values()):
        for name in counts:
            if left[name] > 0:
                out.append(name)
                left[name] -= 1
    return out


def _build(recipe, keytab):
    """One contig from (label, span-1 rows per key, rows per (span, key) group).  The span > 1 rows are spread evenly over the gaps
    between the span-1 rows: first and last row are of span 1 when the contig has two span-1 rows or more; with one, it comes first;
    with none, the contig consists of span > 1 rows."""
    _, s1, gt1 = recipe
    ones = [(1,) + tuple(keytab[k]) for k in _rotation(s1)]
    longs = [(g[0],) + tuple(keytab[g[1]]) for g in _rotation(gt1)]
    n1, ne = len(ones), len(longs)
    if n1 <= 1:
        rows = ones + longs
    else:
        gap = [[] for _ in range(n1 - 1)]
        for j, r in enumerate(longs):
            gap[j * (n1 - 1) // ne].append(r)
        rows = [ones[0]]
        for i in range(1, n1):
            rows += gap[i - 1]
            rows.append(ones[i])
    return np.ascontiguousarray(np.array(rows, dtype=np.int32))


def _counted(contig, keytab):
    """-> (span-1 rows per key name, rows per (span, key name) group), counted from the rows."""
    names = {tuple(v): k for k, v in keytab.items()}
    s1, gt1 = {}, {}
    for r in contig.tolist():
        nm = names[tuple(r[1:])]
        if r[0] == 1:
            s1[nm] = s1.get(nm, 0) + 1
        else:
            gt1[(r[0], nm)] = gt1.get((r[0], nm), 0) + 1
    return s1, gt1


_CONTIGS = {}


def _contigs(kind):
    """The contigs of a kind, each verified against its recipe: the counts are present in what was built."""
    if kind not in _CONTIGS:
        recipes, keytab = KINDS[kind]
        out = []
        for rc in recipes:
            c = _build(rc, keytab)
            s1, gt1 = _counted(c, keytab)
            assert s1 == {k: v for k, v in rc[1].items() if v} and gt1 == dict(rc[2]), (rc[0], s1, gt1)
            assert int(c[:, 0].sum()) <= MAX_POSITIONS, (rc[0], int(c[:, 0].sum()))
            if len(s1) and sum(s1.values()) >= 2:
                assert c[0, 0] == 1 and c[-1, 0] == 1, rc[0]
            out.append(c)
        assert sum(len(c) for c in out) <= MAX_ROWS
        _CONTIGS[kind] = out
    return _CONTIGS[kind]


# ---------------------------------------------------------------------------------------------------------------------------------
# forms
# ---------------------------------------------------------------------------------------------------------------------------------
S16 = {"SMCPP_SLAB_ROWS": "16"}
FOLD = "fold on the scans"


def _forms(M):
    """name -> (switches, save_gamma, expected describe()["statistics"] fields, eigen_free_statistics)."""
    f = {}
    if M <= 64:
        f["default"] = ({}, False, dict(span1_form="one pass", rank_update="teams", eigen=FOLD), True)
        f["two_kernels"] = ({"SMCPP_S1_FUSE": "0"}, False, dict(span1_form="two kernels", rank_update="teams", eigen=FOLD), True)
        f["per_slab"] = ({"SMCPP_STATS_TEAM": "0"}, False, dict(span1_form="one pass", rank_update="per slab", eigen=FOLD), True)
        f["two_kernels_per_slab"] = ({"SMCPP_S1_FUSE": "0", "SMCPP_STATS_TEAM": "0"}, False,
                                     dict(span1_form="two kernels", rank_update="per slab", eigen=FOLD), True)
        f["eigensystem"] = ({"SMCPP_EIGFREE": "0"}, False, dict(span1_form="two kernels", rank_update="teams", eigen="generation 2"), False)
        crossed = ("default", "two_kernels", "per_slab", "two_kernels_per_slab", "eigensystem")
    elif M <= 128:
        f["default"] = ({}, False, dict(span1_form="two kernels", rank_update="teams", eigen=FOLD), True)
        f["per_slab"] = ({"SMCPP_STATS_TEAM": "0"}, False, dict(span1_form="two kernels", rank_update="per slab", eigen=FOLD), True)
        f["eigensystem"] = ({"SMCPP_EIGFREE": "0"}, False, dict(span1_form="two kernels", rank_update="teams", eigen="classic"), False)
        crossed = ("default", "per_slab", "eigensystem")
    else:
        f["default"] = ({}, False, dict(span1_form="two kernels", rank_update="wide", eigen=FOLD), True)
        f["wide_no_teams"] = ({"SMCPP_STATS_TEAM": "0"}, False, dict(span1_form="two kernels", rank_update="wide", eigen=FOLD), True)
        f["narrow"] = ({"SMCPP_RANK_WIDE": "0"}, False, dict(span1_form="two kernels", rank_update="teams", eigen=FOLD), True)
        f["per_slab"] = ({"SMCPP_RANK_WIDE": "0", "SMCPP_STATS_TEAM": "0"}, False,
                         dict(span1_form="two kernels", rank_update="per slab", eigen=FOLD), True)
        f["eigensystem"] = ({"SMCPP_EIGFREE": "0"}, False, dict(span1_form="two kernels", rank_update="wide", eigen="classic"), False)
        crossed = ("default", "narrow", "per_slab", "eigensystem")
    f["matrix_core_fold"] = ({"SMCPP_SPAN_SCAN": "0"}, False, dict(f["default"][2], eigen="fold on the matrix cores"), True)
    f["save_gamma"] = ({}, True, dict(f["default"][2], span1_form="two kernels", per_row_gamma="scan steps"), True)
    for name in crossed:
        sw, sg, want, ef = f[name]
        f[name + "_slab16"] = (dict(sw, **S16), sg, want, ef)
    return f


MS = (13, 48, 64, 80, 144)
